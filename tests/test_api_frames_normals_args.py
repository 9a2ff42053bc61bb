"""The many-frames calls of the second engine without a device: the exports, the refusals of the C-ABI that need no context or no
device (null arguments, negative counts, a stride below 3, offsets that do not start at 0 or decrease), n_frames == 0, and the arguments
the Context methods check before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

NEW = ("dcreg_register_frames_normals", "dcreg_icp_run_trials_normals", "dcreg_normals_reserve_slots", "dcreg_normals_reset_slot",
       "dcreg_normals_batch_begin", "dcreg_normals_batch_end")
FP, I64P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
I4 = np.eye(4)


def _frames(n=3, pts=4):
    xyz = np.zeros((n * pts, 3), np.float32)
    off = np.arange(n + 1, dtype=np.int64) * pts
    R0 = np.tile(np.eye(3).reshape(9), (n, 1))
    t0 = np.zeros((n, 3))
    return xyz, off, R0, t0


def _register(L, ctx, n, xyz, off, stride, R0, t0, cfg, res):
    return L.dcreg_register_frames_normals(ctx, n, None if xyz is None else xyz.ctypes.data_as(FP), None if off is None else off.ctypes.data_as(I64P),
                                           stride, None if R0 is None else api._dp(R0), None if t0 is None else api._dp(t0), 0, 0,
                                           None if cfg is None else C.byref(cfg), 0, res)


def test_every_symbol_is_exported_and_no_struct_moved():
    L = api.load()
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name, cls in (("dcreg_trial_result", api.TrialResult), ("dcreg_lin_out", api.LinOut), ("dcreg_lin_params", api.LinParams)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    xyz, off, R0, t0 = _frames()
    cfg, q = api.default_config(), api.default_lin_params(0.5)
    res = (api.TrialResult * 3)()
    outs = (api.LinOut * 3)()
    ids = np.zeros(3, np.int32)
    assert _register(L, None, 3, xyz, off, 3, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, None, 0, xyz, off, 3, R0, t0, cfg, res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_normals(None, 3, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), res) == api.E_INVALID
    assert L.dcreg_normals_reserve_slots(None, 4, 1) == api.E_INVALID
    assert L.dcreg_normals_reset_slot(None, 0) == api.E_INVALID
    assert L.dcreg_normals_batch_begin(None, 0, 3, api._dp(R0), api._dp(t0), ids.ctypes.data_as(I32P), ids.ctypes.data_as(I32P), C.byref(q)) == api.E_INVALID
    assert L.dcreg_normals_batch_end(None, 0, outs) == api.E_INVALID
    assert all(r.iterations == 0 and r.status == 0 for r in res) and outs[0].n_eff == 0


def test_argument_refusals_that_need_no_device():
    """the checks of dcreg_register_frames_normals come before the context is looked at: any non-null handle serves"""
    L = api.load()
    xyz, off, R0, t0 = _frames()
    cfg = api.default_config()
    res = (api.TrialResult * 3)()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # never dereferenced by the refusals below
    assert _register(L, fake, -1, xyz, off, 3, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, fake, 3, xyz, off, 2, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, fake, 3, xyz, off, 3, R0, t0, None, res) == api.E_INVALID
    assert _register(L, fake, 3, xyz, None, 3, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, fake, 3, xyz, off, 3, None, t0, cfg, res) == api.E_INVALID
    assert _register(L, fake, 3, xyz, off, 3, R0, None, cfg, res) == api.E_INVALID
    assert _register(L, fake, 3, xyz, off, 3, R0, t0, cfg, None) == api.E_INVALID
    # n_frames == 0 does nothing, whatever else is passed
    assert _register(L, fake, 0, None, None, 3, None, None, cfg, None) == api.OK
    assert L.dcreg_icp_run_trials_normals(fake, 0, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), res) == api.OK
    assert L.dcreg_icp_run_trials_normals(fake, -1, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_normals(fake, 3, None, api._dp(t0), 0, 0, C.byref(cfg), res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_normals(fake, 3, api._dp(R0), api._dp(t0), 0, 0, None, res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_normals(fake, 3, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), None) == api.E_INVALID
    assert all(r.iterations == 0 and r.status == 0 for r in res)


class _Ctx(C.Structure):
    """the head of a context as far as dcreg_set_error_message writes: room for the whole object is what matters here"""
    _fields_ = [("bytes", C.c_char * (1 << 16))]


def test_offsets_must_start_at_zero_and_not_decrease():
    """these two refusals leave their text in the context (dcreg_last_error): a zeroed block of memory stands in for one"""
    L = api.load()
    xyz, off, R0, t0 = _frames()
    cfg = api.default_config()
    res = (api.TrialResult * 3)()
    blob = _Ctx()
    ctx = C.c_void_p(C.addressof(blob))
    L.dcreg_last_error.restype = C.c_char_p
    late = off + 1
    assert _register(L, ctx, 3, xyz, late, 3, R0, t0, cfg, res) == api.E_INVALID
    assert b"start at 0" in L.dcreg_last_error(ctx)
    down = np.array([0, 8, 4, 12], np.int64)
    assert _register(L, ctx, 3, xyz, down, 3, R0, t0, cfg, res) == api.E_INVALID
    assert b"decrease" in L.dcreg_last_error(ctx)
    assert all(r.iterations == 0 and r.status == 0 for r in res)


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_the_methods_check_frames_poses_and_method():
    c = _ctx()
    cfg = api.default_config()
    f = [np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32)]
    with pytest.raises(ValueError, match="one initial pose per frame"):
        c.register_frames_normals(f, [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="float32"):
        c.register_frames_normals([np.zeros((4, 3))], [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="columns"):
        c.register_frames_normals([f[0], np.zeros((4, 4), np.float32)], [I4, I4], "Ours", cfg)
    with pytest.raises(ValueError, match="method"):
        c.register_frames_normals(f, [I4, I4], "XICP", cfg)
    with pytest.raises(ValueError, match="method"):
        c.icp_run_trials_normals([I4], "XICP", cfg)
    euler = api.default_lin_params(0.5, euler_rpy=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="parameterization"):
        c.normals_batch_begin([I4], params=euler)
    p = api.default_lin_params(0.5)
    p.search_radius = np.nan
    with pytest.raises(ValueError, match="search_radius"):
        c.normals_batch_begin([I4], params=p)
