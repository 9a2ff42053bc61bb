"""The fourth engine's many-frames calls without a device: the exports, the refusals of the C-ABI that need no context or no device (null
arguments, a stride below 3, negative counts, offsets that do not start at 0 or decrease), n_frames == 0 / n_trials == 0, what the batched
seam refuses before it looks at the device, and the arguments the Context methods check before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

NEW = ("dcreg_voxels_batch_begin", "dcreg_voxels_batch_end", "dcreg_register_frames_voxels", "dcreg_icp_run_trials_voxels")
FP, I64P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
I4 = np.eye(4)


class _Ctx(C.Structure):
    """a zeroed block of memory stands in for a context: the refusals below leave their text in it and look at nothing else (its
    "voxels_source_cov" reads 0: frame_normals is not looked at)"""
    _fields_ = [("bytes", C.c_char * (1 << 16))]


def _frames(n=3, pts=4):
    xyz = np.zeros((n * pts, 3), np.float32)
    off = np.arange(n + 1, dtype=np.int64) * pts
    R0 = np.tile(np.eye(3).reshape(9), (n, 1))
    t0 = np.zeros((n, 3))
    return xyz, off, R0, t0


def _register(L, ctx, n, xyz, off, stride, prm, R0, t0, cfg, res):
    return L.dcreg_register_frames_voxels(ctx, n, None if xyz is None else xyz.ctypes.data_as(FP), None if off is None else off.ctypes.data_as(I64P),
                                          stride, None if prm is None else C.byref(prm), None if R0 is None else api._dp(R0),
                                          None if t0 is None else api._dp(t0), 0, 0, None if cfg is None else C.byref(cfg), 0, res)


def _trials(L, ctx, n, R0, t0, cfg, res):
    return L.dcreg_icp_run_trials_voxels(ctx, n, None if R0 is None else api._dp(R0), None if t0 is None else api._dp(t0), 0, 0,
                                         None if cfg is None else C.byref(cfg), res)


def test_every_symbol_is_exported_and_no_struct_moved():
    L = api.load()
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name, cls in (("dcreg_trial_result", api.TrialResult), ("dcreg_lin_out", api.LinOut), ("dcreg_lin_params", api.LinParams),
                      ("dcreg_normal_params", api.NormalParams), ("dcreg_normal_info", api.NormalInfo), ("dcreg_config", api.Config)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    xyz, off, R0, t0 = _frames()
    cfg, q, prm = api.default_config(), api.default_lin_params(0.5), api.normal_params()
    res = (api.TrialResult * 3)()
    outs = (api.LinOut * 3)()
    ids = np.zeros(3, np.int32)
    for n in (3, 0):
        for p in (prm, None):
            assert _register(L, None, n, xyz, off, 3, p, R0, t0, cfg, res) == api.E_INVALID
        assert _trials(L, None, n, R0, t0, cfg, res) == api.E_INVALID
    for fids in (None, ids.ctypes.data_as(I32P)):
        assert L.dcreg_voxels_batch_begin(None, 0, 3, api._dp(R0), api._dp(t0), fids, C.byref(q)) == api.E_INVALID
    assert L.dcreg_voxels_batch_end(None, 0, outs) == api.E_INVALID
    assert all(r.iterations == 0 and r.status == 0 for r in res) and outs[0].n_eff == 0


def test_argument_refusals_that_need_no_device():
    L = api.load()
    L.dcreg_last_error.restype = C.c_char_p
    xyz, off, R0, t0 = _frames()
    cfg, prm = api.default_config(), api.normal_params()
    res = (api.TrialResult * 3)()
    blob = _Ctx()
    ctx = C.c_void_p(C.addressof(blob))
    # ---- dcreg_register_frames_voxels (mode 0: frame_normals may be null, and is not the reason for any of these)
    for p in (prm, None):
        assert _register(L, ctx, -1, xyz, off, 3, p, R0, t0, cfg, res) == api.E_INVALID
        assert _register(L, ctx, 3, xyz, off, 2, p, R0, t0, cfg, res) == api.E_INVALID
        assert _register(L, ctx, 3, xyz, off, 3, p, R0, t0, None, res) == api.E_INVALID
        assert _register(L, ctx, 3, xyz, None, 3, p, R0, t0, cfg, res) == api.E_INVALID
        assert _register(L, ctx, 3, xyz, off, 3, p, None, t0, cfg, res) == api.E_INVALID
        assert _register(L, ctx, 3, xyz, off, 3, p, R0, None, cfg, res) == api.E_INVALID
        assert _register(L, ctx, 3, xyz, off, 3, p, R0, t0, cfg, None) == api.E_INVALID
        assert _register(L, ctx, 3, xyz, off + 1, 3, p, R0, t0, cfg, res) == api.E_INVALID
        assert b"start at 0" in L.dcreg_last_error(ctx)
        assert _register(L, ctx, 3, xyz, np.array([0, 8, 4, 12], np.int64), 3, p, R0, t0, cfg, res) == api.E_INVALID
        assert b"decrease" in L.dcreg_last_error(ctx)
        # valid arguments: the state is next (a zeroed block has no target)
        assert _register(L, ctx, 3, xyz, off, 3, p, R0, t0, cfg, res) == api.E_STATE
        # n_frames == 0 does nothing, whatever else is passed
        assert _register(L, ctx, 0, None, None, 3, p, None, None, cfg, None) == api.OK
    bad = api.normal_params()
    bad.k = 2
    assert _register(L, ctx, 3, xyz, off, 3, bad, R0, t0, cfg, res) == api.E_STATE          # mode 0: not read - the state is the reason
    # ---- dcreg_icp_run_trials_voxels
    assert _trials(L, ctx, 0, R0, t0, cfg, res) == api.OK
    assert _trials(L, ctx, -1, R0, t0, cfg, res) == api.E_INVALID
    assert _trials(L, ctx, 3, None, t0, cfg, res) == api.E_INVALID
    assert _trials(L, ctx, 3, R0, None, cfg, res) == api.E_INVALID
    assert _trials(L, ctx, 3, R0, t0, None, res) == api.E_INVALID
    assert _trials(L, ctx, 3, R0, t0, cfg, None) == api.E_INVALID
    assert _trials(L, ctx, 3, R0, t0, cfg, res) == api.E_STATE
    assert all(r.iterations == 0 and r.status == 0 and r.time_ms == 0.0 for r in res)
    # ---- the batched seam: what dcreg_voxels_batch_begin refuses before it looks at the device, in the header's order
    q = api.default_lin_params(0.5)
    outs = (api.LinOut * 3)()
    begin = L.dcreg_voxels_batch_begin
    for slot in (-1, 2):
        assert begin(ctx, slot, 3, api._dp(R0), api._dp(t0), None, C.byref(q)) == api.E_INVALID
        assert b"slot" in L.dcreg_last_error(ctx)
        assert L.dcreg_voxels_batch_end(ctx, slot, outs) == api.E_INVALID
    for n in (0, -1):
        assert begin(ctx, 0, n, api._dp(R0), api._dp(t0), None, C.byref(q)) == api.E_INVALID
    assert begin(ctx, 0, 3, None, api._dp(t0), None, C.byref(q)) == api.E_INVALID
    assert begin(ctx, 0, 3, api._dp(R0), None, None, C.byref(q)) == api.E_INVALID
    assert begin(ctx, 0, 3, api._dp(R0), api._dp(t0), None, None) == api.E_INVALID
    many = 65536
    Rm, tm = np.tile(np.eye(3).reshape(9), (many, 1)), np.zeros((many, 3))
    assert begin(ctx, 0, many, api._dp(Rm), api._dp(tm), None, C.byref(q)) == api.E_INVALID
    assert b"65535" in L.dcreg_last_error(ctx)
    # valid arguments: the state is next (a zeroed block reads as a context whose gated launch waits; the refusals behind that one -
    # parameterization, poses, target, kept voxels - need a real context: tests/test_gpu_frames_voxels.py)
    assert begin(ctx, 0, 3, api._dp(R0), api._dp(t0), None, C.byref(q)) == api.E_STATE
    assert L.dcreg_voxels_batch_end(ctx, 0, outs) == api.E_STATE                            # nothing in flight
    assert outs[0].n_eff == 0


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_the_methods_check_their_arguments():
    c = _ctx()
    cfg = api.default_config()
    f = [np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32)]
    with pytest.raises(ValueError, match="one initial pose per frame"):
        c.register_frames_voxels(f, [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="float32"):
        c.register_frames_voxels([np.zeros((4, 3))], [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="columns"):
        c.register_frames_voxels([f[0], np.zeros((4, 4), np.float32)], [I4, I4], "Ours", cfg)
    with pytest.raises(ValueError, match="method"):
        c.register_frames_voxels(f, [I4, I4], "XICP", cfg)
    with pytest.raises(ValueError, match="normal_params"):
        c.register_frames_voxels(f, [I4, I4], "Ours", cfg, frame_normals=5)
    bad = api.normal_params()
    bad.k = 40
    with pytest.raises(ValueError, match="k in"):
        c.register_frames_voxels(f, [I4, I4], "Ours", cfg, frame_normals=bad)
    with pytest.raises(ValueError, match="method"):
        c.icp_run_trials_voxels([I4], "XICP", cfg)
    euler = api.default_lin_params(0.5, euler_rpy=(0.0, 0.0, 0.0))
    for call in (c.voxels_batch_begin, c.voxels_batch):
        with pytest.raises(ValueError, match="parameterization"):
            call([I4], params=euler)
        with pytest.raises(ValueError, match="default_lin_params"):
            call([I4], params=5)
    with pytest.raises(ValueError):
        c.voxels_batch_begin([I4, I4], frame_ids=[0])          # one frame id per pose
