"""The many-clouds normal estimation and the third engine's many-frames calls without a device: the exports, the refusals of the C-ABI
that need no context or no device (null arguments, a stride below 3, offsets that do not start at 0 or decrease, null parameters, both
outputs null), n_frames == 0 / n_clouds == 0, and the arguments the Context methods check before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

NEW = ("dcreg_normals_clouds", "dcreg_normals_clouds_device", "dcreg_frames_normals_keep", "dcreg_frames_normals_set",
       "dcreg_frames_normals_kept", "dcreg_gicp_batch_begin", "dcreg_gicp_batch_end", "dcreg_normal_params_check",
       "dcreg_register_frames_gicp", "dcreg_icp_run_trials_gicp")
FP, I64P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
I4 = np.eye(4)


class _Ctx(C.Structure):
    """a zeroed block of memory stands in for a context: the refusals below leave their text in it and look at nothing else"""
    _fields_ = [("bytes", C.c_char * (1 << 16))]


def _frames(n=3, pts=4):
    xyz = np.zeros((n * pts, 3), np.float32)
    off = np.arange(n + 1, dtype=np.int64) * pts
    R0 = np.tile(np.eye(3).reshape(9), (n, 1))
    t0 = np.zeros((n, 3))
    return xyz, off, R0, t0


def _register(L, ctx, n, xyz, off, stride, prm, R0, t0, cfg, res):
    return L.dcreg_register_frames_gicp(ctx, n, None if xyz is None else xyz.ctypes.data_as(FP), None if off is None else off.ctypes.data_as(I64P),
                                        stride, None if prm is None else C.byref(prm), None if R0 is None else api._dp(R0),
                                        None if t0 is None else api._dp(t0), 0, 0, None if cfg is None else C.byref(cfg), 0, res)


def _clouds(L, ctx, n, xyz, off, stride, prm, nrm, cur, infos, device=False):
    fn = L.dcreg_normals_clouds_device if device else L.dcreg_normals_clouds
    return fn(ctx, n, None if xyz is None else xyz.ctypes.data, None if off is None else off.ctypes.data_as(I64P), stride,
              None if prm is None else C.byref(prm), None if nrm is None else nrm.ctypes.data, None if cur is None else cur.ctypes.data, infos)


def test_every_symbol_is_exported_and_no_struct_moved():
    L = api.load()
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name, cls in (("dcreg_trial_result", api.TrialResult), ("dcreg_lin_out", api.LinOut), ("dcreg_lin_params", api.LinParams),
                      ("dcreg_normal_params", api.NormalParams), ("dcreg_normal_info", api.NormalInfo)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    xyz, off, R0, t0 = _frames()
    cfg, q, prm = api.default_config(), api.default_lin_params(0.5), api.normal_params()
    res = (api.TrialResult * 3)()
    outs = (api.LinOut * 3)()
    infos = (api.NormalInfo * 3)()
    ids = np.zeros(3, np.int32)
    nrm, cur = np.full((12, 3), 7.0, np.float32), np.full(12, 7.0, np.float32)
    assert _register(L, None, 3, xyz, off, 3, prm, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, None, 0, xyz, off, 3, prm, R0, t0, cfg, res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_gicp(None, 3, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), res) == api.E_INVALID
    for device in (False, True):
        assert _clouds(L, None, 3, xyz, off, 3, prm, nrm, cur, infos, device) == api.E_INVALID
    assert L.dcreg_frames_normals_keep(None, C.byref(prm), infos) == api.E_INVALID
    assert L.dcreg_frames_normals_set(None, nrm.ctypes.data, 12, 3) == api.E_INVALID
    assert L.dcreg_frames_normals_kept(None) == 0
    assert L.dcreg_normal_params_check(None, C.byref(prm)) == api.E_INVALID
    assert L.dcreg_gicp_batch_begin(None, 0, 3, api._dp(R0), api._dp(t0), ids.ctypes.data_as(I32P), ids.ctypes.data_as(I32P), C.byref(q)) == api.E_INVALID
    assert L.dcreg_gicp_batch_end(None, 0, outs) == api.E_INVALID
    assert all(r.iterations == 0 and r.status == 0 for r in res) and outs[0].n_eff == 0
    assert np.all(nrm == 7.0) and np.all(cur == 7.0) and all(i.n_in == 0 for i in infos)


def test_argument_refusals_that_need_no_device():
    L = api.load()
    L.dcreg_last_error.restype = C.c_char_p
    xyz, off, R0, t0 = _frames()
    cfg, prm = api.default_config(), api.normal_params()
    res = (api.TrialResult * 3)()
    infos = (api.NormalInfo * 3)()
    nrm, cur = np.full((12, 3), 7.0, np.float32), np.full(12, 7.0, np.float32)
    blob = _Ctx()
    ctx = C.c_void_p(C.addressof(blob))
    # ---- dcreg_register_frames_gicp
    assert _register(L, ctx, -1, xyz, off, 3, prm, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, ctx, 3, xyz, off, 2, prm, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, ctx, 3, xyz, off, 3, prm, R0, t0, None, res) == api.E_INVALID
    assert _register(L, ctx, 3, xyz, off, 3, None, R0, t0, cfg, res) == api.E_INVALID
    assert b"null normal parameters" in L.dcreg_last_error(ctx)
    bad = api.normal_params()
    bad.k = 2
    assert _register(L, ctx, 3, xyz, off, 3, bad, R0, t0, cfg, res) == api.E_INVALID
    assert b"normal k" in L.dcreg_last_error(ctx)
    assert _register(L, ctx, 3, xyz, None, 3, prm, R0, t0, cfg, res) == api.E_INVALID
    assert _register(L, ctx, 3, xyz, off, 3, prm, None, t0, cfg, res) == api.E_INVALID
    assert _register(L, ctx, 3, xyz, off, 3, prm, R0, None, cfg, res) == api.E_INVALID
    assert _register(L, ctx, 3, xyz, off, 3, prm, R0, t0, cfg, None) == api.E_INVALID
    assert _register(L, ctx, 3, xyz, off + 1, 3, prm, R0, t0, cfg, res) == api.E_INVALID
    assert b"start at 0" in L.dcreg_last_error(ctx)
    assert _register(L, ctx, 3, xyz, np.array([0, 8, 4, 12], np.int64), 3, prm, R0, t0, cfg, res) == api.E_INVALID
    assert b"decrease" in L.dcreg_last_error(ctx)
    # n_frames == 0 / n_trials == 0 do nothing, whatever else is passed
    assert _register(L, ctx, 0, None, None, 3, prm, None, None, cfg, None) == api.OK
    assert L.dcreg_icp_run_trials_gicp(ctx, 0, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), res) == api.OK
    assert L.dcreg_icp_run_trials_gicp(ctx, -1, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_gicp(ctx, 3, None, api._dp(t0), 0, 0, C.byref(cfg), res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_gicp(ctx, 3, api._dp(R0), api._dp(t0), 0, 0, None, res) == api.E_INVALID
    assert L.dcreg_icp_run_trials_gicp(ctx, 3, api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), None) == api.E_INVALID
    assert all(r.iterations == 0 and r.status == 0 for r in res)
    # ---- dcreg_normals_clouds[_device]
    for device in (False, True):
        assert _clouds(L, ctx, 3, xyz, off, 2, prm, nrm, cur, infos, device) == api.E_INVALID
        assert _clouds(L, ctx, 3, xyz, off, 3, None, nrm, cur, infos, device) == api.E_INVALID
        assert b"null normal parameters" in L.dcreg_last_error(ctx)
        assert _clouds(L, ctx, 3, xyz, off, 3, bad, nrm, cur, infos, device) == api.E_INVALID
        assert _clouds(L, ctx, -1, xyz, off, 3, prm, nrm, cur, infos, device) == api.E_INVALID
        assert _clouds(L, ctx, 3, xyz, None, 3, prm, nrm, cur, infos, device) == api.E_INVALID
        assert _clouds(L, ctx, 3, xyz, off + 1, 3, prm, nrm, cur, infos, device) == api.E_INVALID
        assert b"start at 0" in L.dcreg_last_error(ctx)
        assert _clouds(L, ctx, 3, xyz, np.array([0, 8, 4, 12], np.int64), 3, prm, nrm, cur, infos, device) == api.E_INVALID
        assert b"decrease" in L.dcreg_last_error(ctx)
        assert _clouds(L, ctx, 3, xyz, np.array([0, 4, 8, 2 ** 31], np.int64), 3, prm, nrm, cur, infos, device) == api.E_INVALID
        assert b"too many points" in L.dcreg_last_error(ctx)
        assert _clouds(L, ctx, 3, xyz, off, 3, prm, None, None, infos, device) == api.E_INVALID
        assert b"no output buffer" in L.dcreg_last_error(ctx)
        assert _clouds(L, ctx, 3, None, off, 3, prm, nrm, cur, infos, device) == api.E_INVALID
        # n_clouds == 0 does nothing and writes nothing; so do clouds that are all empty (their infos are zeroed)
        assert _clouds(L, ctx, 0, None, None, 3, prm, nrm, cur, None, device) == api.OK
        assert _clouds(L, ctx, 3, None, np.zeros(4, np.int64), 3, prm, nrm, cur, infos, device) == api.OK
    assert np.all(nrm == 7.0) and np.all(cur == 7.0) and all(i.n_in == 0 and i.n_out == 0 for i in infos)
    # ---- the frames' kept normals: parameters and arguments first, then the context's state (a zeroed block has no frames)
    assert L.dcreg_frames_normals_keep(ctx, None, infos) == api.E_INVALID
    assert L.dcreg_frames_normals_keep(ctx, C.byref(bad), infos) == api.E_INVALID
    assert L.dcreg_frames_normals_keep(ctx, C.byref(prm), infos) == api.E_STATE
    assert L.dcreg_frames_normals_set(ctx, None, 12, 3) == api.E_INVALID
    assert L.dcreg_frames_normals_set(ctx, nrm.ctypes.data, 12, 2) == api.E_INVALID
    assert L.dcreg_frames_normals_set(ctx, nrm.ctypes.data, 12, 3) == api.E_STATE
    assert L.dcreg_frames_normals_kept(ctx) == 0
    assert L.dcreg_normal_params_check(ctx, C.byref(prm)) == api.OK
    for field, value in (("k", 33), ("orient", 2), ("search_radius", -1.0), ("search_radius", np.inf)):
        p = api.normal_params()
        setattr(p, field, value)
        assert L.dcreg_normal_params_check(ctx, C.byref(p)) == api.E_INVALID, field
    p = api.normal_params()
    p.viewpoint[1] = np.nan
    assert L.dcreg_normal_params_check(ctx, C.byref(p)) == api.E_INVALID
    # ---- the batched seam: what dcreg_normals_batch_begin refuses before it looks at the device
    q = api.default_lin_params(0.5)
    ids = np.zeros(3, np.int32)
    outs = (api.LinOut * 3)()
    for slot in (-1, 2):
        assert L.dcreg_gicp_batch_begin(ctx, slot, 3, api._dp(R0), api._dp(t0), None, None, C.byref(q)) == api.E_INVALID
        assert L.dcreg_gicp_batch_end(ctx, slot, outs) == api.E_INVALID
    assert L.dcreg_gicp_batch_begin(ctx, 0, 0, api._dp(R0), api._dp(t0), None, None, C.byref(q)) == api.E_INVALID
    assert L.dcreg_gicp_batch_begin(ctx, 0, 3, None, api._dp(t0), None, None, C.byref(q)) == api.E_INVALID
    assert L.dcreg_gicp_batch_begin(ctx, 0, 3, api._dp(R0), api._dp(t0), None, None, None) == api.E_INVALID
    assert L.dcreg_gicp_batch_begin(ctx, 0, 3, api._dp(R0), api._dp(t0), ids.ctypes.data_as(I32P), None, C.byref(q)) == api.E_STATE     # valid arguments: the state is next
    assert L.dcreg_gicp_batch_end(ctx, 0, outs) == api.E_STATE                                                               # nothing in flight
    assert outs[0].n_eff == 0


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_the_methods_check_their_arguments():
    c = _ctx()
    cfg = api.default_config()
    f = [np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32)]
    with pytest.raises(ValueError, match="one initial pose per frame"):
        c.register_frames_gicp(f, [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="float32"):
        c.register_frames_gicp([np.zeros((4, 3))], [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="columns"):
        c.register_frames_gicp([f[0], np.zeros((4, 4), np.float32)], [I4, I4], "Ours", cfg)
    with pytest.raises(ValueError, match="method"):
        c.register_frames_gicp(f, [I4, I4], "XICP", cfg)
    with pytest.raises(ValueError, match="normal_params"):
        c.register_frames_gicp(f, [I4, I4], "Ours", cfg, frame_normals=5)
    bad = api.normal_params()
    bad.k = 40
    with pytest.raises(ValueError, match="k in"):
        c.register_frames_gicp(f, [I4, I4], "Ours", cfg, frame_normals=bad)
    with pytest.raises(ValueError, match="method"):
        c.icp_run_trials_gicp([I4], "XICP", cfg)
    euler = api.default_lin_params(0.5, euler_rpy=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="parameterization"):
        c.gicp_batch_begin([I4], params=euler)
    p = api.default_lin_params(0.5)
    p.search_radius = np.nan
    with pytest.raises(ValueError, match="search_radius"):
        c.gicp_batch_begin([I4], params=p)
    # normals_clouds
    with pytest.raises(ValueError, match="k in"):
        c.normals_clouds(f, bad)
    with pytest.raises(ValueError, match="at least one"):
        c.normals_clouds(f, want_normals=False, want_curvature=False)
    with pytest.raises(ValueError, match="float32"):
        c.normals_clouds([np.zeros((4, 3))])
    with pytest.raises(ValueError, match="columns"):
        c.normals_clouds([f[0], np.zeros((4, 4), np.float32)])
    with pytest.raises(ValueError, match="offsets"):
        c.normals_clouds((np.zeros((9, 3), np.float32), [0, 5, 4, 9]))
    with pytest.raises(ValueError, match="offsets"):
        c.normals_clouds_device(1, [1, 4], 3, dev_normals_ptr=1)
    with pytest.raises(ValueError, match="stride"):
        c.normals_clouds_device(1, [0, 4], 2, dev_normals_ptr=1)
    with pytest.raises(ValueError, match="at least one"):
        c.normals_clouds_device(1, [0, 4], 3)
    with pytest.raises(ValueError, match="k in"):
        c.frames_normals_keep(bad)
    with pytest.raises(ValueError, match="float32"):
        c.frames_normals_set(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="columns"):
        c.frames_normals_set([np.zeros((4, 3), np.float32), np.zeros((4, 4), np.float32)])
