"""The third engine's binding without a device: the dump block against the header and dcreg_sizeof, the exports, the refusals of the
C-ABI that need no context, and the arguments the Context methods check before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

NEW = ("dcreg_source_normals_keep", "dcreg_source_normals_set", "dcreg_source_normals_set_device", "dcreg_source_normals_get",
       "dcreg_source_normals_get_device", "dcreg_source_normals_kept", "dcreg_source_normals_drop", "dcreg_linearize_gicp",
       "dcreg_linearize_gicp_debug", "dcreg_icp_run_gicp")
I4 = np.eye(4)


def test_the_dump_block_matches_the_header_and_every_symbol_is_exported():
    L = api.load()
    assert [f[0] for f in api.GlinDebug._fields_] == ["nn_idx", "nn_d2", "flag", "normal_map", "normal_src", "w", "r", "row"]
    assert C.sizeof(api.GlinDebug) == 64 and L.dcreg_sizeof(b"dcreg_glin_debug") == 64
    assert api._STRUCTS["dcreg_glin_debug"] is api.GlinDebug
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name), name


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p, q = api.normal_params(), api.default_lin_params(0.5)
    out, info, res = api.LinOut(), api.NormalInfo(), api.IcpResult()
    nrm = np.zeros((4, 4), np.float32)
    R, t = np.eye(3).reshape(9), np.zeros(3)
    assert L.dcreg_source_normals_keep(None, C.byref(p), C.byref(info)) == api.E_INVALID
    assert L.dcreg_source_normals_set(None, nrm.ctypes.data, 4, 4) == api.E_INVALID
    assert L.dcreg_source_normals_set_device(None, None, 4, 3) == api.E_INVALID
    assert L.dcreg_source_normals_get(None, nrm.ctypes.data, 4) == api.E_INVALID
    assert L.dcreg_source_normals_get_device(None, None, 4) == api.E_INVALID
    assert L.dcreg_source_normals_kept(None) == 0
    assert L.dcreg_source_normals_drop(None) == api.E_INVALID
    assert L.dcreg_linearize_gicp(None, api._dp(R), api._dp(t), C.byref(q), C.byref(out)) == api.E_INVALID
    assert L.dcreg_linearize_gicp_debug(None, api._dp(R), api._dp(t), C.byref(q), C.byref(out), C.byref(api.GlinDebug())) == api.E_INVALID
    cfg = api.default_config()
    assert L.dcreg_icp_run_gicp(None, api._dp(R), api._dp(t), 0, 0, C.byref(cfg), None, 0, C.byref(res)) == api.E_INVALID
    assert out.n_eff == 0 and info.n_in == 0 and res.iterations == 0 and not nrm.any()


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_keep_checks_its_parameter_block():
    c = _ctx()
    p = api.normal_params()
    p.k = 2
    with pytest.raises(ValueError, match="k"):
        c.keep_source_normals(p)
    with pytest.raises(ValueError, match="normal_params"):
        c.keep_source_normals(api.voxel_params(0.1))


def test_set_checks_its_normals():
    c = _ctx()
    for bad in (np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float64), np.zeros(12, np.float32)):
        with pytest.raises(ValueError, match="float32"):
            c.set_source_normals(bad)
    with pytest.raises(ValueError, match="either"):
        c.set_source_normals()
    with pytest.raises(ValueError, match="either"):
        c.set_source_normals(np.zeros((4, 3), np.float32), dev_ptr=16)
    with pytest.raises(ValueError, match="n and stride"):
        c.set_source_normals(dev_ptr=16)
    with pytest.raises(ValueError, match="stride"):
        c.set_source_normals(dev_ptr=16, n=4, stride=2)
    with pytest.raises(ValueError, match="points"):
        c.set_source_normals(dev_ptr=16, n=-1, stride=3)


def test_get_checks_its_capacity():
    c = _ctx()
    for cap in (None, -1, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="capacity"):
            c.kept_source_normals(dev_ptr=16, capacity=cap)
    with pytest.raises(ValueError, match="dev_ptr only"):
        c.kept_source_normals(capacity=4)


def test_the_linearisation_checks_pose_and_parameters():
    c = _ctx()
    euler = api.default_lin_params(0.5, euler_rpy=(0.0, 0.0, 0.0))
    for debug in (False, True):
        with pytest.raises(ValueError, match="parameterization"):
            c.linearize_gicp(I4, euler, debug=debug)
        for r in (0.0, -1.0, np.nan, np.inf):
            p = api.default_lin_params(0.5)
            p.search_radius = r
            with pytest.raises(ValueError, match="search_radius"):
                c.linearize_gicp(I4, p, debug=debug)
        with pytest.raises(ValueError, match="default_lin_params"):
            c.linearize_gicp(I4, api.normal_params(), debug=debug)
        for T in (np.eye(3), np.full((4, 4), np.nan), np.zeros(16)):
            with pytest.raises(ValueError, match="4 x 4"):
                c.linearize_gicp(T, api.default_lin_params(0.5), debug=debug)


def test_the_engine_checks_pose_and_method():
    c = _ctx()
    cfg = api.default_config()
    with pytest.raises(ValueError, match="4 x 4"):
        c.icp_run_gicp(np.eye(3), "Ours", cfg)
    bad = np.eye(4)
    bad[0, 3] = np.inf
    with pytest.raises(ValueError, match="4 x 4"):
        c.icp_run_gicp(bad, "Ours", cfg)
    with pytest.raises(ValueError, match="method"):
        c.icp_run_gicp(I4, "XICP", cfg)
