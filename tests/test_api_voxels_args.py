"""The fourth engine's binding without a device: the structs against the header and dcreg_sizeof, the exports, the refusals of the C-ABI
that need no context, and the arguments the Context methods check before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

NEW = ("dcreg_default_voxel_map_params", "dcreg_target_voxels_keep", "dcreg_target_voxels_get", "dcreg_target_voxels_kept",
       "dcreg_target_voxels_drop", "dcreg_linearize_voxels", "dcreg_linearize_voxels_debug", "dcreg_icp_run_voxels")
I4 = np.eye(4)


def test_the_structs_match_the_header_and_every_symbol_is_exported():
    L = api.load()
    assert [f[0] for f in api.VlinDebug._fields_] == ["voxel_idx", "flag", "mean", "cov", "normal_src", "w", "r", "row"]
    assert C.sizeof(api.VlinDebug) == 64 and L.dcreg_sizeof(b"dcreg_vlin_debug") == 64
    assert [f[0] for f in api.VoxelMapParams._fields_] == ["leaf", "epsilon", "min_points", "reserved_"]
    assert C.sizeof(api.VoxelMapParams) == 24 and L.dcreg_sizeof(b"dcreg_voxel_map_params") == 24
    assert [f[0] for f in api.VoxelMapInfo._fields_] == ["n_points", "n_voxels", "n_small", "n_degenerate", "n_kept"]
    assert C.sizeof(api.VoxelMapInfo) == 40 and L.dcreg_sizeof(b"dcreg_voxel_map_info") == 40
    for name, cls in (("dcreg_vlin_debug", api.VlinDebug), ("dcreg_voxel_map_params", api.VoxelMapParams), ("dcreg_voxel_map_info", api.VoxelMapInfo)):
        assert api._STRUCTS[name] is cls
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name), name


def test_the_defaults_are_the_headers():
    L = api.load()
    p = api.VoxelMapParams()
    assert L.dcreg_default_voxel_map_params(C.byref(p)) == 0
    assert (p.leaf, p.epsilon, p.min_points, p.reserved_) == (1.0, 1e-3, 6, 0)
    assert L.dcreg_default_voxel_map_params(None) == api.E_INVALID
    q = api.voxel_map_params()
    assert (q.leaf, q.epsilon, q.min_points) == (1.0, 1e-3, 6)


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p, q = api.voxel_map_params(), api.default_lin_params(0.5)
    out, info, res = api.LinOut(), api.VoxelMapInfo(), api.IcpResult()
    R, t = np.eye(3).reshape(9), np.zeros(3)
    buf = np.zeros(16, np.int64)
    assert L.dcreg_target_voxels_keep(None, C.byref(p), C.byref(info)) == api.E_INVALID
    assert L.dcreg_target_voxels_get(None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 1) == api.E_INVALID
    assert L.dcreg_target_voxels_kept(None) == 0
    assert L.dcreg_target_voxels_drop(None) == api.E_INVALID
    assert L.dcreg_linearize_voxels(None, api._dp(R), api._dp(t), C.byref(q), C.byref(out)) == api.E_INVALID
    assert L.dcreg_linearize_voxels_debug(None, api._dp(R), api._dp(t), C.byref(q), C.byref(out), C.byref(api.VlinDebug())) == api.E_INVALID
    cfg = api.default_config()
    assert L.dcreg_icp_run_voxels(None, api._dp(R), api._dp(t), 0, 0, C.byref(cfg), None, 0, C.byref(res)) == api.E_INVALID
    assert out.n_eff == 0 and info.n_kept == 0 and res.iterations == 0 and not buf.any()


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_keep_checks_its_parameter_block():
    c = _ctx()
    for leaf in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="leaf"):
            api.voxel_map_params(leaf=leaf)
        p = api.voxel_map_params()
        p.leaf = leaf
        with pytest.raises(ValueError, match="leaf"):
            c.keep_target_voxels(p)
    for eps in (0.0, 9.9e-7, 1.0000001, np.nan, -1e-3):
        p = api.voxel_map_params()
        p.epsilon = eps
        with pytest.raises(ValueError, match="epsilon"):
            c.keep_target_voxels(p)
    for mp in (1, 0, -3):
        p = api.voxel_map_params()
        p.min_points = mp
        with pytest.raises(ValueError, match="min_points"):
            c.keep_target_voxels(p)
    with pytest.raises(ValueError, match="voxel_map_params"):
        c.keep_target_voxels(api.voxel_params(0.1))
    for ok in (api.voxel_map_params(0.5, 1e-6, 2), api.voxel_map_params(2.0, 1.0, 100)):
        api._check_voxel_map_params(ok, "test")


def test_the_linearisation_checks_pose_and_parameters():
    c = _ctx()
    euler = api.default_lin_params(0.5, euler_rpy=(0.0, 0.0, 0.0))
    for debug in (False, True):
        with pytest.raises(ValueError, match="parameterization"):
            c.linearize_voxels(I4, euler, debug=debug)
        with pytest.raises(ValueError, match="default_lin_params"):
            c.linearize_voxels(I4, api.normal_params(), debug=debug)
        for T in (np.eye(3), np.full((4, 4), np.nan), np.zeros(16)):
            with pytest.raises(ValueError, match="4 x 4"):
                c.linearize_voxels(T, api.default_lin_params(0.5), debug=debug)
    with pytest.raises(ValueError, match="parameterization"):
        c.linearize_voxels_debug(I4, euler)


def test_the_engine_checks_pose_and_method():
    c = _ctx()
    cfg = api.default_config()
    with pytest.raises(ValueError, match="4 x 4"):
        c.icp_run_voxels(np.eye(3), "Ours", cfg)
    bad = np.eye(4)
    bad[0, 3] = np.inf
    with pytest.raises(ValueError, match="4 x 4"):
        c.icp_run_voxels(bad, "Ours", cfg)
    with pytest.raises(ValueError, match="method"):
        c.icp_run_voxels(I4, "XICP", cfg)
