"""Arguments the descriptor and matching methods of Context check before anything reaches the library (no device needed), the parameter
blocks against the header and dcreg_sizeof, the default parameters, and the refusals of the C-ABI that need no context."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)
ROWS = np.zeros((4, 33), np.float32)


def test_the_parameter_blocks_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.FpfhParams._fields_] == ["k", "reserved0_", "search_radius", "reserved_"]
    assert [f[0] for f in api.FpfhInfo._fields_] == ["n_in", "n_used", "n_empty", "n_out"]
    assert [f[0] for f in api.MatchInfo._fields_] == ["n_a_valid", "n_b_valid", "n_mutual", "reserved_"]
    assert C.sizeof(api.FpfhParams) == 32 and C.sizeof(api.FpfhInfo) == 32 and C.sizeof(api.MatchInfo) == 32
    for name, cls in (("dcreg_fpfh_params", api.FpfhParams), ("dcreg_fpfh_info", api.FpfhInfo), ("dcreg_match_info", api.MatchInfo)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name
        assert api._STRUCTS[name] is cls
    assert api.FPFH_DIM == 33
    for name in ("dcreg_default_fpfh_params", "dcreg_fpfh", "dcreg_fpfh_device", "dcreg_target_fpfh", "dcreg_target_fpfh_device",
                 "dcreg_fpfh_debug_counts", "dcreg_feature_match", "dcreg_feature_match_device"):
        assert name in api.EXPORTS and hasattr(L, name), name


def test_the_default_parameters():
    p = api.FpfhParams()
    p.k, p.reserved0_, p.search_radius, p.reserved_[1] = 9, 5, 2.0, 4.0
    assert api.load().dcreg_default_fpfh_params(C.byref(p)) == api.OK
    assert (p.k, p.reserved0_, p.search_radius, list(p.reserved_)) == (16, 0, 0.0, [0.0, 0.0])
    assert bytes(p) == bytes(api.fpfh_params())
    assert api.load().dcreg_default_fpfh_params(None) == -1
    q = api.fpfh_params(k=32, search_radius=0.5)
    assert (q.k, q.search_radius) == (32, 0.5)
    api.fpfh_params(k=3)


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p, np_ = api.fpfh_params(), api.normal_params()
    out = np.zeros(330, np.float32)
    info, minfo = api.FpfhInfo(), api.MatchInfo()
    idx, d = np.zeros(4, np.int32), np.zeros(4)
    assert L.dcreg_fpfh(None, CLOUD.ctypes.data, 10, 3, CLOUD.ctypes.data, 3, None, C.byref(p), out.ctypes.data, None, C.byref(info)) == -1
    assert L.dcreg_fpfh_device(None, None, 10, 3, None, 3, C.byref(np_), C.byref(p), None, None, None) == -1
    assert L.dcreg_target_fpfh(None, C.byref(p), out.ctypes.data, 10, C.byref(info)) == -1
    assert L.dcreg_target_fpfh_device(None, C.byref(p), None, 10, None) == -1
    assert L.dcreg_fpfh_debug_counts(None, out.ctypes.data, 10) == -1
    assert L.dcreg_feature_match(None, ROWS.ctypes.data, 4, 33, ROWS.ctypes.data, 4, 33, idx.ctypes.data, d.ctypes.data, None, None, None, C.byref(minfo)) == -1
    assert L.dcreg_feature_match_device(None, None, 4, 33, None, 4, 33, None, None, None, None, None, None) == -1
    assert not out.any() and info.n_in == 0 and minfo.n_a_valid == 0 and not idx.any()


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def _block(**kw):
    p = api.fpfh_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [("k", 2), ("k", 0), ("k", 33), ("k", -5), ("search_radius", -0.5), ("search_radius", np.nan), ("search_radius", np.inf)]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    with pytest.raises(ValueError, match=field):
        api.fpfh_params(**{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.fpfh(CLOUD, CLOUD, params=p), lambda: c.fpfh(CLOUD, params=p), lambda: c.fpfh_device(1, 10, 3, 1, 1, 3, None, p),
                 lambda: c.target_fpfh(p)):
        with pytest.raises(ValueError, match=field):
            call()


def test_the_normal_parameters_are_checked_when_the_normals_are_estimated():
    c = _ctx()
    bad = api.normal_params()
    bad.k = 40
    for call in (lambda: c.fpfh(CLOUD, normal_params=bad), lambda: c.fpfh_device(1, 10, 3, 1, 0, 3, bad)):
        with pytest.raises(ValueError, match="k in"):
            call()
    for call in (lambda: c.fpfh(CLOUD, normal_params=api.fpfh_params()), lambda: c.fpfh_device(1, 10, 3, 1, 0, 3, api.voxel_params(0.1))):
        with pytest.raises(ValueError, match="normal_params"):
            call()
    for call in (lambda: c.fpfh(CLOUD, CLOUD, params=api.normal_params()), lambda: c.target_fpfh(api.outlier_params()),
                 lambda: c.fpfh_device(1, 10, 3, 1, 1, 3, None, api.place_params())):
        with pytest.raises(ValueError, match="fpfh_params"):
            call()


def test_clouds_normals_and_outputs_are_checked():
    c = _ctx()
    for call in (lambda: c.fpfh(np.zeros((4, 2), np.float32), CLOUD[:4]), lambda: c.fpfh(np.zeros((4, 3), np.float64), CLOUD[:4]),
                 lambda: c.fpfh(CLOUD, np.zeros((10, 2), np.float32)), lambda: c.fpfh(CLOUD, np.zeros(30, np.float32))):
        with pytest.raises(ValueError, match="float32"):
            call()
    with pytest.raises(ValueError, match="one normal per point"):
        c.fpfh(CLOUD, CLOUD[:9])
    with pytest.raises(ValueError, match="want_normals"):
        c.fpfh(CLOUD, CLOUD, want_normals=True)
    with pytest.raises(ValueError, match="stride"):
        c.fpfh_device(1, 10, 2, 1, 1)
    with pytest.raises(ValueError, match="normals stride"):
        c.fpfh_device(1, 10, 3, 1, 1, 2)
    for call in (lambda: c.fpfh_device(1, -1, 3, 1, 1), lambda: c.fpfh_device(1, 2 ** 31, 3, 1, 1)):
        with pytest.raises(ValueError, match="points"):
            call()
    with pytest.raises(ValueError, match="output"):
        c.fpfh_device(1, 10, 3, 0, 1)


def test_descriptor_rows_are_checked():
    c = _ctx()
    for call in (lambda: c.feature_match(np.zeros((4, 32), np.float32), ROWS), lambda: c.feature_match(ROWS, np.zeros((4, 33), np.float64)),
                 lambda: c.feature_match(np.zeros(33, np.float32), ROWS)):
        with pytest.raises(ValueError, match="float32"):
            call()
    for call in (lambda: c.feature_match_device(1, 4, 32, 1, 4, 33, 1, 1), lambda: c.feature_match_device(1, 4, 33, 1, 4, 3, 1, 1)):
        with pytest.raises(ValueError, match="stride"):
            call()
    for call in (lambda: c.feature_match_device(1, -1, 33, 1, 4, 33, 1, 1), lambda: c.feature_match_device(1, 4, 33, 1, 2 ** 31, 33, 1, 1)):
        with pytest.raises(ValueError, match="rows"):
            call()
    for call in (lambda: c.feature_match_device(1, 4, 33, 1, 4, 33, 0, 1), lambda: c.feature_match_device(1, 4, 33, 1, 4, 33, 1, 0)):
        with pytest.raises(ValueError, match="outputs"):
            call()
