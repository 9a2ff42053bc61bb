"""Arguments the radius-support descriptor methods of Context check before anything reaches the library (no device needed), the parameter
blocks against the header and dcreg_sizeof, the default parameters, and the refusals of the C-ABI that need no context."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)


def test_the_parameter_blocks_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.FpfhRadiusParams._fields_] == ["radius", "max_neighbors", "reserved0_", "reserved_"]
    assert [f[0] for f in api.FpfhRadiusInfo._fields_] == ["n_in", "n_used", "n_empty", "n_crowded", "n_out", "m_max", "m_sum", "reserved_"]
    assert C.sizeof(api.FpfhRadiusParams) == 32 and C.sizeof(api.FpfhRadiusInfo) == 64
    for name, cls in (("dcreg_fpfh_radius_params", api.FpfhRadiusParams), ("dcreg_fpfh_radius_info", api.FpfhRadiusInfo)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name
        assert api._STRUCTS[name] is cls
    for name in ("dcreg_default_fpfh_radius_params", "dcreg_fpfh_radius", "dcreg_fpfh_radius_device", "dcreg_target_fpfh_radius",
                 "dcreg_target_fpfh_radius_device", "dcreg_fpfh_radius_debug_counts"):
        assert name in api.EXPORTS and hasattr(L, name), name


def test_the_default_parameters():
    p = api.FpfhRadiusParams()
    p.radius, p.max_neighbors, p.reserved0_, p.reserved_[1] = 9.0, 5, 7, 4.0
    assert api.load().dcreg_default_fpfh_radius_params(C.byref(p)) == api.OK
    assert (p.radius, p.max_neighbors, p.reserved0_, list(p.reserved_)) == (1.0, 65535, 0, [0.0, 0.0])
    assert bytes(p) == bytes(api.fpfh_radius_params())
    assert api.load().dcreg_default_fpfh_radius_params(None) == -1
    q = api.fpfh_radius_params(radius=2.5, max_neighbors=2)
    assert (q.radius, q.max_neighbors) == (2.5, 2)
    api.fpfh_radius_params(radius=1e-20)            # (its square, 1e-40, is a float above 0 - a denormal)
    api.fpfh_radius_params(radius=1.7e19)


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p, np_ = api.fpfh_radius_params(), api.normal_params()
    out = np.zeros(330, np.float32)
    info = api.FpfhRadiusInfo()
    assert L.dcreg_fpfh_radius(None, CLOUD.ctypes.data, 10, 3, CLOUD.ctypes.data, 3, None, C.byref(p), out.ctypes.data, None, C.byref(info)) == -1
    assert L.dcreg_fpfh_radius_device(None, None, 10, 3, None, 3, C.byref(np_), C.byref(p), None, None, None) == -1
    assert L.dcreg_target_fpfh_radius(None, C.byref(p), out.ctypes.data, 10, C.byref(info)) == -1
    assert L.dcreg_target_fpfh_radius_device(None, C.byref(p), None, 10, None) == -1
    assert L.dcreg_fpfh_radius_debug_counts(None, out.ctypes.data, 10) == -1
    assert not out.any() and info.n_in == 0 and info.m_sum == 0


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def _block(**kw):
    p = api.fpfh_radius_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [("radius", 0.0), ("radius", -0.5), ("radius", np.nan), ("radius", np.inf), ("radius", 1e-30), ("radius", 1.8e19),
              ("max_neighbors", 1), ("max_neighbors", 0), ("max_neighbors", -3), ("max_neighbors", 65536)]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    with pytest.raises(ValueError, match=field):
        api.fpfh_radius_params(**{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.fpfh_radius(CLOUD, CLOUD, params=p), lambda: c.fpfh_radius(CLOUD, params=p),
                 lambda: c.fpfh_radius_device(1, 10, 3, 1, 1, 3, None, p), lambda: c.target_fpfh_radius(p)):
        with pytest.raises(ValueError, match=field):
            call()


def test_the_normal_parameters_are_checked_when_the_normals_are_estimated():
    c = _ctx()
    bad = api.normal_params()
    bad.k = 40
    for call in (lambda: c.fpfh_radius(CLOUD, normal_params=bad), lambda: c.fpfh_radius_device(1, 10, 3, 1, 0, 3, bad)):
        with pytest.raises(ValueError, match="k in"):
            call()
    for call in (lambda: c.fpfh_radius(CLOUD, normal_params=api.fpfh_radius_params()), lambda: c.fpfh_radius_device(1, 10, 3, 1, 0, 3, api.voxel_params(0.1))):
        with pytest.raises(ValueError, match="normal_params"):
            call()
    # the k-form's block is not this rule's, and the other way round
    for call in (lambda: c.fpfh_radius(CLOUD, CLOUD, params=api.fpfh_params()), lambda: c.target_fpfh_radius(api.outlier_params()),
                 lambda: c.fpfh_radius_device(1, 10, 3, 1, 1, 3, None, api.normal_params())):
        with pytest.raises(ValueError, match="fpfh_radius_params"):
            call()
    with pytest.raises(ValueError, match="fpfh_params"):
        c.fpfh(CLOUD, CLOUD, params=api.fpfh_radius_params())


def test_clouds_normals_and_outputs_are_checked():
    c = _ctx()
    for call in (lambda: c.fpfh_radius(np.zeros((4, 2), np.float32), CLOUD[:4]), lambda: c.fpfh_radius(np.zeros((4, 3), np.float64), CLOUD[:4]),
                 lambda: c.fpfh_radius(CLOUD, np.zeros((10, 2), np.float32)), lambda: c.fpfh_radius(CLOUD, np.zeros(30, np.float32))):
        with pytest.raises(ValueError, match="float32"):
            call()
    with pytest.raises(ValueError, match="one normal per point"):
        c.fpfh_radius(CLOUD, CLOUD[:9])
    with pytest.raises(ValueError, match="want_normals"):
        c.fpfh_radius(CLOUD, CLOUD, want_normals=True)
    with pytest.raises(ValueError, match="stride"):
        c.fpfh_radius_device(1, 10, 2, 1, 1)
    with pytest.raises(ValueError, match="normals stride"):
        c.fpfh_radius_device(1, 10, 3, 1, 1, 2)
    for call in (lambda: c.fpfh_radius_device(1, -1, 3, 1, 1), lambda: c.fpfh_radius_device(1, 2 ** 31, 3, 1, 1)):
        with pytest.raises(ValueError, match="points"):
            call()
    with pytest.raises(ValueError, match="output"):
        c.fpfh_radius_device(1, 10, 3, 0, 1)
