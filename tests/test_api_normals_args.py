"""Arguments the normal methods of Context check before anything reaches the library (no device needed), the parameter blocks against the
header and dcreg_sizeof, the default parameters, and the refusals of the C-ABI that need no context."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)


def test_the_parameter_blocks_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.NormalParams._fields_] == ["k", "orient", "search_radius", "viewpoint", "reserved_"]
    assert [f[0] for f in api.NormalInfo._fields_] == ["n_in", "n_finite", "n_sparse", "n_out"]
    assert C.sizeof(api.NormalParams) == 56 and C.sizeof(api.NormalInfo) == 32
    assert L.dcreg_sizeof(b"dcreg_normal_params") == C.sizeof(api.NormalParams)
    assert L.dcreg_sizeof(b"dcreg_normal_info") == C.sizeof(api.NormalInfo)
    assert api.NORMAL_ORIENT == {"viewpoint": 0, "none": 1}
    assert api._STRUCTS["dcreg_normal_params"] is api.NormalParams and api._STRUCTS["dcreg_normal_info"] is api.NormalInfo
    for name in ("dcreg_default_normal_params", "dcreg_normals", "dcreg_normals_device", "dcreg_target_normals", "dcreg_target_normals_device"):
        assert name in api.EXPORTS and hasattr(L, name)


def test_the_default_parameters():
    p = api.NormalParams()
    p.k, p.orient, p.search_radius, p.viewpoint[1], p.reserved_[0] = 9, 1, 2.0, 3.0, 4.0
    assert api.load().dcreg_default_normal_params(C.byref(p)) == api.OK
    assert (p.k, p.orient, p.search_radius, list(p.viewpoint), list(p.reserved_)) == (5, 0, 0.0, [0.0, 0.0, 0.0], [0.0, 0.0])
    assert bytes(p) == bytes(api.normal_params())
    assert api.load().dcreg_default_normal_params(None) == -1
    q = api.normal_params(k=16, search_radius=0.5, viewpoint=(1.0, -2.0, 3.5))
    assert (q.k, q.orient, q.search_radius, list(q.viewpoint)) == (16, 0, 0.5, [1.0, -2.0, 3.5])
    r = api.normal_params(viewpoint=None)
    assert (r.k, r.orient, list(r.viewpoint)) == (5, 1, [0.0, 0.0, 0.0])
    api.normal_params(k=3)
    api.normal_params(k=32)


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p = api.normal_params()
    out = np.zeros(30, np.float32)
    info = api.NormalInfo()
    assert L.dcreg_normals(None, CLOUD.ctypes.data, 10, 3, C.byref(p), out.ctypes.data, None, None, C.byref(info)) == -1
    assert L.dcreg_normals_device(None, None, 10, 3, C.byref(p), None, None, None, None) == -1
    assert L.dcreg_target_normals(None, C.byref(p), out.ctypes.data, None, None, 10, C.byref(info)) == -1
    assert L.dcreg_target_normals_device(None, C.byref(p), None, None, None, 10, None) == -1
    assert not out.any() and info.n_in == 0


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def _block(**kw):
    p = api.normal_params()
    for k, v in kw.items():
        if k == "viewpoint":
            p.viewpoint[0], p.viewpoint[1], p.viewpoint[2] = v
        else:
            setattr(p, k, v)
    return p


BAD_PARAMS = [("k", 2), ("k", 0), ("k", 33), ("k", -5), ("orient", 2), ("orient", -1), ("search_radius", -0.5), ("search_radius", np.nan),
              ("search_radius", np.inf), ("viewpoint", (np.nan, 0.0, 0.0)), ("viewpoint", (0.0, np.inf, 0.0)), ("viewpoint", (0.0, 0.0, -np.inf))]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    if field != "orient":
        with pytest.raises(ValueError, match=field):
            api.normal_params(**{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.normals(CLOUD, p), lambda: c.normals_device(0, 10, 3, p, 1), lambda: c.target_normals(p)):
        with pytest.raises(ValueError, match=field):
            call()


def test_a_viewpoint_that_is_not_three_values_and_a_block_that_is_not_one_are_refused():
    with pytest.raises(ValueError, match="viewpoint"):
        api.normal_params(viewpoint=(0.0, 1.0))
    for call in (lambda: _ctx().normals(CLOUD, api.voxel_params(0.1)), lambda: _ctx().normals_device(0, 10, 3, api.outlier_params(), 1),
                 lambda: _ctx().target_normals(api.place_params())):
        with pytest.raises(ValueError, match="normal_params"):
            call()


def test_clouds_and_outputs_are_checked():
    c = _ctx()
    for call in (lambda: c.normals(np.zeros((4, 2), np.float32)), lambda: c.normals(np.zeros((4, 3), np.float64)),
                 lambda: c.normals(np.zeros(12, np.float32))):
        with pytest.raises(ValueError, match="float32"):
            call()
    with pytest.raises(ValueError, match="stride"):
        c.normals_device(0, 10, 2, None, 1)
    for call in (lambda: c.normals_device(0, -1, 3, None, 1), lambda: c.normals_device(0, 2 ** 31, 3, None, 1)):
        with pytest.raises(ValueError, match="points"):
            call()
    for call in (lambda: c.normals(CLOUD, want_normals=False, want_curvature=False), lambda: c.normals_device(0, 10, 3),
                 lambda: c.target_normals(want_normals=False, want_curvature=False, want_eigenvalues=False)):
        with pytest.raises(ValueError, match="at least one"):
            call()
