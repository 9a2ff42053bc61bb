"""Arguments the outlier methods of Context check before anything reaches the library (no device needed), the parameter blocks against the
header and dcreg_sizeof, and the default parameters."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)


def test_the_parameter_blocks_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.OutlierParams._fields_] == ["mode", "k", "std_mul", "search_radius", "radius", "min_neighbors", "reserved_"]
    assert [f[0] for f in api.OutlierInfo._fields_] == ["n_in", "n_finite", "n_sparse", "n_out", "mean", "stddev", "threshold"]
    assert C.sizeof(api.OutlierParams) == 40 and C.sizeof(api.OutlierInfo) == 56
    assert L.dcreg_sizeof(b"dcreg_outlier_params") == C.sizeof(api.OutlierParams)
    assert L.dcreg_sizeof(b"dcreg_outlier_info") == C.sizeof(api.OutlierInfo)
    assert api.OUTLIER_MODES == {"statistical": 0, "radius": 1}


def test_the_default_parameters():
    p = api.OutlierParams()
    assert api.load().dcreg_default_outlier_params(C.byref(p)) == api.OK
    assert (p.mode, p.k, p.std_mul, p.search_radius, p.radius, p.min_neighbors) == (0, 8, 2.0, 0.0, 0.5, 3)
    assert bytes(p) == bytes(api.outlier_params())
    assert api.load().dcreg_default_outlier_params(None) == -1
    q = api.outlier_params("radius", radius=0.25, min_neighbors=7)
    assert (q.mode, q.radius, q.min_neighbors) == (1, 0.25, 7)
    api.outlier_params(k=1)
    api.outlier_params(k=32, std_mul=-1.0, search_radius=3.0)


def _block(**kw):
    p = api.outlier_params("radius" if set(kw) & {"radius", "min_neighbors"} else "statistical")
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


BAD_PARAMS = [("k", 0), ("k", 33), ("k", -1), ("std_mul", np.nan), ("std_mul", np.inf), ("search_radius", -0.5), ("search_radius", np.nan),
              ("search_radius", np.inf), ("radius", 0.0), ("radius", -1.0), ("radius", np.nan), ("radius", np.inf), ("min_neighbors", 0),
              ("min_neighbors", -4), ("mode", 2), ("mode", -1)]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    if field != "mode":
        with pytest.raises(ValueError, match=field):
            api.outlier_params("radius" if field in ("radius", "min_neighbors") else "statistical", **{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.outlier_filter(CLOUD, p), lambda: c.outlier_filter_device(0, 10, 3, 0, 10, p), lambda: c.set_source_outliers(CLOUD, p),
                 lambda: c.set_source_outliers_device(0, 10, 3, p), lambda: c.set_target_outliers(CLOUD, 1.0, p),
                 lambda: c.set_target_outliers_device(0, 10, 3, 1.0, p), lambda: c.remove_outliers(p)):
        with pytest.raises(ValueError, match=field):
            call()


def test_a_mode_name_and_a_block_that_is_not_one_are_refused():
    with pytest.raises(ValueError, match="mode"):
        api.outlier_params("median")
    for call in (lambda: _ctx().outlier_filter(CLOUD, api.voxel_params(0.1)), lambda: _ctx().remove_outliers(api.place_params())):
        with pytest.raises(ValueError, match="outlier_params"):
            call()


def test_clouds_and_voxel_blocks_are_checked_as_the_voxel_calls_check_them():
    c = _ctx()
    for call in (lambda: c.outlier_filter(np.zeros((4, 2), np.float32)), lambda: c.set_source_outliers(np.zeros((4, 3), np.float64)),
                 lambda: c.set_target_outliers(np.zeros(12, np.float32), 1.0)):
        with pytest.raises(ValueError, match="float32"):
            call()
    for call in (lambda: c.outlier_filter_device(0, 10, 2, 0, 10), lambda: c.set_source_outliers_device(0, 10, 2),
                 lambda: c.set_target_outliers_device(0, 10, 1, 1.0)):
        with pytest.raises(ValueError, match="stride"):
            call()
    for call in (lambda: c.outlier_filter_device(0, -1, 3, 0, 10), lambda: c.set_source_outliers_device(0, 2 ** 31, 3),
                 lambda: c.set_target_outliers_device(0, 2 ** 31, 3, 1.0)):
        with pytest.raises(ValueError, match="points"):
            call()
    with pytest.raises(ValueError, match="capacity"):
        c.outlier_filter_device(0, 10, 3, 0, -1)
    for call in (lambda: c.set_source_outliers(CLOUD, leaf=0.0), lambda: c.set_target_outliers(CLOUD, 1.0, leaf=[0.1, 0.1]),
                 lambda: c.set_source_outliers_device(0, 10, 3, leaf=np.nan)):
        with pytest.raises(ValueError, match="leaf"):
            call()
    with pytest.raises(ValueError, match="voxel mode"):
        c.set_source_outliers(CLOUD, leaf=0.1, mode="median")
