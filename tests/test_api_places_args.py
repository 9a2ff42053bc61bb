"""Arguments the place-recognition methods of Context check before anything reaches the library (no device needed), the parameter blocks
against the header and dcreg_sizeof, the default parameters, and place_guess."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)
DESC = np.ones((2, 20, 60), np.float32)


def test_the_parameter_blocks_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.PlaceParams._fields_] == ["n_rings", "n_sectors", "max_range", "min_range", "z_offset"]
    assert [f[0] for f in api.PlaceInfo._fields_] == ["n_in", "n_finite", "n_used"]
    assert C.sizeof(api.PlaceParams) == 32 and C.sizeof(api.PlaceInfo) == 24
    assert L.dcreg_sizeof(b"dcreg_place_params") == C.sizeof(api.PlaceParams)
    assert L.dcreg_sizeof(b"dcreg_place_info") == C.sizeof(api.PlaceInfo)


def test_the_default_parameters():
    p = api.PlaceParams()
    assert api.load().dcreg_default_place_params(C.byref(p)) == api.OK
    assert (p.n_rings, p.n_sectors, p.max_range, p.min_range, p.z_offset) == (20, 60, 80.0, 0.0, 2.0)
    q = api.place_params()
    assert bytes(p) == bytes(q)
    assert api.load().dcreg_default_place_params(None) == -1
    q = api.place_params(8, 128, 30.0, 1.5, -0.25)
    assert (q.n_rings, q.n_sectors, q.max_range, q.min_range, q.z_offset) == (8, 128, 30.0, 1.5, -0.25)
    api.place_params(64, 1)
    api.place_params(1, 128)


def _block(**kw):
    p = api.PlaceParams()
    p.n_rings, p.n_sectors, p.max_range, p.min_range, p.z_offset = 20, 60, 80.0, 0.0, 2.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ctx(reset=True):
    c = object.__new__(api.Context)          # no device: the checks come first
    if reset:
        c._place_shape = (20, 60)
    return c


BAD_PARAMS = [("n_rings", 0), ("n_rings", 65), ("n_rings", -3), ("n_sectors", 0), ("n_sectors", 129), ("max_range", 0.0), ("max_range", -1.0),
              ("max_range", np.nan), ("max_range", np.inf), ("min_range", -0.1), ("min_range", np.nan), ("min_range", np.inf),
              ("min_range", 80.0), ("min_range", 90.0), ("z_offset", np.nan), ("z_offset", np.inf), ("z_offset", -np.inf)]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    with pytest.raises(ValueError, match=field):
        api.place_params(**{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.place_descriptors([CLOUD], p), lambda: c.place_descriptors_device(0, [0, 10], 3, 0, p), lambda: c.places_reset(p)):
        with pytest.raises(ValueError, match=field):
            call()


def test_a_block_that_is_not_one_is_refused():
    with pytest.raises(ValueError, match="place_params"):
        _ctx().places_reset(api.voxel_params(0.1))


def test_database_calls_before_a_reset_are_refused():
    c = _ctx(reset=False)
    for call in (lambda: c.places_add(DESC), lambda: c.places_add_clouds([CLOUD]), lambda: c.places_add_clouds_device(0, [0, 10], 3),
                 lambda: c.places_add_source(), lambda: c.places_get(0, 0), lambda: c.places_query(DESC, 1, 0, 0),
                 lambda: c.places_query_clouds([CLOUD], 1, 0, 0), lambda: c.places_query_clouds_device(0, [0, 10], 3, 1, 0, 0),
                 lambda: c.places_query_source(1, 0, 0)):
        with pytest.raises(ValueError, match="places_reset"):
            call()


@pytest.mark.parametrize("first,last,k,match", [(3, 2, 1, "range"), (-1, 2, 1, "range"), (0, 2, 0, "k"), (0, 2, 65, "k"), (0, 2, -1, "k")])
def test_bad_ranges_and_k_are_refused_by_every_query(first, last, k, match):
    c = _ctx()
    for call in (lambda: c.places_query(DESC, k, first, last), lambda: c.places_query_clouds([CLOUD], k, first, last),
                 lambda: c.places_query_clouds_device(0, [0, 10], 3, k, first, last), lambda: c.places_query_source(k, first, last)):
        with pytest.raises(ValueError, match=match):
            call()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_descriptors_that_are_not_finite_or_of_another_shape_are_refused(bad):
    c = _ctx()
    d = DESC.copy()
    d[1, 3, 7] = bad
    for call in (lambda: c.places_add(d), lambda: c.places_query(d, 1, 0, 0)):
        with pytest.raises(ValueError, match="finite"):
            call()
    for wrong in (np.ones((2, 20, 59), np.float32), np.ones((2, 1199), np.float32), np.ones(7, np.float32)):
        for call in (lambda: c.places_add(wrong), lambda: c.places_query(wrong, 1, 0, 0)):
            with pytest.raises(ValueError, match="1200 floats"):
                call()


def test_clouds_are_checked_as_the_voxel_calls_check_them():
    c = _ctx()
    for call in (lambda: c.place_descriptors([np.zeros((4, 2), np.float32)]), lambda: c.places_add_clouds([np.zeros((4, 3), np.float64)]),
                 lambda: c.places_query_clouds([np.zeros(12, np.float32)], 1, 0, 0)):
        with pytest.raises(ValueError, match="float32"):
            call()
    with pytest.raises(ValueError, match="columns"):
        c.places_add_clouds([np.zeros((4, 3), np.float32), np.zeros((4, 4), np.float32)])
    with pytest.raises(ValueError, match="offsets"):
        c.place_descriptors((CLOUD, [0, 4]))
    for call in (lambda: c.place_descriptors_device(0, [1, 10], 3, 0), lambda: c.places_add_clouds_device(0, [0, 10, 4], 3),
                 lambda: c.places_query_clouds_device(0, [], 3, 1, 0, 0)):
        with pytest.raises(ValueError, match="offsets"):
            call()
    for call in (lambda: c.place_descriptors_device(0, [0, 10], 2, 0), lambda: c.places_add_clouds_device(0, [0, 10], 2),
                 lambda: c.places_query_clouds_device(0, [0, 10], 2, 1, 0, 0)):
        with pytest.raises(ValueError, match="stride"):
            call()
    with pytest.raises(ValueError, match="first"):
        c.places_get(-1, 2)
    with pytest.raises(ValueError, match="first"):
        c.places_get(0, -2)


@pytest.mark.parametrize("n_sectors,shift", [(60, 0), (60, 1), (60, 15), (60, 59), (128, 77), (7, 3), (1, 0)])
def test_place_guess_is_a_rotation_about_z_by_the_stated_angle(n_sectors, shift):
    T = api.place_guess(shift, n_sectors)
    a = 2.0 * np.pi * shift / n_sectors
    assert T.shape == (4, 4) and T.dtype == np.float64
    assert np.array_equal(T[:3, 3], np.zeros(3)) and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.array_equal(T[2, :3], [0, 0, 1]) and np.array_equal(T[:3, 2], [0, 0, 1])
    assert np.allclose(T[:2, :2], [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], rtol=0, atol=1e-15)
    assert np.allclose(T[:3, :3].T @ T[:3, :3], np.eye(3), rtol=0, atol=1e-15) and np.linalg.det(T[:3, :3]) > 0
    # +x of the query lands at azimuth a in the entry's frame
    v = T[:3, :3] @ [1.0, 0.0, 0.0]
    assert np.isclose(np.arctan2(v[1], v[0]) % (2 * np.pi), a % (2 * np.pi), rtol=0, atol=1e-12)


@pytest.mark.parametrize("n_sectors,shift", [(60, 60), (60, -1), (0, 0), (129, 3)])
def test_place_guess_refuses_shifts_outside_the_descriptor(n_sectors, shift):
    with pytest.raises(ValueError, match="shift|n_sectors"):
        api.place_guess(shift, n_sectors)
