"""Arguments the visibility methods of Context check before anything reaches the library (no device needed), and the new symbols of the
built library with the argument types the header declares."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

I = np.eye(4)
CLOUD = np.zeros((10, 3), np.float32)


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_every_new_symbol_is_exported_with_the_declared_argument_types():
    L = api.load()
    vp, i64, i64p, dp = C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double)
    sp, si = C.POINTER(api.VisibilityParams), C.POINTER(api.VisibilityInfo)
    images = [vp, i64, i64p, sp, vp]
    filt = [vp, vp, i64, i64, i64, i64p, dp, sp, vp, i64, i64p, vp, vp, vp, si]
    want = {"dcreg_default_visibility_params": [sp], "dcreg_keyframes_range_images": images, "dcreg_keyframes_range_images_device": images,
            "dcreg_visibility_filter": filt, "dcreg_visibility_filter_device": filt, "dcreg_target_remove_dynamic": [vp, i64, i64p, dp, sp, si]}
    for name, argtypes in want.items():
        assert name in api.EXPORTS
        assert list(getattr(L, name).argtypes) == argtypes, name
    assert L.dcreg_sizeof(b"dcreg_visibility_params") == C.sizeof(api.VisibilityParams) == 72
    assert L.dcreg_sizeof(b"dcreg_visibility_info") == C.sizeof(api.VisibilityInfo) == 48
    # a null context is refused by every call
    p = api.visibility_params()
    n_out = C.c_int64(0)
    assert L.dcreg_keyframes_range_images(None, 0, None, C.byref(p), None) == -1
    assert L.dcreg_visibility_filter(None, None, 0, 3, 0, None, None, C.byref(p), None, 0, C.byref(n_out), None, None, None, None) == -1
    assert L.dcreg_target_remove_dynamic(None, 0, None, None, C.byref(p), None) == -1
    assert L.dcreg_default_visibility_params(None) == -1


def test_the_defaults_are_the_headers():
    d = api.VisibilityParams()
    assert api.load().dcreg_default_visibility_params(C.byref(d)) == 0
    assert bytes(d) == bytes(api.visibility_params())
    assert (d.rows, d.cols, d.min_range, d.max_range, d.margin_abs, d.margin_rel, d.window, d.min_votes, d.min_ratio) == \
        (64, 1024, 0.5, 80.0, 0.2, 0.01, 1, 2, 0.0)
    assert d.elev_min == -np.pi / 8 and d.elev_max == np.pi / 8


BAD_PARAMS = [dict(rows=0), dict(rows=257), dict(cols=0), dict(cols=4097), dict(rows=2.0), dict(cols=True), dict(elev_min=0.4, elev_max=0.4),
              dict(elev_min=0.5, elev_max=0.1), dict(elev_min=-1.6), dict(elev_max=1.6), dict(elev_min=np.nan), dict(elev_max=np.inf),
              dict(min_range=-0.1), dict(min_range=80.0), dict(max_range=np.inf), dict(min_range=np.nan), dict(margin_abs=-1e-9),
              dict(margin_abs=np.inf), dict(margin_rel=-0.01), dict(margin_rel=np.nan), dict(window=-1), dict(window=4), dict(window=1.0),
              dict(min_votes=0), dict(min_votes="2"), dict(min_ratio=-0.1), dict(min_ratio=1.01), dict(min_ratio=np.nan)]


@pytest.mark.parametrize("kw", BAD_PARAMS, ids=[str(k) for k in range(len(BAD_PARAMS))])
def test_parameters_outside_the_headers_ranges_are_refused(kw):
    with pytest.raises(ValueError, match=next(iter(kw)).split("_")[0]):
        api.visibility_params(**kw)


def test_the_edges_of_the_ranges_are_accepted():
    api.visibility_params(rows=1, cols=1, window=0, min_votes=1, min_ratio=1.0, min_range=0.0, margin_abs=0.0, margin_rel=0.0,
                          elev_min=-0.5 * np.pi, elev_max=0.5 * np.pi)
    api.visibility_params(rows=256, cols=4096, window=3)


def test_a_block_changed_after_it_was_made_or_of_another_type_is_refused_by_every_call():
    c = _ctx()
    members = [(0, I)]
    broken = api.visibility_params()
    broken.window = 9
    for block, what in ((broken, "window"), (api.outlier_params(), "visibility_params"), ({"rows": 4}, "visibility_params")):
        for call in (lambda: c.keyframe_range_images([0], block), lambda: c.keyframe_range_images_device([0], 0, block),
                     lambda: c.visibility_filter(CLOUD, members, block), lambda: c.visibility_filter_device(0, 10, 3, members, 0, 10, block),
                     lambda: c.remove_dynamic(members, block)):
            with pytest.raises(ValueError, match=what):
                call()


@pytest.mark.parametrize("bad", [[1.0], ["3"], [None], [True], [-1], [[0, 1]], np.array([0.5])], ids=repr)
def test_ids_that_are_not_integers_are_refused(bad):
    c = _ctx()
    for call in (lambda: c.keyframe_range_images(bad), lambda: c.keyframe_range_images_device(bad, 0),
                 lambda: c.visibility_filter(CLOUD, (np.asarray(bad).reshape(-1), np.stack([I])), None),
                 lambda: c.remove_dynamic([(bad[0], I)])):
        with pytest.raises(ValueError, match="ids|members"):
            call()


def _nonfinite(v):
    T = np.eye(4)
    T[1, 3] = v
    return T


BAD_MEMBERS = [7, "members", [7], [(0, I, 1)], [(0,)], [(0, np.eye(3))], [(0, I), (1, np.zeros((3, 4)))], [(0, "pose")],
               [(0, I), (1, _nonfinite(np.nan))], [(0, _nonfinite(np.inf))], (np.array([0, 1]), np.stack([I])), (np.array([0]), np.zeros((1, 3, 4)))]


@pytest.mark.parametrize("bad", BAD_MEMBERS, ids=[str(k) for k in range(len(BAD_MEMBERS))])
def test_member_lists_of_the_wrong_shape_and_poses_that_are_not_finite_are_refused(bad):
    c = _ctx()
    for call in (lambda: c.visibility_filter(CLOUD, bad), lambda: c.visibility_filter_device(0, 10, 3, bad, 0, 10), lambda: c.remove_dynamic(bad)):
        with pytest.raises(ValueError, match="members"):
            call()


def test_members_are_taken_as_a_list_of_pairs_or_as_a_pair_of_arrays():
    Ts = np.stack([I, _nonfinite(2.0)])
    a = api._vote_members([(3, Ts[0]), (5, Ts[1])], "t")
    b = api._vote_members((np.array([3, 5], np.int32), Ts), "t")
    assert np.array_equal(a[0], b[0]) and a[0].dtype == np.int64 and np.array_equal(a[1], b[1]) and a[1].shape == (2, 12)
    assert list(a[1][1]) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 0]
    ids, poses = api._vote_members([], "t")
    assert ids.shape == (0,) and poses.shape == (0, 12)


def test_clouds_and_capacities_of_the_filter():
    c = _ctx()
    members = [(0, I)]
    for bad in (np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float64), np.zeros(12, np.float32)):
        with pytest.raises(ValueError, match="float32"):
            c.visibility_filter(bad, members)
    with pytest.raises(ValueError, match="points"):
        c.visibility_filter_device(0, -1, 3, members, 0, 10)
    with pytest.raises(ValueError, match="stride"):
        c.visibility_filter_device(0, 10, 2, members, 0, 10)
    for cap in (-1, 2.5, None):
        with pytest.raises(ValueError, match="capacity"):
            c.visibility_filter_device(0, 10, 3, members, 0, cap)
