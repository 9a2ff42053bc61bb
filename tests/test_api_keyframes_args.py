"""Arguments the keyframe methods of Context check before anything reaches the library (no device needed), and the new symbols of the
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
    vpp, vi = C.POINTER(api.VoxelParams), C.POINTER(api.VoxelInfo)
    submaps = [vp, C.c_int, i64p, i64p, dp, vpp, vp, i64, i64p, vi]
    adds = [vp, C.c_int, vp, i64p, i64, i64p]
    want = {"dcreg_keyframes_reset": [vp], "dcreg_keyframes_count": [vp], "dcreg_keyframes_sizes": [vp, i64, i64, i64p],
            "dcreg_keyframes_add_clouds": adds, "dcreg_keyframes_add_clouds_device": adds, "dcreg_keyframes_add_source": [vp, i64p],
            "dcreg_keyframes_get": [vp, i64, vp, i64], "dcreg_keyframes_submaps": submaps, "dcreg_keyframes_submaps_device": submaps,
            "dcreg_set_target_keyframes": [vp, i64, i64p, dp, vpp, C.c_double, vi]}
    for name, argtypes in want.items():
        assert name in api.EXPORTS
        assert list(getattr(L, name).argtypes) == argtypes, name
    assert L.dcreg_keyframes_count.restype is C.c_int64
    # a null context is refused by every call, and counts nothing
    assert L.dcreg_keyframes_count(None) == 0
    assert L.dcreg_keyframes_reset(None) == -1 and L.dcreg_keyframes_add_source(None, None) == -1
    assert L.dcreg_set_target_keyframes(None, 0, None, None, None, 1.0, None) == -1


def test_clouds_of_an_add_are_checked_as_the_voxel_calls_check_them():
    c = _ctx()
    for bad in ([np.zeros((4, 2), np.float32)], [np.zeros((4, 3), np.float64)], [CLOUD, np.zeros(12, np.float32)]):
        with pytest.raises(ValueError, match="float32"):
            c.keyframes_add(bad)
    with pytest.raises(ValueError, match="columns"):
        c.keyframes_add([CLOUD, np.zeros((4, 5), np.float32)])
    for off in ([1, 10], [0, 6, 4, 10], [0, 4], []):
        with pytest.raises(ValueError, match="offsets"):
            c.keyframes_add((CLOUD, off))
    for off in ([1, 10], [0, 6, 4, 10], []):
        with pytest.raises(ValueError, match="offsets"):
            c.keyframes_add_device(0, off, 3)
    with pytest.raises(ValueError, match="stride"):
        c.keyframes_add_device(0, [0, 10], 2)


@pytest.mark.parametrize("bad", [1.0, "3", None, True, -1, np.float32(2)], ids=repr)
def test_ids_that_are_not_integers_are_refused(bad):
    c = _ctx()
    for call in (lambda: c.keyframes_get(bad), lambda: c.keyframes_sizes(bad, 1), lambda: c.keyframe_submaps([[(bad, I)]]),
                 lambda: c.keyframe_submaps_device([[(0, I)], [(bad, I)]], 0, 10), lambda: c.set_target_keyframes([(bad, I)], 0.5)):
        with pytest.raises(ValueError, match="ids"):
            call()
    with pytest.raises(ValueError, match="n:"):
        c.keyframes_sizes(0, -1 if bad is None else bad if bad != -1 else 1.5)


def _nonfinite(v):
    T = np.eye(4)
    T[1, 3] = v
    return T


BAD_POSES = [np.eye(3), np.zeros((3, 4)), np.zeros(16), "pose", _nonfinite(np.nan), _nonfinite(np.inf), _nonfinite(-np.inf)]


@pytest.mark.parametrize("T", BAD_POSES, ids=[str(k) for k in range(len(BAD_POSES))])
def test_poses_that_are_not_4x4_or_not_finite_are_refused(T):
    c = _ctx()
    for call in (lambda: c.keyframe_submaps([[(0, I), (1, T)]]), lambda: c.keyframe_submaps_device([[], [(0, T)]], 0, 10),
                 lambda: c.set_target_keyframes([(0, I), (0, T)], 0.5)):
        with pytest.raises(ValueError, match=r"members\[\d\]\[\d\]"):
            call()


def test_member_lists_of_the_wrong_shape_are_refused():
    c = _ctx()
    for bad in (7, "members", [7], [[7]], [[(0, I, 1)]], [[(0,)]], [["ab"]]):
        with pytest.raises(ValueError, match="members"):
            c.keyframe_submaps(bad)
        with pytest.raises(ValueError, match="members"):
            c.keyframe_submaps_device(bad, 0, 10)
    for bad in (7, [7], [(0, I, 1)], []):
        with pytest.raises(ValueError, match="members"):
            c.set_target_keyframes(bad, 0.5)


def test_voxel_blocks_leaves_and_capacities():
    c = _ctx()
    members = [[(0, I)]]
    for block in (api.place_params(), api.outlier_params(), "0.2", {"leaf": 0.2}):          # a block of the wrong type
        for call in (lambda: c.keyframe_submaps(members, block), lambda: c.keyframe_submaps_device(members, 0, 10, block),
                     lambda: c.set_target_keyframes(members[0], 0.5, block)):
            with pytest.raises(ValueError, match="voxel_params"):
                call()
    broken = api.voxel_params(0.2)
    broken.leaf[1] = -1.0
    wrong_mode = api.voxel_params(0.2)
    wrong_mode.mode = 5
    for leaf, what in ((0.0, "leaf"), (-0.5, "leaf"), (np.nan, "leaf"), ([0.1, 0.2], "leaf"), (np.inf, "leaf"), (broken, "leaf"), (wrong_mode, "mode")):
        for call in (lambda: c.keyframe_submaps(members, leaf), lambda: c.keyframe_submaps_device(members, 0, 10, leaf),
                     lambda: c.set_target_keyframes(members[0], 0.5, leaf)):
            with pytest.raises(ValueError, match=what):
                call()
    with pytest.raises(ValueError, match="voxel mode"):
        c.keyframe_submaps(members, 0.2, mode="median")
    for cap in (-1, 2.5, None):
        with pytest.raises(ValueError, match="capacity"):
            c.keyframe_submaps_device(members, 0, cap)
    with pytest.raises(ValueError, match="search_radius"):
        c.set_target_keyframes(members[0], np.nan)
