"""The numpy reference of the keyframe store (tests/keyframes_ref.py) checked against itself: what the rules of include/dcreg.h imply."""
import numpy as np

import keyframes_ref as kr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rot_z(deg, t=(0.0, 0.0, 0.0)):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


def store():
    rng = np.random.default_rng(3)
    return [rng.uniform(-4, 4, (n, 3)).astype(np.float32) for n in (40, 0, 7, 120)]


def test_an_identity_pose_returns_the_stored_values_and_minus_zero_becomes_plus_zero():
    s = store()
    s[2][1] = [-0.0, 0.0, -0.0]
    (out,), info = kr.submaps_ref(s, [[(2, np.eye(4))]])
    assert np.array_equal(out, s[2])                        # values: -0.0 == +0.0
    assert np.array_equal(bits(out[1]), bits(np.zeros(3)))  # bits: 1 * -0.0 + 0 * y + 0 * z + 0 = +0.0
    keep = np.ones(len(out), bool)
    keep[1] = False
    assert np.array_equal(bits(out[keep]), bits(s[2][keep]))
    assert info == {"n_in": 7, "n_finite": 7, "n_voxels": 0, "n_out": 7}


def test_a_repeated_member_doubles_the_count_without_moving_the_centroid():
    s = store()
    T = rot_z(30.0, (1.0, -2.0, 0.5))
    # a power-of-two leaf and one voxel's worth of exactly representable points: the sums are exact, so the centroid of the doubled
    # sequence is bitwise the single one's
    s[0] = (np.random.default_rng(8).integers(0, 64, (40, 3)) / 64.0).astype(np.float32)
    (one,), i1 = kr.submaps_ref(s, [[(0, np.eye(4))]], leaf=1.0)
    (two,), i2 = kr.submaps_ref(s, [[(0, np.eye(4)), (0, np.eye(4))]], leaf=1.0)
    assert len(one) == 1 and np.array_equal(bits(one), bits(two))
    assert i2["n_in"] == 2 * i1["n_in"] and i2["n_voxels"] == i1["n_voxels"]
    # min_points counts the repeats: a voxel of one point survives min_points = 2 only when its member is repeated
    (a,), _ = kr.submaps_ref(s, [[(2, T)]], leaf=1e-3, min_points=2)
    (b,), _ = kr.submaps_ref(s, [[(2, T), (2, T)]], leaf=1e-3, min_points=2)
    assert len(a) == 0 and len(b) == 7
    # ... and a generic cloud moves by rounding only
    (c1,), _ = kr.submaps_ref(s, [[(3, T)]], leaf=0.5)
    (c2,), _ = kr.submaps_ref(s, [[(3, T), (3, T)]], leaf=0.5)
    assert c1.shape == c2.shape and np.allclose(c1, c2, rtol=0, atol=1e-6)


def test_member_order_changes_the_raw_output_and_the_first_mode():
    s = store()
    s[2] = s[0][:7] + np.float32(0.001)        # the same voxels as the head of keyframe 0, other points
    A, B = (0, rot_z(0.0)), (2, rot_z(0.0))
    (ab,), _ = kr.submaps_ref(s, [[A, B]])
    (ba,), _ = kr.submaps_ref(s, [[B, A]])
    assert np.array_equal(bits(ab[:40]), bits(s[0] + np.float32(0.0))) and np.array_equal(bits(ba[:7]), bits(s[2] + np.float32(0.0)))
    assert not np.array_equal(bits(ab), bits(ba))
    (fab,), _ = kr.submaps_ref(s, [[A, B]], leaf=0.5, mode="first")
    (fba,), _ = kr.submaps_ref(s, [[B, A]], leaf=0.5, mode="first")
    assert fab.shape == fba.shape and not np.array_equal(bits(fab), bits(fba))


def test_a_submap_does_not_depend_on_the_other_submaps_of_the_call():
    s = store()
    members = [[(0, rot_z(10.0)), (3, rot_z(-5.0, (2.0, 0.0, 0.0)))], [], [(1, np.eye(4))], [(3, rot_z(90.0)), (0, np.eye(4)), (3, rot_z(90.0))]]
    for leaf in (None, 0.4):
        together, info = kr.submaps_ref(s, members, leaf)
        n = 0
        for g, sub in enumerate(members):
            (alone,), i = kr.submaps_ref(s, [sub], leaf)
            assert alone.shape == together[g].shape and np.array_equal(bits(alone), bits(together[g]))
            n += i["n_out"]
        assert info["n_out"] == n and len(together[1]) == 0 and len(together[2]) == 0


def test_an_overflowing_pose_gives_inf_that_the_voxel_form_drops():
    s = [np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], np.float32)]
    T = np.eye(4)
    T[0, 0] = 1e39
    (raw,), _ = kr.submaps_ref(s, [[(0, T)]])
    assert np.isinf(raw[0, 0]) and raw[1, 0] == 0.0
    (v,), info = kr.submaps_ref(s, [[(0, T)]], leaf=0.5)
    assert len(v) == 1 and info["n_in"] - info["n_finite"] == 1
