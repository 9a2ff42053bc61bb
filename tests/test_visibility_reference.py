"""Hand-made truths held against the numpy reference of the visibility rule (tests/visibility_ref.py), and the conditions the shared scene has to
meet before the device is compared with the reference on it.  No device needed."""
import numpy as np

import visibility_ref as vr
from dcreg_amd import api

I = np.eye(4)


def f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def shifted(x, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


def test_one_point_and_one_pixel():
    p = api.visibility_params(rows=1, cols=1, window=0)
    store = [f32([[10.0, 2.0, 1.0], [20.0, -3.0, 2.0]])]
    r = np.float32(np.sqrt(10.0 * 10.0 + 2.0 * 2.0 + 1.0))
    assert np.array_equal(vr.range_image(store[0], p), [[r]])                     # the nearer of the two
    q = f32([[5.0, 1.0, 0.5], [10.0, 2.0, 1.0], [15.0, 3.0, 1.5], [200.0, 0.0, 0.0], [9.99, 2.0, 1.0]])
    through, observed = vr.votes(q, store, [(0, I)], p)
    # 5.12 m: seen through.  The image's own point: its float range against its double range decides, with the margins it stands.  15.4 m:
    # behind the surface.  200 m: beyond max_range, no vote.  1 cm in front: inside the margin.
    assert list(observed) == [1, 1, 1, 0, 1] and list(through) == [1, 0, 0, 0, 0]
    # the sensor moved 4 m towards the points: its image is the stored one, the map points are 4 m nearer in its frame
    through, observed = vr.votes(q + np.float32([4.0, 0.0, 0.0]), store, [(0, shifted(4.0))], p)
    assert list(observed) == [1, 1, 1, 0, 1] and list(through) == [1, 0, 0, 0, 0]


def test_the_window_wraps_across_column_0_and_the_last_column():
    store = [f32([[10.0, -1.0, 0.2]])]                   # azimuth just below 2 pi: the last column
    q = f32([[5.0, 0.5, 0.1]])                           # azimuth just above 0: column 0
    p0 = api.visibility_params(rows=1, cols=8, window=0)
    assert np.isfinite(vr.range_image(store[0], p0)).nonzero()[1].tolist() == [7]
    assert [list(v) for v in vr.votes(q, store, [(0, I)], p0)] == [[0], [0]]        # its own pixel is empty: no vote
    p1 = api.visibility_params(rows=1, cols=8, window=1)
    assert [list(v) for v in vr.votes(q, store, [(0, I)], p1)] == [[1], [1]]        # column -1 is column 7
    # ... and from the other side: the image point in column 0, the map point in column 7
    store = [f32([[10.0, 1.0, 0.2]])]
    q = f32([[5.0, -0.5, 0.1]])
    assert [list(v) for v in vr.votes(q, store, [(0, I)], p0)] == [[0], [0]]
    assert [list(v) for v in vr.votes(q, store, [(0, I)], p1)] == [[1], [1]]
    # a window wider than the image covers it once
    p3 = api.visibility_params(rows=1, cols=2, window=3)
    assert [list(v) for v in vr.votes(q, store, [(0, I)], p3)] == [[1], [1]]


def test_the_window_is_clipped_at_the_top_and_bottom_rows():
    p = lambda w: api.visibility_params(rows=4, cols=4, elev_min=-0.4, elev_max=0.4, window=w)      # noqa: E731  (rows of 0.2 rad)
    top, bottom = [10.0, 1.0, 10.0 * np.tan(0.3)], [10.0, 1.0, -10.0 * np.tan(0.3)]
    store = [f32([bottom])]
    img = vr.range_image(store[0], p(0))
    assert np.isfinite(img).nonzero()[0].tolist() == [3]
    q = f32([[0.5 * v for v in top]])                    # row 0
    assert vr.pixels(q.astype(np.float64), p(0))[1].tolist() == [0]
    for w, seen in ((0, 0), (1, 0), (2, 0), (3, 1)):      # rows do not wrap: row 3 enters only with the window that reaches it
        assert [list(v) for v in vr.votes(q, store, [(0, I)], p(w))] == [[seen], [seen]], w
    store = [f32([top])]
    q = f32([[0.5 * v for v in bottom]])                 # row 3
    for w, seen in ((0, 0), (1, 0), (2, 0), (3, 1)):
        assert [list(v) for v in vr.votes(q, store, [(0, I)], p(w))] == [[seen], [seen]], w


def test_an_empty_window_casts_no_vote_and_points_outside_the_image_neither():
    p = api.visibility_params(rows=8, cols=16, window=1)
    store = [f32([[10.0, 0.5, 0.3]]), np.zeros((0, 3), np.float32)]
    q = f32([[-5.0, 0.5, 0.3],          # the far side: nothing in its window
             [5.0, 0.25, 8.0],          # above the elevation span
             [5.0, 0.25, -8.0],         # below it
             [0.1, 0.01, 0.01],         # nearer than min_range
             [5.0, 0.25, 0.15]])        # in front of the image point
    through, observed = vr.votes(q, store, [(0, I), (1, I)], p)      # (an empty keyframe has an empty image)
    assert list(observed) == [0, 0, 0, 0, 1] and list(through) == [0, 0, 0, 0, 1]
    assert not np.isfinite(vr.range_image(store[1], p)).any()


def test_min_ratio_and_min_votes():
    p = api.visibility_params(rows=1, cols=1, window=0, min_votes=2)
    far, near = f32([[30.0, 1.0, 0.5]]), f32([[5.0, 1.0 / 6.0, 1.0 / 12.0]])
    store = [far, far, near, near, near]
    q = f32([[10.0, 1.0 / 3.0, 1.0 / 6.0]])
    members = [(k, I) for k in range(5)]
    through, observed = vr.votes(q, store, members, p)
    assert list(through) == [2] and list(observed) == [5]          # a repeated image votes again
    for ratio, gone in ((0.0, True), (0.4, True), (0.41, False), (1.0, False)):
        pr = api.visibility_params(rows=1, cols=1, window=0, min_votes=2, min_ratio=ratio)
        assert vr.removed(through, observed, pr).tolist() == [gone], ratio
        assert vr.filter_ref(q, store, members, pr)[4]["n_flagged"] == int(gone)
    assert vr.removed(through, observed, api.visibility_params(min_votes=3)).tolist() == [False]
    kept, keep, th, ob, info = vr.filter_ref(np.concatenate([q, f32([[np.nan, 0.0, 0.0]])]), store, members, p)
    assert info == {"n_in": 2, "n_finite": 1, "n_observed": 1, "n_flagged": 1, "n_out": 0, "n_members": 5}
    assert keep.tolist() == [False, False] and th.tolist() == [2, 0] and ob.tolist() == [5, 0] and kept.shape == (0, 3)


def test_the_image_takes_the_minimum_of_the_float_ranges_whatever_the_order():
    rng = np.random.default_rng(3)
    d = np.array([0.8, 0.5, 0.1]) / np.linalg.norm([0.8, 0.5, 0.1])
    pts = (d[None, :] * rng.uniform(3.0, 40.0, 500)[:, None] + rng.normal(0.0, 1e-4, (500, 3))).astype(np.float32)
    p = api.visibility_params(rows=8, cols=16)
    img = vr.range_image(pts, p)
    assert np.isfinite(img).sum() == 1
    r = np.sqrt((pts.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    assert img[np.isfinite(img)][0] == r.min()
    assert np.array_equal(vr.range_image(pts[rng.permutation(500)], p).view(np.uint32), img.view(np.uint32))


def test_the_scene_meets_its_conditions():
    """Conditions on the choice of scene, not accuracy claims about the device: no stored point and no (map point, member) pair lies within
    1e-9 of a pixel edge, and with the default parameters the reference takes out most of the mover and next to nothing else."""
    sc = vr.mover_scene()
    p = api.visibility_params()
    members = list(enumerate(sc["poses"]))
    assert len(sc["store"]) == vr.N_SWEEPS == 12
    assert vr.ambiguous(sc["store"], p, sc["map"], members) == 0
    keep = vr.filter_ref(sc["map"], sc["store"], members, p)[1]
    mover = sc["in_mover"]
    assert mover.sum() > 5000
    assert (~keep[mover]).mean() >= 0.70
    assert (~keep[~mover]).mean() <= 0.005
    # the minimum over the window is part of the rule: without it the ground at grazing incidence goes
    keep0 = vr.filter_ref(sc["map"], sc["store"], members, api.visibility_params(window=0))[1]
    assert (~keep0[~mover]).mean() > 0.05
