"""Visibility votes on the device (dcreg_keyframes_range_images*, dcreg_visibility_filter*, dcreg_target_remove_dynamic) against the numpy
reference of tests/visibility_ref.py, which applies include/dcreg.h's rule literally.  Every comparison is bitwise; nothing has a tolerance.
Every test first asserts that its data has no point and no (point, member) pair within 1e-9 of a pixel edge: only there may the device's
atan2 and numpy's put a point into different pixels.  The reference is the yardstick, never a second device run."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
import visibility_ref as vr
from dcreg_amd import api
from test_gpu_configs import cfg_pair
from test_gpu_device_seam import D2H, DevCloud, _info, hip, strided
from test_gpu_map_update import RADIUS, ZERO, assert_same_as_fresh

pytestmark = pytest.mark.gpu

I64P, DP = C.POINTER(C.c_int64), C.POINTER(C.c_double)
I = np.eye(4)
EMPTY = np.zeros((0, 3), np.float32)
WINDOW_OPTS = [("max_table_entries", 1 << 16), ("roi_index", 2), ("roi_margin", 2.0)]      # a window 2 m beyond what the source needs
SMALL = dict(rows=16, cols=64)


def shell(n, seed, r_lo=2.0, r_hi=40.0, el=0.45):
    """n seeded points at random azimuths, elevations within +-el radians and ranges in [r_lo, r_hi)"""
    rng = np.random.default_rng(9000 + seed)
    az, e, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(-el, el, n), rng.uniform(r_lo, r_hi, n)
    return np.stack([r * np.cos(e) * np.cos(az), r * np.cos(e) * np.sin(az), r * np.sin(e)], 1).astype(np.float32)


def pose(seed, spread=3.0):
    r = np.random.default_rng(600 + seed)
    return h.pose6d_matrix(*r.uniform(-spread, spread, 2), r.uniform(-0.5, 0.5), *h.deg2rad(r.uniform(-4, 4, 2)), h.deg2rad(r.uniform(-180, 180)))


def p12(T):
    T = np.asarray(T, np.float64)
    return np.r_[T[:3, :3].ravel(), T[:3, 3]]


def make_ctx(store):
    c = api.Context(0)
    c.keyframes_reset()
    assert c.keyframes_add(store) == 0
    return c


def same_images(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_images(c, store, ids, p, what=""):
    assert vr.ambiguous([store[i] for i in set(ids)], p) == 0, what
    got = c.keyframe_range_images(ids, p)
    ref = np.stack([vr.range_image(store[i], p) for i in ids]) if len(ids) else np.zeros((0, p.rows, p.cols), np.float32)
    assert same_images(got, ref), (what, [int((g.view(np.uint32) != r.view(np.uint32)).sum()) for g, r in zip(got, ref)])
    return got


def assert_filter(got, ref, what=""):
    kept, mask, through, observed, info = got
    rkept, rmask, rthrough, robserved, rinfo = ref
    assert np.array_equal(through, rthrough) and np.array_equal(observed, robserved), (what, int((through != rthrough).sum()), int((observed != robserved).sum()))
    assert np.array_equal(mask, rmask), what
    assert kept.shape == rkept.shape and np.array_equal(kept.view(np.uint32), rkept.view(np.uint32)), what
    assert info == rinfo, (what, info, rinfo)


def assert_votes(c, store, q, members, p, what=""):
    assert vr.ambiguous([store[i] for i in {i for i, _ in members}], p, q, members) == 0, what
    got = c.visibility_filter(q, members, p)
    assert_filter(got, vr.filter_ref(q, store, members, p), what)
    return got


# ---- 1. range images
TILE_SIZES = [0, 1, 3, 2047, 2048, 2049]       # a tile of k_vis_image = 2048 stored points


@pytest.fixture(scope="module")
def tiles():
    rng = np.random.default_rng(78)
    d = np.array([0.7, -0.6, 0.12]) / np.linalg.norm([0.7, -0.6, 0.12])
    one_pixel = (d[None, :] * rng.uniform(3.0, 60.0, 5000)[:, None] + rng.normal(0.0, 2e-4, (5000, 3))).astype(np.float32)
    store = [shell(n, n) for n in TILE_SIZES] + [shell(int(n), 100 + k) for k, n in enumerate(rng.integers(1, 4, 300))] + [EMPTY.copy(), one_pixel,
                                                                                                                       shell(5000, 7, el=1.4)]
    c = make_ctx(store)
    yield c, store
    c.close()


@pytest.mark.parametrize("kw", [{}, SMALL, dict(rows=1, cols=1), dict(rows=256, cols=4096), dict(rows=7, cols=13, elev_min=-0.2, elev_max=0.9, window=3)],
                         ids=["default", "16x64", "1x1", "256x4096", "7x13"])
def test_the_range_images_are_the_reference(tiles, kw):
    c, store = tiles
    p = api.visibility_params(**kw)
    n = len(store)
    if p.rows * p.cols > 1 << 18:                # the largest image: a handful of keyframes across the tile edges
        assert_images(c, store, [3, 4, 5, 0, n - 2, n - 1], p)
        return
    got = assert_images(c, store, list(range(n)), p, "every keyframe, in store order")      # 300 keyframes of 1 - 3 points share one tile
    assert not np.isfinite(got[0]).any() and not np.isfinite(got[n - 3]).any()              # the empty keyframes
    if kw == SMALL:
        assert np.isfinite(got[n - 2]).sum() == 1                                            # 5000 points in one pixel
        used = vr.pixels(store[n - 1].astype(np.float64), p)[0]                              # points above and below the elevation span are not used
        assert 0.2 < used.mean() < 0.4 and np.isfinite(got[n - 1]).sum() <= used.sum()
    assert_images(c, store, [5, 5, 2, n - 2, 0, 4, 7, 3], p, "repeated ids, out of order")
    assert c.keyframe_range_images([], p).shape == (0, p.rows, p.cols)


def test_points_at_exactly_min_range_and_max_range():
    # squares that compare exactly: 2^2 + 3^2 + 6^2 = 7^2 (used: min_range^2 <= r2), 4^2 + 4^2 + 7^2 = 1^2 + 4^2 + 8^2 = 9^2 (not: r2 < max_range^2)
    pts = np.array([[2, 3, 6], [6, -3, 2], [-3, 2, -6], [4, 4, 7], [1, 4, 8], [-8, 1, -4], [2, 3, 5.99], [4, 3.9, 7.05], [3, -5, 4]], np.float32)
    p = api.visibility_params(rows=32, cols=64, elev_min=-1.3, elev_max=1.3, min_range=7.0, max_range=9.0, window=0, margin_abs=0.0, margin_rel=0.0)
    store = [pts[k:k + 1] for k in range(len(pts))]
    c = make_ctx(store)
    try:
        got = assert_images(c, store, list(range(len(pts))), p)
        assert [int(np.isfinite(g).sum()) for g in got] == [1, 1, 1, 0, 0, 0, 0, 1, 1]
        # ... and as map points under the identity: each looks at an image that holds every point
        c.keyframes_add([pts])
        _, _, through, observed, info = assert_votes(c, store + [pts], pts, [(len(pts), I)], p)
        assert list(observed) == [1, 1, 1, 0, 0, 0, 0, 1, 1] and info["n_observed"] == 5
    finally:
        c.close()


# ---- 2. votes
@pytest.fixture(scope="module")
def five():
    store = [shell(4000, 40 + k, r_lo=3.0, el=0.38) for k in range(5)]
    poses = [pose(k) for k in range(5)]
    rng = np.random.default_rng(11)
    q = rng.uniform([-40, -40, -6], [40, 40, 6], (30_000, 3)).astype(np.float32)
    c = make_ctx(store)
    yield c, store, poses, q
    c.close()


@pytest.mark.parametrize("window", [0, 1, 3])
def test_the_votes_are_the_reference(five, window):
    c, store, poses, q = five
    p = api.visibility_params(window=window, **SMALL)
    members = list(enumerate(poses))
    used, row, col, _ = vr.pixels(vr.sensor_frame(q, poses[0]), p)
    for edge in (row == 0, row == p.rows - 1, col == 0, col == p.cols - 1):        # pixels in the first and last row and column
        assert (used & edge).sum() > 50
    _, _, through, observed, info = assert_votes(c, store, q, members, p)
    assert through.max() >= 3 and 0 < info["n_flagged"] < info["n_observed"] < len(q)
    assert_votes(c, store, q, members, api.visibility_params(window=window, min_ratio=0.5, min_votes=1, **SMALL), "min_ratio")
    assert_votes(c, store, q[:1], members[:1], p, "one point, one member")
    assert_votes(c, store, q, [], p, "no member")
    assert_votes(c, store, EMPTY, members, p, "no point")


def test_a_keyframes_own_points_under_the_identity_with_zero_margins(five):
    """(double)(float)r > r decides: a point whose range rounds UP to float is seen through by its own pixel.  The rule says so and the
    reference agrees; margins are what keeps a static point."""
    c, store, poses, q = five
    p = api.visibility_params(window=0, margin_abs=0.0, margin_rel=0.0, min_votes=1, **SMALL)
    _, mask, through, observed, _ = assert_votes(c, store, store[2], [(2, I)], p)
    assert observed.min() == 1 and 0 < through.sum() < len(through)


def test_points_beyond_every_members_range_are_not_observed(five):
    c, store, poses, q = five
    far = shell(2000, 5, r_lo=150.0, r_hi=300.0)
    _, mask, through, observed, info = assert_votes(c, store, far, list(enumerate(poses)), api.visibility_params(**SMALL))
    assert not observed.any() and not through.any() and mask.all() and info["n_observed"] == 0 and info["n_out"] == len(far)


@pytest.fixture(scope="module")
def mover():
    """the shared scene, a context that holds its sweeps, and the reference's answer with the default parameters (computed once)"""
    sc = vr.mover_scene()
    p = api.visibility_params()
    members = list(enumerate(sc["poses"]))
    assert vr.ambiguous(sc["store"], p, sc["map"], members) == 0
    ref = vr.filter_ref(sc["map"], sc["store"], members, p)
    c = make_ctx(sc["store"])
    yield c, sc, members, p, ref
    c.close()


def test_the_mixed_pose_scene(mover):
    c, sc, members, p, ref = mover
    got = c.visibility_filter(sc["map"], members, p)
    assert_filter(got, ref)
    gone = ~got[1]
    assert gone[sc["in_mover"]].mean() >= 0.70 and gone[~sc["in_mover"]].mean() <= 0.005
    # the members as a pair of arrays, a cloud with further columns
    got = c.visibility_filter(strided(sc["map"], 5), (np.arange(12), np.stack(sc["poses"])), p)
    assert_filter(got, ref, "arrays")


# ---- 3. independence
def test_member_order_batching_repeats_and_a_second_context_do_not_change_a_count(mover):
    c, sc, members, p, ref = mover
    q = sc["map"]
    perm = [members[k] for k in np.random.default_rng(1).permutation(12)]
    assert_filter(c.visibility_filter(q, perm, p), ref, "permuted")
    c.set_option("visibility_max_bytes", 4 * p.rows * p.cols)           # one image per batch
    try:
        assert_filter(c.visibility_filter(q, members, p), ref, "one image per batch")
        assert_filter(c.visibility_filter(q, perm, p), ref, "one image per batch, permuted")
        imgs = c.keyframe_range_images(list(range(12)), p)
    finally:
        c.set_option("visibility_max_bytes", 1 << 28)
    assert same_images(imgs, c.keyframe_range_images(list(range(12)), p))
    assert same_images(imgs, np.stack([vr.range_image(s, p) for s in sc["store"]]))
    c.set_option("visibility_max_bytes", 5 * 4 * p.rows * p.cols)       # 5 + 5 + 2
    try:
        assert_filter(c.visibility_filter(q, members, p), ref, "batches of five")
    finally:
        c.set_option("visibility_max_bytes", 1 << 28)
    twice = members + [members[3], members[3]]
    got = c.visibility_filter(q, twice, p)
    assert_filter(got, vr.filter_ref(q, sc["store"], twice, p), "a repeated member votes again")
    one = vr.votes(q, sc["store"], [members[3]], p)
    assert np.array_equal(got[2], ref[2] + 2 * one[0]) and np.array_equal(got[3], ref[3] + 2 * one[1])
    d = api.Context(0)
    try:
        d.keyframes_reset()
        d.keyframes_add([shell(999, 1)])             # the other store holds something else in front, and a map
        d.set_target(shell(20_000, 2), RADIUS)
        d.keyframes_add(sc["store"])
        assert_filter(d.visibility_filter(q, [(i + 1, T) for i, T in members], p), ref, "a second context")
        assert_filter(c.visibility_filter(q, members, p), ref, "again")
    finally:
        d.close()


# ---- 4. the device form, strided input with NaN rows, the capacity protocol
def read_dev(ptr, n, dtype, cols=1):
    out = np.empty((n, cols) if cols > 1 else n, dtype)
    if n:
        assert hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), out.nbytes, D2H) == 0
    return out


def test_the_device_form_and_the_capacity_protocol(five):
    c, store, poses, q = five
    p = api.visibility_params(**SMALL)
    members = list(enumerate(poses))
    q = q[:9001].copy()
    q[::7, 1] = np.nan
    q[5, 0] = np.inf
    ref = vr.filter_ref(q, store, members, p)
    n, m = len(q), ref[4]["n_out"]
    assert vr.ambiguous(store, p, q, members) == 0 and 0 < ref[4]["n_flagged"] and ref[4]["n_finite"] < n
    assert_filter(c.visibility_filter(strided(q, 6), members, p), ref, "host, stride 6")
    src = DevCloud(strided(q, 6), offset=8)
    out, counts = DevCloud(np.full((n, 3), 7.0, np.float32)), DevCloud(np.full((3 * n, 1), 7.0, np.float32))
    mask_ptr, through_ptr, observed_ptr = counts.ptr, counts.ptr + 4 * n, counts.ptr + 8 * n
    try:
        for cap in (0, m - 1):                  # too small: the sizes come back, nothing is written
            with pytest.raises(api.CapacityError) as e:
                c.visibility_filter_device(src.ptr, n, 6, members, out.ptr, cap, p, mask_ptr, through_ptr, observed_ptr)
            assert e.value.info == ref[4]
            assert np.all(read_dev(out.ptr, n, np.float32, 3) == 7.0) and np.all(read_dev(counts.ptr, 3 * n, np.float32) == 7.0)
        for cap in (m, n):
            n_out, info = c.visibility_filter_device(src.ptr, n, 6, members, out.ptr, cap, p, mask_ptr, through_ptr, observed_ptr)
            assert n_out == m and info == ref[4]
            got = (read_dev(out.ptr, m, np.float32, 3), read_dev(mask_ptr, n, np.uint8).astype(bool), read_dev(through_ptr, n, np.int32),
                   read_dev(observed_ptr, n, np.int32), info)
            assert_filter(got, ref, "device")
            assert np.all(read_dev(out.ptr, n, np.float32, 3)[m:] == 7.0)
        n_out, info = c.visibility_filter_device(src.ptr, n, 6, members, out.ptr, n, p)          # no optional output
        assert n_out == m and info == ref[4]
        imgs = DevCloud(np.zeros((2 * p.rows, p.cols), np.float32))
        try:
            c.keyframe_range_images_device([4, 1], imgs.ptr, p)
            got = read_dev(imgs.ptr, 2 * p.rows * p.cols, np.float32).reshape(2, p.rows, p.cols)
            assert same_images(got, np.stack([vr.range_image(store[4], p), vr.range_image(store[1], p)]))
        finally:
            imgs.free()
    finally:
        src.free()
        out.free()
        counts.free()


# ---- 5. the resident map
def _probe(sc, reach=None):
    """a source cloud for the registrations that compare two maps: every third point of sweep 6 in its stored frame (reach: only those
    within that many metres of the sensor - a source whose window index holds a part of the map, not all of it), a pose 10 cm off"""
    T0 = sc["poses"][6].copy()
    T0[:3, 3] += [0.1, -0.05, 0.02]
    s = sc["store"][6]
    if reach is not None:
        s = s[np.sqrt((s.astype(np.float64) ** 2).sum(1)) < reach]
    return np.ascontiguousarray(s[::3]), T0


def test_remove_dynamic_after_inserts_and_a_crop(mover):
    c, sc, members, p, _ = mover
    cfg, _ = cfg_pair(RADIUS, 30, 0, 1e-5, 1e-3)
    probe, T0 = _probe(sc)
    sizes = np.cumsum([0] + [len(s) for s in sc["store"]])
    A = api.Context(0)
    try:
        A.keyframes_reset()
        A.keyframes_add(sc["store"])
        A.set_target(sc["map"][:sizes[8]], RADIUS)
        for k in range(8, 12):                     # four keyframes inserted, as a mapper does
            A.insert(sc["store"][k], sc["poses"][k])
        lo, hi = [-30.0, -20.0, -1.0], [55.0, 11.0, 6.0]          # the crop takes one wall and the far ends
        A.crop(lo, hi)
        pts = sc["map"].astype(np.float64)
        expected = sc["map"][np.all((pts >= lo) & (pts <= hi), 1)]
        assert np.array_equal(A.target_points().view(np.uint32), expected.view(np.uint32))
        assert vr.ambiguous(sc["store"], p, expected, members) == 0
        ref = vr.filter_ref(expected, sc["store"], members, p)
        info = A.remove_dynamic(members, p)
        assert info == ref[4] and 0 < info["n_flagged"]
        assert_same_as_fresh(A, ref[0], probe, T0, cfg)
        # the survivors voted on again: what the reference says of them, through the same path
        ref2 = vr.filter_ref(ref[0], sc["store"], members, p)
        assert A.remove_dynamic(members, p) == ref2[4]
        assert np.array_equal(A.target_points().view(np.uint32), ref2[0].view(np.uint32)) and A.index_check() == ZERO
    finally:
        A.close()


@pytest.mark.parametrize("order", [1, 0], ids=["cell-order", "index-order"])
def test_remove_dynamic_on_a_capped_map_with_a_window_index(mover, order):
    c, sc, members, p, ref = mover
    cfg, _ = cfg_pair(RADIUS, 30, 0, 1e-5, 1e-3)
    probe, T0 = _probe(sc, reach=10.0)
    prm = api.default_lin_params(RADIUS, 0)
    A = api.Context(0)
    try:
        for k, v in WINDOW_OPTS + [("visibility_order", order)]:
            A.set_option(k, v)
        A.keyframes_reset()
        A.keyframes_add(sc["store"])
        A.set_target(sc["map"], RADIUS)
        A.set_source(probe)
        A.linearize(T0[:3, :3], T0[:3, 3], prm)
        assert A.roi_info()["active"]                # the window is the active index: the votes go over the whole map's points
        assert A.remove_dynamic(members, p) == ref[4]
        assert_same_as_fresh(A, ref[0], probe, T0, cfg, options=WINDOW_OPTS)
    finally:
        A.close()


def test_a_call_that_flags_nothing_changes_nothing_and_one_that_flags_everything_is_refused(mover):
    c, sc, members, p, _ = mover
    probe, T0 = _probe(sc)
    prm = api.default_lin_params(RADIUS, 0)
    A = api.Context(0)
    try:
        A.set_option("count_searches", 1)
        A.keyframes_reset()
        A.keyframes_add(sc["store"])
        A.set_target(sc["map"], RADIUS)
        A.set_source(probe)
        A.linearize(T0[:3, :3], T0[:3, 3], prm)

        def snapshot():
            A.launch_stats(reset=True)
            lin = A.linearize(T0[:3, :3], T0[:3, 3], prm)
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"],
                    A.launch_stats()["points_searched"], _info(A), A.target_points().tobytes())

        before = snapshot()
        assert before[6] == 0                        # warm
        never = api.visibility_params(min_votes=13)  # twelve members cannot cast thirteen votes
        info = A.remove_dynamic(members, never)
        assert info["n_flagged"] == 0 and info["n_out"] == info["n_in"] == len(sc["map"]) and info["n_observed"] > 0
        assert snapshot() == before
        assert A.remove_dynamic([], p)["n_out"] == len(sc["map"]) and snapshot() == before
        # a map every point of which two members look through: refused, and nothing has changed
        wall = np.ascontiguousarray(shell(4000, 3, r_lo=60.0, r_hi=70.0))
        first = A.keyframes_add([wall])
        A.set_target(shell(3000, 4, r_lo=5.0, r_hi=20.0), RADIUS)
        A.set_source(probe)
        coarse = api.visibility_params(rows=8, cols=16, elev_min=-0.6, elev_max=0.6)
        both = [(first, I), (first, I)]
        assert vr.filter_ref(A.target_points(), sc["store"] + [wall], both, coarse)[4]["n_out"] == 0
        A.linearize(T0[:3, :3], T0[:3, 3], prm)
        before = snapshot()
        with pytest.raises(api.DcregError, match="every point"):
            A.remove_dynamic(both, coarse)
        assert snapshot() == before and A.index_check() == ZERO
    finally:
        A.close()


# ---- 6. isolation
def test_the_calls_leave_source_places_keyframes_and_window_index_alone(mover):
    c, sc, members, p, ref = mover
    probe, T0 = _probe(sc, reach=10.0)
    prm = api.default_lin_params(RADIUS, 0)
    A = api.Context(0)
    n = len(sc["map"])
    dev, out = DevCloud(sc["map"]), DevCloud(np.zeros((n, 3), np.float32))
    try:
        for k, v in WINDOW_OPTS + [("count_searches", 1)]:
            A.set_option(k, v)
        A.keyframes_reset()
        A.keyframes_add(sc["store"])
        A.set_target(sc["map"], RADIUS)
        A.set_source(probe)
        A.places_reset(api.place_params())
        A.places_add_clouds(sc["store"][:3])
        A.linearize(T0[:3, :3], T0[:3, 3], prm)

        def snapshot():
            A.launch_stats(reset=True)
            lin = A.linearize(T0[:3, :3], T0[:3, 3], prm)
            roi = A.roi_info()
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"],
                    A.launch_stats()["points_searched"], roi["active"], roi["windows_built"], _info(A), A.places_count(),
                    A.places_get(0, 3).tobytes(), A.keyframes_count(), [A.keyframes_get(i).tobytes() for i in (0, 11)])

        before = snapshot()
        assert before[6] == 0 and before[7]          # warm, the window active
        steps = [lambda: A.keyframe_range_images([0, 5, 11], p), lambda: A.visibility_filter(sc["map"], members, p),
                 lambda: A.visibility_filter_device(dev.ptr, n, 3, members, out.ptr, n, p),
                 lambda: A.keyframe_range_images(list(range(12)), api.visibility_params(rows=256, cols=4096)),
                 lambda: A.remove_dynamic(members, api.visibility_params(min_votes=13))]
        for k, step in enumerate(steps):
            step()
            assert snapshot() == before, k
    finally:
        A.close()
        dev.free()
        out.free()


# ---- 7. refusals at the C-ABI
def test_refusals_at_the_c_abi(five):
    _, store, poses5, q = five
    L = api.load()
    prm = api.default_lin_params(RADIUS, 0)
    c = api.Context(0)
    try:
        c.set_target(q, RADIUS)
        c.set_source(store[0])
        good = api.visibility_params(**SMALL)
        ids = np.array([0, 1], np.int64)
        poses = np.concatenate([p12(poses5[0]), p12(poses5[1])])
        xyz = np.ascontiguousarray(q[:100])
        img = np.full((2, 16, 64), 7.0, np.float32)
        out = np.full((100, 3), 7.0, np.float32)
        mask, through, observed = np.full(100, 7, np.uint8), np.full(100, 7, np.int32), np.full(100, 7, np.int32)
        n_out, info = C.c_int64(-5), api.VisibilityInfo()
        info.n_in = -5

        def images(n=2, i=ids, p=good, o=img.ctypes.data):
            return L.dcreg_keyframes_range_images(c._h, n, i.ctypes.data_as(I64P) if i is not None else None, C.byref(p) if p is not None else None, o)

        def filt(x=xyz.ctypes.data, n=100, stride=3, m=2, i=ids, ps=poses, p=good, o=out.ctypes.data, cap=100, no=C.byref(n_out)):
            return L.dcreg_visibility_filter(c._h, x, n, stride, m, i.ctypes.data_as(I64P) if i is not None else None,
                                             ps.ctypes.data_as(DP) if ps is not None else None, C.byref(p) if p is not None else None, o, cap, no,
                                             mask.ctypes.data, through.ctypes.data, observed.ctypes.data, C.byref(info))

        def remove(m=2, i=ids, ps=poses, p=good):
            return L.dcreg_target_remove_dynamic(c._h, m, i.ctypes.data_as(I64P) if i is not None else None,
                                                 ps.ctypes.data_as(DP) if ps is not None else None, C.byref(p) if p is not None else None, C.byref(info))

        every = [images, filt, remove]
        for k, call in enumerate(every):             # no store yet
            assert call() == -4, k
        c.keyframes_reset()
        c.keyframes_add(store[:2])

        def state():
            lin = c.linearize(poses5[0][:3, :3], poses5[0][:3, 3], prm)
            return (lin["n_eff"], tuple(lin["H_upper"]), _info(c), c.target_points().tobytes(), c.keyframes_count(),
                    [c.keyframes_get(i).tobytes() for i in range(2)])

        before = state()

        def arr(*v):
            return np.array(v, np.int64)

        def bad_pose(v):
            ps = poses.copy()
            ps[20] = v
            return ps

        def bad(**kw):
            p = api.visibility_params(**SMALL)
            for key, val in kw.items():
                setattr(p, key, val)
            return p

        bad_blocks = [bad(rows=0), bad(rows=257), bad(cols=0), bad(cols=4097), bad(elev_min=0.5), bad(elev_min=-1.6), bad(elev_max=1.6),
                      bad(elev_max=np.nan), bad(min_range=-1.0), bad(min_range=80.0), bad(max_range=np.inf), bad(margin_abs=-0.1),
                      bad(margin_rel=np.nan), bad(window=-1), bad(window=4), bad(min_votes=0), bad(min_ratio=-0.5), bad(min_ratio=1.5),
                      bad(min_ratio=np.nan)]
        calls = [lambda: images(n=-1), lambda: images(i=None), lambda: images(p=None), lambda: images(o=None), lambda: images(i=arr(0, 2)),
                 lambda: images(i=arr(-1, 0)),
                 lambda: filt(x=None), lambda: filt(n=-1), lambda: filt(stride=2), lambda: filt(m=-1), lambda: filt(i=None), lambda: filt(ps=None),
                 lambda: filt(p=None), lambda: filt(o=None), lambda: filt(cap=-1), lambda: filt(no=None), lambda: filt(i=arr(0, 2)),
                 lambda: filt(i=arr(-1, 1)), lambda: filt(ps=bad_pose(np.nan)), lambda: filt(ps=bad_pose(np.inf)), lambda: filt(n=2 ** 31),
                 lambda: remove(m=-1), lambda: remove(i=None), lambda: remove(ps=None), lambda: remove(p=None), lambda: remove(i=arr(2, 0)),
                 lambda: remove(ps=bad_pose(-np.inf))]
        calls += [lambda b=b: images(p=b) for b in bad_blocks] + [lambda b=b: filt(p=b) for b in bad_blocks] + [lambda b=b: remove(p=b) for b in bad_blocks]
        for k, call in enumerate(calls):
            assert call() == -1, k
            assert c._L.dcreg_last_error(c._h)
        assert np.all(img == 7.0) and np.all(out == 7.0) and np.all(mask == 7) and np.all(through == 7) and np.all(observed == 7)
        assert n_out.value == -5 and info.n_in == -5
        assert state() == before
        # the capacity protocol fills the sizes of a refused call
        ref = vr.filter_ref(xyz, store, [(0, poses5[0]), (1, poses5[1])], good)
        assert 0 < ref[4]["n_out"]
        assert filt(cap=ref[4]["n_out"] - 1) == -1 and n_out.value == ref[4]["n_out"] and api._visibility_info_dict(info) == ref[4]
        assert np.all(out == 7.0) and np.all(mask == 7) and np.all(through == 7)
        # a linearisation in flight
        c.linearize_begin(poses5[0][:3, :3], poses5[0][:3, 3], prm, slot=0)
        for k, call in enumerate(every):
            assert call() == -4, k
        c.linearize_end(slot=0)
        assert state() == before
        assert images() == 0 and filt() == 0 and n_out.value == ref[4]["n_out"]
        # the map form without a target
        e = api.Context(0)
        try:
            e.keyframes_reset()
            e.keyframes_add(store[:2])
            assert L.dcreg_target_remove_dynamic(e._h, 2, ids.ctypes.data_as(I64P), poses.ctypes.data_as(DP), C.byref(good), None) == -4
        finally:
            e.close()
    finally:
        c.close()
