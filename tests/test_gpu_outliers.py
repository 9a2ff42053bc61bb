"""Outlier removal on the device (dcreg_outlier_filter*, dcreg_set_*_outliers*, dcreg_target_remove_outliers) against the numpy reference of
tests/outliers_ref.py, which applies include/dcreg.h's rules literally: mask, scores, kept points, counts, and mean, stddev and threshold as
doubles must be BITWISE the reference's.  The contracts of the set / in-place forms are checked against the plain calls on the filtered
cloud.  The reference is the yardstick, never a second device run."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
import outliers_ref as orf
from dcreg_amd import api
from oracle import pyoracle as po
from test_gpu_device_seam import D2H, DevCloud, _info, _lin_equal, hip, strided
from test_gpu_map_update import RADIUS, assert_same_as_fresh, crop_ref, transform
from test_gpu_map_update import park            # noqa: F401  (fixture)
from test_gpu_configs import cfg_pair
from test_gpu_round6 import _window_pair
from test_outliers_reference import planted_scene

pytestmark = pytest.mark.gpu

MODES = {0: "statistical", 1: "radius"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_scores(a, b):
    """bitwise, any NaN equal to any NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def same_double(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def ref_of(cloud, p, neighbours=None):
    return orf.outlier_reference(cloud, MODES[p.mode], k=p.k, std_mul=p.std_mul, search_radius=p.search_radius, radius=p.radius,
                                 min_neighbors=p.min_neighbors, neighbours=neighbours)


def assert_bitwise(got, ref, what=""):
    kept, mask, scores, info = got
    assert np.array_equal(mask, ref["mask"]), what
    assert same_scores(scores, ref["scores"]), what
    assert kept.shape == ref["kept"].shape and np.array_equal(bits(kept), bits(ref["kept"])), what
    for key in ("n_in", "n_finite", "n_sparse", "n_out"):
        assert info[key] == ref[key], (what, key, info[key], ref[key])
    for key in ("mean", "stddev", "threshold"):
        assert same_double(info[key], ref[key]), (what, key, info[key], ref[key])


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def uniform(n, seed=0):
    return (np.random.default_rng(1000 + seed + n).uniform(-2, 2, (n, 3)) * [1.0, 1.0, 0.3]).astype(np.float32)


def lattice(m=9, step=0.25):
    """m^3 points on a regular lattice whose spacing is exact in float: every distance tied, interior scores equal"""
    g = np.arange(m, dtype=np.float32) * np.float32(step)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def with_duplicates(n=600, copies=40, seed=4):
    pts = uniform(n, seed)
    at = np.random.default_rng(seed).choice(n, copies, replace=False)
    pts[at] = pts[at[0]]
    return pts, at


def organised_sweep():
    """an organised 16 x 256 sweep (rows without a return are NaN, a few single NaN / inf coordinates) in a strided record of 5 floats"""
    rng = np.random.default_rng(21)
    az = np.linspace(-np.pi, np.pi, 256, endpoint=False)
    el = np.deg2rad(np.linspace(-15, 15, 16))
    rng_m = 4.0 / np.maximum(np.abs(np.sin(el))[:, None], 0.15) + rng.normal(0, 0.02, (16, 256))
    pts = np.stack([rng_m * np.cos(el)[:, None] * np.cos(az), rng_m * np.cos(el)[:, None] * np.sin(az), rng_m * np.sin(el)[:, None] * np.ones(256)], -1)
    pts = pts.astype(np.float32)
    pts[[3, 11]] = np.nan
    pts[5, 17, 1] = np.inf
    pts[9, 200, 2] = np.nan
    return strided(pts.reshape(-1, 3), 5)


@pytest.fixture(scope="module")
def window():
    """a map wide enough for a window index (a 180 m square, the frame 60 m across), its frame, the pose and a start pose"""
    tgt, src, gt, T0 = _window_pair(n_map=600_000, extent=90.0)
    return tgt, src, gt, T0, cfg_pair(RADIUS, 30, 0, 1e-5, 1e-3, gt.reshape(16))[0], [("max_table_entries", 1 << 16), ("roi_index", 2)]


@pytest.fixture(scope="module")
def scene():
    return planted_scene()


CLOUDS = {"uniform": lambda: uniform(1000), "lattice": lattice, "duplicates": lambda: with_duplicates()[0], "sweep": organised_sweep,
          "planted": lambda: planted_scene()[0]}


# ---- 1. bitwise against the reference: sizes, k, clouds
@pytest.mark.parametrize("n", [1, 2, 8, 9, 10, 63, 64, 65, 255, 256, 257, 4097])
def test_statistical_sizes_across_wave_block_and_tree_boundaries(ctx, n):
    cloud = uniform(n)
    p = api.outlier_params(k=8, std_mul=1.0)
    assert_bitwise(ctx.outlier_filter(cloud, p), ref_of(cloud, p), n)


@pytest.mark.parametrize("k", [1, 5, 8, 9, 16, 17, 32])
def test_statistical_every_heap_size(ctx, k):
    cloud = uniform(1000)
    p = api.outlier_params(k=k, std_mul=1.5)
    ref = ref_of(cloud, p)
    assert 0 < ref["n_out"] < 1000
    assert_bitwise(ctx.outlier_filter(cloud, p), ref, k)
    p = api.outlier_params(k=k, std_mul=1.5, search_radius=0.45)
    ref = ref_of(cloud, p)
    assert ref["n_sparse"] > 0 or k < 5
    assert_bitwise(ctx.outlier_filter(cloud, p), ref, (k, "bounded"))


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_statistical_clouds(ctx, name):
    cloud = CLOUDS[name]()
    for k, std_mul in ((8, 1.0), (32, 0.0)):
        p = api.outlier_params(k=k, std_mul=std_mul)
        ref = ref_of(cloud, p)
        assert 0 < ref["n_out"] < len(cloud)
        assert_bitwise(ctx.outlier_filter(cloud, p), ref, (name, k))


def test_a_lattice_ties_every_distance(ctx):
    cloud = lattice()
    p = api.outlier_params(k=6, std_mul=0.0)
    ref = ref_of(cloud, p)
    inner = np.all((cloud > 0) & (cloud < 2.0), axis=1)
    assert np.all(ref["scores"][inner] == np.float32(0.25)) and ref["n_out"] >= inner.sum()
    assert_bitwise(ctx.outlier_filter(cloud, p), ref)


@pytest.mark.parametrize("k", [8, 32])
def test_more_duplicates_than_k_exclude_a_point_by_its_index(ctx, k):
    cloud, at = with_duplicates()
    p = api.outlier_params(k=k, std_mul=1.0)
    ref = ref_of(cloud, p)
    assert np.all(ref["scores"][at] == 0.0)
    assert_bitwise(ctx.outlier_filter(cloud, p), ref)


def test_the_planted_scene(ctx, scene):
    cloud, planted = scene
    p = api.outlier_params(k=8, std_mul=2.0)
    got = ctx.outlier_filter(cloud, p)
    assert np.array_equal(~got[1], planted)
    assert_bitwise(got, ref_of(cloud, p))
    # bounded: the planted points come out sparse, the statistics run over the plane alone
    p = api.outlier_params(k=8, std_mul=2.0, search_radius=1.0)
    got = ctx.outlier_filter(cloud, p)
    assert got[3]["n_sparse"] == 20 and np.array_equal(np.isnan(got[2]), planted)
    assert_bitwise(got, ref_of(cloud, p))


@pytest.mark.parametrize("name", sorted(CLOUDS))
@pytest.mark.parametrize("m", [1, 3, 8])
def test_radius_mode(ctx, name, m):
    cloud = CLOUDS[name]()
    radius = {"uniform": 0.3, "lattice": 0.25, "duplicates": 0.35, "sweep": 1.5, "planted": 0.5}[name]     # lattice: exactly its spacing
    p = api.outlier_params("radius", radius=radius, min_neighbors=m)
    ref = ref_of(cloud, p)
    if name == "lattice":
        assert ref["n_out"] == 0                     # the comparison is strict: a neighbour AT the radius does not count
        p2 = api.outlier_params("radius", radius=float(np.nextafter(np.float32(0.25), np.float32(1))), min_neighbors=m)
        ref2 = ref_of(cloud, p2)
        assert ref2["n_out"] == {1: 729, 3: 729, 8: 0}[m]      # (a lattice point has 3 to 6 neighbours at the spacing)
        assert_bitwise(ctx.outlier_filter(cloud, p2), ref2, (name, m, "above"))
    else:
        assert 0 < ref["n_out"] < len(cloud)
    assert_bitwise(ctx.outlier_filter(cloud, p), ref, (name, m))


def test_at_size_against_the_oracle_tree(ctx):
    rng = np.random.default_rng(77)
    n = 200_000
    cloud = np.column_stack([rng.uniform(0, 60, n), rng.uniform(0, 60, n), rng.normal(0, 0.05, n) + (rng.uniform(0, 1, n) < 0.002) * rng.uniform(1, 6, n)])
    cloud = cloud.astype(np.float32)
    p = api.outlier_params(k=16, std_mul=2.0)
    ref = ref_of(cloud, p, neighbours=lambda q, kk: po.KdTree(q).knn(q, kk))
    assert 0 < n - ref["n_out"] < n // 20
    assert_bitwise(ctx.outlier_filter(cloud, p), ref)


@pytest.mark.parametrize("mode", ["statistical", "radius"])
def test_a_cloud_without_a_finite_point(ctx, mode):
    """65 points, every one NaN or inf in some coordinate: nothing is used, nothing is searched"""
    cloud = np.full((65, 3), np.nan, np.float32)
    cloud[1::3] = [1.0, np.inf, 2.0]
    cloud[2::3] = [0.5, 0.25, -np.inf]
    p = api.outlier_params(k=8, std_mul=1.0) if mode == "statistical" else api.outlier_params("radius", radius=0.5, min_neighbors=1)
    got = ctx.outlier_filter(cloud, p)
    kept, mask, scores, info = got
    assert np.all(np.isnan(scores)) and not mask.any() and len(kept) == 0 and info["n_out"] == 0 and info["n_finite"] == 0
    assert_bitwise(got, ref_of(cloud, p), mode)


def test_fewer_points_than_k_bounded_and_unbounded(ctx):
    """5 finite points, k = 8.  Bounded, the index is built and searched although no point can have k neighbours; unbounded, neither
    happens and every point is kept"""
    cloud = uniform(5)
    bounded, unbounded = api.outlier_params(k=8, std_mul=1.0, search_radius=10.0), api.outlier_params(k=8, std_mul=1.0)
    ref_b, ref_u = ref_of(cloud, bounded), ref_of(cloud, unbounded)
    assert ref_b["n_finite"] == ref_u["n_finite"] == 5 and ref_u["n_out"] == 5 and ref_u["mask"].all()
    got_b, got_u = ctx.outlier_filter(cloud, bounded), ctx.outlier_filter(cloud, unbounded)
    assert_bitwise(got_b, ref_b, "bounded")
    assert_bitwise(got_u, ref_u, "unbounded")
    assert got_u[3]["n_out"] == 5 and got_u[1].all() and np.array_equal(bits(got_u[0]), bits(cloud))


# ---- 2. determinism, device form, capacity
def test_repeated_calls_and_other_contexts_give_the_same_bits(ctx, park):        # noqa: F811
    cloud = CLOUDS["planted"]()
    p = api.outlier_params(k=8, std_mul=1.0)
    a = ctx.outlier_filter(cloud, p)
    b = ctx.outlier_filter(cloud, p)
    big = api.Context(0)
    try:
        big.set_option("cell", 0.9)
        big.set_target(park[0], RADIUS)
        big.set_source(park[1])
        c = big.outlier_filter(cloud, p)
    finally:
        big.close()
    for other in (b, c):
        assert np.array_equal(a[1], other[1]) and same_scores(a[2], other[2]) and np.array_equal(bits(a[0]), bits(other[0]))
        assert all(same_double(a[3][key], other[3][key]) for key in ("mean", "stddev", "threshold")) and a[3]["n_out"] == other[3]["n_out"]


def test_the_device_form_and_the_capacity_protocol(ctx):
    cloud = organised_sweep()
    n = len(cloud)
    p = api.outlier_params(k=8, std_mul=1.0)
    ref = ref_of(cloud, p)
    dev, out = DevCloud(cloud), DevCloud(np.full((n, 3), 7.0, np.float32))
    mask, scores = DevCloud(np.zeros((n, 1), np.float32)), DevCloud(np.zeros((n, 1), np.float32))
    try:
        n_out, info = ctx.outlier_filter_device(dev.ptr, n, 5, out.ptr, n, p, mask.ptr, scores.ptr)
        assert n_out == ref["n_out"] and info["n_finite"] == ref["n_finite"]
        kept, m, s = np.zeros((n, 3), np.float32), np.zeros(4 * n, np.uint8), np.zeros(n, np.float32)
        for host, d, nb in ((kept, out, kept.nbytes), (m, mask, n), (s, scores, 4 * n)):
            assert hip().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(d.ptr), nb, D2H) == 0
        assert np.array_equal(bits(kept[:n_out]), bits(ref["kept"])) and np.all(kept[n_out:] == 7.0)
        assert np.array_equal(m[:n].astype(bool), ref["mask"]) and same_scores(s, ref["scores"])
        # a capacity that is too small: the size needed, nothing written
        out.write(np.full((n, 3), 7.0, np.float32))
        L, n_need, oi = api.load(), C.c_int64(0), api.OutlierInfo()
        rc = L.dcreg_outlier_filter_device(ctx._h, C.c_void_p(dev.ptr), n, 5, C.byref(p), C.c_void_p(out.ptr), ref["n_out"] - 1, C.byref(n_need), None,
                                           None, C.byref(oi))
        assert rc == -1 and n_need.value == ref["n_out"] == oi.n_out
        assert hip().hipMemcpy(C.c_void_p(kept.ctypes.data), C.c_void_p(out.ptr), kept.nbytes, D2H) == 0
        assert np.all(kept == 7.0)
    finally:
        for d in (dev, out, mask, scores):
            d.free()
    kept, m, s, info = ctx.outlier_filter(cloud, p, want_mask=False, want_scores=False)
    assert m is None and s is None and np.array_equal(bits(kept), bits(ref["kept"]))


# ---- 3. the set forms: the context is left as the plain calls on the filtered cloud leave it
@pytest.mark.parametrize("leaf", [None, 0.4])
@pytest.mark.parametrize("mode", ["statistical", "radius"])
def test_set_source_and_set_target_outliers(park, leaf, mode):        # noqa: F811
    tgt, src, gt = park[0][:120_000], park[1], park[2]
    p = api.outlier_params(mode, k=8, std_mul=1.0, radius=0.8 if leaf else 0.3, min_neighbors=4)
    prm = api.default_lin_params(RADIUS, 0)
    q = transform(src[:3000], gt)
    A, B = api.Context(0), api.Context(0)
    dev_t, dev_s = DevCloud(strided(tgt, 4)), DevCloud(strided(src, 4))
    try:
        ft, fs = (B.voxel_downsample([c], leaf)[0][0] if leaf else c for c in (tgt, src))
        ft, fs = B.outlier_filter(ft, p)[0], B.outlier_filter(fs, p)[0]
        assert 0 < len(ft) < len(tgt) and 0 < len(fs) < len(src)
        B.set_target(ft, RADIUS)
        B.set_source(fs)
        want = (B.linearize(gt[:3, :3], gt[:3, 3], prm), B.knn(q, 5, 1.0), _info(B))
        for device in (False, True):
            if device:
                it, _ = A.set_target_outliers_device(dev_t.ptr, len(tgt), 4, RADIUS, p, leaf)
                iS, vs = A.set_source_outliers_device(dev_s.ptr, len(src), 4, p, leaf)
            else:
                it, _ = A.set_target_outliers(tgt, RADIUS, p, leaf)
                iS, vs = A.set_source_outliers(src, p, leaf)
            assert it["n_out"] == len(ft) and iS["n_out"] == len(fs) and (vs is None) == (leaf is None)
            got = (A.linearize(gt[:3, :3], gt[:3, 3], prm), A.knn(q, 5, 1.0), _info(A))
            _lin_equal(got[0], want[0])
            assert np.array_equal(got[1][0], want[1][0]) and np.array_equal(bits(got[1][1]), bits(want[1][1])) and got[2] == want[2]
            assert np.array_equal(bits(A.target_points()), bits(ft))
    finally:
        for x in (A, B):
            x.close()
        dev_t.free()
        dev_s.free()


# ---- 4. the resident map cleaned in place
def test_remove_outliers_after_inserts_and_a_crop(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    base = tgt[:100_000]
    rng = np.random.default_rng(12)
    dust = (base[rng.choice(len(base), 300, replace=False)] + rng.uniform(1.5, 4.0, (300, 1)) * [0, 0, 1]).astype(np.float32)
    A = api.Context(0)
    try:
        A.set_target(np.concatenate([base, dust]), RADIUS)
        A.insert(frames[2], T[2])
        A.insert(frames[3], T[3], min_spacing=0.1)
        cloud = A.target_points()
        lo, hi = cloud.min(0).astype(np.float64) + [3.0, 3.0, -1.0], cloud.max(0).astype(np.float64) + 1.0
        A.crop(lo, hi)
        cloud = crop_ref(cloud, lo, hi)
        assert np.array_equal(bits(A.target_points()), bits(cloud))
        for p in (api.outlier_params(k=8, std_mul=2.0, search_radius=1.0), api.outlier_params("radius", radius=0.4, min_neighbors=3)):
            ref = ref_of(cloud, p, neighbours=lambda q, kk: po.KdTree(q).knn(q, kk)) if p.mode == 0 else None
            A.set_source(src)
            A.linearize(T0[3][:3, :3], T0[3][:3, 3], api.default_lin_params(RADIUS, 0))
            info = A.remove_outliers(p)
            if ref is None:                          # (the brute-force reference is for small clouds: the filter call, checked above, stands in)
                B = api.Context(0)
                try:
                    kept, _, _, binfo = B.outlier_filter(cloud, p)
                finally:
                    B.close()
                ref = dict(kept=kept, n_out=binfo["n_out"], n_sparse=0, mean=np.nan, stddev=np.nan, threshold=np.nan)
            assert info["n_in"] == info["n_finite"] == len(cloud) and 0 < info["n_out"] == ref["n_out"] < len(cloud)
            assert info["n_sparse"] == ref["n_sparse"] and all(same_double(info[key], ref[key]) for key in ("mean", "stddev", "threshold"))
            cloud = ref["kept"]
            assert_same_as_fresh(A, cloud, src, T0[3], cfg, frames=frames[:2])
    finally:
        A.close()


def test_a_clean_that_removes_nothing_changes_nothing(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    A = api.Context(0)
    try:
        A.set_option("count_searches", 1)
        A.set_target(tgt[:100_000], RADIUS)
        A.set_source(src)
        prm = api.default_lin_params(RADIUS, 0)
        ref = A.linearize(T0[3][:3, :3], T0[3][:3, 3], prm)
        before = (_info(A), A.target_points())
        A.launch_stats(reset=True)
        info = A.remove_outliers(api.outlier_params(k=8, std_mul=1e9))
        assert info["n_out"] == info["n_in"] == 100_000
        info = A.remove_outliers(api.outlier_params("radius", radius=50.0, min_neighbors=1))
        assert info["n_out"] == 100_000
        again = A.linearize(T0[3][:3, :3], T0[3][:3, 3], prm)
        assert A.launch_stats()["points_searched"] == 0          # the neighbour state of the first launch still serves
        assert np.array_equal(again["H_upper"], ref["H_upper"]) and np.array_equal(again["g"], ref["g"])
        assert _info(A) == before[0] and np.array_equal(bits(A.target_points()), bits(before[1]))
        # a clean that would remove every point is refused and changes nothing
        with pytest.raises(api.DcregError, match="every point"):
            A.remove_outliers(api.outlier_params("radius", radius=1e-4, min_neighbors=30))
        again = A.linearize(T0[3][:3, :3], T0[3][:3, 3], prm)
        assert A.launch_stats()["points_searched"] == 0 and np.array_equal(again["H_upper"], ref["H_upper"])
    finally:
        A.close()


def test_a_capped_map_is_cleaned_through_the_whole_maps_index(window):
    base, src, gt, T0, cfg, opts = window
    p = api.outlier_params("radius", radius=0.3, min_neighbors=3)
    A, B = api.Context(0), api.Context(0)
    try:
        for k, v in opts:
            A.set_option(k, v)
        A.set_target(base, RADIUS)
        A.set_source(src)
        A.icp_run(T0, "Ours", cfg)
        assert A.roi_info()["active"]
        kept = B.outlier_filter(base, p)[0]
        info = A.remove_outliers(p)
        assert 0 < info["n_out"] == len(kept) < len(base) and not A.roi_info()["active"]
        assert_same_as_fresh(A, kept, src, T0, cfg, options=opts)
    finally:
        A.close()
        B.close()


# ---- 5. the filter calls leave the rest of the context alone
def test_the_filter_calls_leave_the_rest_of_the_context_alone(window, park):        # noqa: F811
    tgt, src, gt, T0, cfg, opts = window
    frames = park[5]
    prm = api.default_lin_params(RADIUS, 0)
    pp = api.place_params()
    c = api.Context(0)
    cloud = organised_sweep()
    dev, out = DevCloud(cloud), DevCloud(np.zeros((len(cloud), 3), np.float32))
    try:
        for k, v in opts + [("count_searches", 1)]:
            c.set_option(k, v)
        c.set_target(tgt, RADIUS)
        c.set_source(src)
        c.places_reset(pp)
        c.places_add_clouds(frames[:3])
        c.linearize(T0[:3, :3], T0[:3, 3], prm)
        assert c.roi_info()["active"]

        def snapshot():
            c.launch_stats(reset=True)
            lin = c.linearize(T0[:3, :3], T0[:3, 3], prm)
            roi = c.roi_info()
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"],
                    c.launch_stats()["points_searched"], roi["active"], roi["windows_built"], _info(c), c.places_count(),
                    c.places_get(0, 3).tobytes())

        before = snapshot()
        assert before[6] == 0                        # warm
        steps = [lambda: c.outlier_filter(cloud, api.outlier_params(k=8)), lambda: c.outlier_filter(tgt[:50_000], api.outlier_params(k=16, search_radius=1.0)),
                 lambda: c.outlier_filter(cloud, api.outlier_params("radius", radius=0.5, min_neighbors=2)),
                 lambda: c.outlier_filter_device(dev.ptr, len(cloud), 5, out.ptr, len(cloud), api.outlier_params(k=4))]
        for k, step in enumerate(steps):
            step()
            assert snapshot() == before, k
    finally:
        c.close()
        dev.free()
        out.free()


# ---- 6. refusals at the C-ABI
def test_refusals_at_the_c_abi(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    L = api.load()
    cloud = np.ascontiguousarray(CLOUDS["planted"]())
    n = len(cloud)
    out, mask, scores = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
    n_out, info, vinfo = C.c_int64(-5), api.OutlierInfo(), api.VoxelInfo()
    prm = api.default_lin_params(RADIUS, 0)
    c = api.Context(0)
    try:
        c.set_target(tgt[:60_000], RADIUS)
        c.set_source(src)

        def state():
            lin = c.linearize(T0[3][:3, :3], T0[3][:3, 3], prm)
            return (lin["n_eff"], tuple(lin["H_upper"]), _info(c), c.target_points().tobytes())

        before = state()
        good = api.outlier_params()

        def bad(**kw):
            p = api.outlier_params("radius" if set(kw) & {"radius", "min_neighbors"} else "statistical")
            for key, v in kw.items():
                setattr(p, key, v)
            return p

        blocks = [bad(k=0), bad(k=33), bad(std_mul=np.nan), bad(search_radius=-1.0), bad(search_radius=np.inf), bad(radius=0.0), bad(radius=np.nan),
                  bad(min_neighbors=0), bad(mode=7)]
        ptr = cloud.ctypes.data

        def filt(p, xyz=ptr, m=n, stride=3, o=out.ctypes.data, cap=n, no=C.byref(n_out)):
            return L.dcreg_outlier_filter(c._h, xyz, m, stride, p, o, cap, no, mask.ctypes.data, scores.ctypes.data, C.byref(info))

        calls = [lambda p=p: filt(C.byref(p)) for p in blocks]
        calls += [lambda p=p: L.dcreg_set_source_outliers(c._h, ptr, n, 3, None, C.byref(p), None, None) for p in blocks]
        calls += [lambda p=p: L.dcreg_set_target_outliers(c._h, ptr, n, 3, None, C.byref(p), 1.0, None, None) for p in blocks]
        calls += [lambda p=p: L.dcreg_target_remove_outliers(c._h, C.byref(p), None) for p in blocks]
        g = C.byref(good)
        calls += [lambda: filt(None), lambda: filt(g, stride=2), lambda: filt(g, m=-1), lambda: filt(g, xyz=None), lambda: filt(g, no=None),
                  lambda: filt(g, cap=-1), lambda: filt(g, o=None), lambda: filt(g, m=2 ** 31),
                  lambda: L.dcreg_set_source_outliers(c._h, ptr, 0, 3, None, g, None, None),
                  lambda: L.dcreg_set_source_outliers(c._h, None, n, 3, None, g, None, None),
                  lambda: L.dcreg_set_target_outliers(c._h, ptr, n, 2, None, g, 1.0, None, None),
                  lambda: L.dcreg_set_source_outliers(c._h, ptr, n, 3, C.byref(api.VoxelParams()), g, C.byref(vinfo), None),
                  lambda: L.dcreg_target_remove_outliers(c._h, None, None)]
        for k, call in enumerate(calls):
            assert call() == -1, k
            assert c._L.dcreg_last_error(c._h)
        assert not out.any() and not mask.any() and not scores.any() and n_out.value == -5
        # a source that the filter empties is refused too
        assert L.dcreg_set_source_outliers(c._h, ptr, n, 3, None, C.byref(api.outlier_params("radius", radius=1e-5, min_neighbors=9)), None, None) == -1
        assert state() == before
        # a linearisation in flight: DCREG_E_STATE
        c.linearize_gated_begin(prm)
        for call in (lambda: filt(g), lambda: L.dcreg_set_source_outliers(c._h, ptr, n, 3, None, g, None, None),
                     lambda: L.dcreg_set_target_outliers(c._h, ptr, n, 3, None, g, 1.0, None, None), lambda: L.dcreg_target_remove_outliers(c._h, g, None)):
            assert call() == -4
        c.gate_abort()
        assert state() == before
        assert filt(g) == 0 and n_out.value == 2000
        # no target for the in-place call
        e = api.Context(0)
        try:
            assert L.dcreg_target_remove_outliers(e._h, g, None) == -4
            assert L.dcreg_outlier_filter(e._h, ptr, 0, 3, g, None, 0, C.byref(n_out), None, None, C.byref(info)) == 0 and n_out.value == 0 and info.n_in == 0
        finally:
            e.close()
    finally:
        c.close()


# ---- 7. the third level of the summation tree
def mostly_nan(n, n_finite=3000):
    """n rows, all NaN except about n_finite seeded finite points; rows 0, 262 143, 262 144 (where present) and the last are finite"""
    rng = np.random.default_rng(3000 + n)
    cloud = np.full((n, 3), np.nan, np.float32)
    at = np.unique(np.concatenate([rng.choice(n, n_finite, replace=False), [0, 262143, min(262144, n - 1), n - 1]]))
    cloud[at] = (rng.uniform(-2, 2, (len(at), 3)) * [1.0, 1.0, 0.3]).astype(np.float32)
    return cloud, at


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
@pytest.mark.parametrize("n", [262144, 262145, 262657])
def test_statistical_past_the_second_level_of_the_summation_tree(ctx, n, bounded):
    """The tree sums run over the INPUT rows (a dropped row adds +0.0): a block reduces 512 values, a second level 512 blocks = 262 144
    rows, and one row more needs a third level.  At exactly two levels, one value past them, and one block past them, the means, the
    deviation and the threshold are bitwise the reference's T(a), and so is everything decided by them."""
    cloud, at = mostly_nan(n)
    p = api.outlier_params(k=8, std_mul=1.0, search_radius=0.3 if bounded else 0.0)
    ref = ref_of(cloud, p)
    assert ref["n_in"] == n and ref["n_finite"] == len(at) and 2900 < len(at) <= 3004
    assert 0 < ref["n_out"] < ref["n_finite"] and (ref["n_sparse"] > 0) == bounded
    assert_bitwise(ctx.outlier_filter(cloud, p), ref, (n, bounded))
