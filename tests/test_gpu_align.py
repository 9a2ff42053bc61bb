"""A pose from correspondences on the device (dcreg_align_correspondences*) against tests/align_ref.py, which applies include/dcreg.h's
rule literally: records, mask and counters must be the reference's bit for bit - every field, doubles as bit patterns - whatever the
number of used pairs, of hypotheses and of survivors, the scorer's LDS tile and its split of the pairs over blocks."""
import ctypes as C

import numpy as np
import pytest

import align_ref as ar
import align_scenes as sc
import helpers as h
from dcreg_amd import api
from test_fpfh_reference import lot_cloud, moved_copy
from test_gpu_device_seam import D2H, DevCloud, hip, strided
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

TILE = 256                       # used pairs per LDS tile of k_align_score (align.hip kScoreTile)
GRID = 4096 * 256                # hypotheses per stride of k_align_hypotheses' grid (align.hip kHypGrid * kHypBlock)
INT_FIELDS = ("hypothesis", "pairs", "count", "cost", "n_inliers", "refined")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def assert_same(got, ref, what=""):
    assert got["info"] == ref["info"], (what, got["info"], ref["info"])
    assert len(got["records"]) == len(ref["records"]) == ref["info"]["n_returned"], what
    for k, (g, r) in enumerate(zip(got["records"], ref["records"])):
        for f in INT_FIELDS:
            assert g[f] == r[f], (what, k, f, g[f], r[f])
        assert np.array_equal(bits(g["T"]), bits(r["T"])), (what, k, g["T"], r["T"])
        assert bits(g["rmse"]) == bits(r["rmse"]), (what, k, g["rmse"], r["rmse"])
    if got.get("mask") is not None:
        assert np.array_equal(got["mask"], ref["mask"]), what


def both(ctx, a, b, ca, cb, what="", **kw):
    got = ctx.align_correspondences(a, b, ca, cb, api.align_params(**kw))
    ref = ar.align(a, b, ca, cb, **kw)
    assert_same(got, ref, what)
    return got, ref


def pairs(m, share=0.5, seed=0):
    return sc.synthetic(m, share, 0.02, 100 + seed)[:4]


@pytest.mark.parametrize("m_u", [3, 4, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_used_pairs_around_the_tile_size(ctx, m_u):
    a, b, ca, cb = pairs(m_u, 1.0 if m_u < 5 else 0.5, m_u)
    for s in (0.0, 0.9):
        got, ref = both(ctx, a, b, ca, cb, m_u, n_hypotheses=300, seed=m_u, inlier_distance=0.3, edge_similarity=s, n_best=5, refine_iterations=1)
        assert ref["info"]["n_used"] == m_u and ref["info"]["n_scored"] > 0


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 256, 257])
def test_hypotheses_across_wave_and_block_boundaries(ctx, n_hyp):
    a, b, ca, cb = pairs(60, 0.5, 1)
    for seed in (0, 0xFFFFFFFFFFFFFFF1):
        got, ref = both(ctx, a, b, ca, cb, n_hyp, n_hypotheses=n_hyp, seed=seed, inlier_distance=0.3, edge_similarity=0.0, n_best=4, refine_iterations=2)
        i = ref["info"]
        assert i["n_drawn"] == n_hyp == i["n_degenerate"] + i["n_rejected"] + i["n_scored"] and i["n_rejected"] == 0


def test_hypotheses_past_one_stride_of_the_grid(ctx):
    a, b, ca, cb = pairs(60, 0.5, 2)
    got, ref = both(ctx, a, b, ca, cb, "grid", n_hypotheses=GRID + 1, seed=9, inlier_distance=0.3, edge_similarity=0.9, n_best=32, refine_iterations=0)
    assert ref["info"]["n_scored"] > 1000 and ref["info"]["n_rejected"] > GRID // 2
    # the last hypothesis is the only one of the grid's second stride: it must have been drawn and counted
    assert sum(ref["info"][k] for k in ("n_degenerate", "n_rejected", "n_scored")) == GRID + 1


@pytest.mark.parametrize("s", [0.0, 0.9])
@pytest.mark.parametrize("n_best", [1, 5, 32])
def test_pre_rejection_and_the_number_of_records(ctx, s, n_best):
    a, b, ca, cb = pairs(300, 0.3, 3)
    got, ref = both(ctx, a, b, ca, cb, (s, n_best), n_hypotheses=257, seed=4, inlier_distance=0.3, edge_similarity=s, n_best=n_best, refine_iterations=3)
    assert len(ref["records"]) == min(n_best, ref["info"]["n_scored"])
    if s == 0.0:
        assert ref["info"]["n_rejected"] == 0 and ref["info"]["n_scored"] >= 250
    else:
        assert 0 < ref["info"]["n_scored"] < 32 < ref["info"]["n_rejected"]       # (n_best = 32: more records asked for than scored)


@pytest.mark.parametrize("refine", [0, 1, 8])
def test_refinement_steps(ctx, refine):
    a, b, ca, cb = pairs(200, 0.4, 4)
    got, ref = both(ctx, a, b, ca, cb, refine, n_hypotheses=400, seed=6, inlier_distance=0.25, edge_similarity=0.9, n_best=8, refine_iterations=refine)
    assert any(r["refined"] == refine for r in ref["records"])
    # a d that leaves wrong hypotheses fewer than three inliers: their refinement stops at once
    got, ref = both(ctx, a, b, ca, cb, refine, n_hypotheses=64, seed=6, inlier_distance=1e-3, edge_similarity=0.0, n_best=32, refine_iterations=refine)
    assert all(r["refined"] == 0 for r in ref["records"])


def test_ties_come_in_ascending_h(ctx):
    g = sc.lattice(40)
    idx = np.arange(40, dtype=np.int32)
    got, ref = both(ctx, g, g, idx, idx, "ties", n_hypotheses=200, seed=8, inlier_distance=0.5, edge_similarity=0.0, n_best=32, refine_iterations=0)
    hs = [r["hypothesis"] for r in got["records"]]
    assert len(hs) == 32 and hs == sorted(hs) and all(r["count"] == 40 and r["cost"] == 0 for r in got["records"])
    assert ref["info"]["n_degenerate"] > 0 and got["mask"].all()


def test_unused_pairs_strides_and_reordered_inputs(ctx):
    a, b, ca, cb = [x.copy() for x in pairs(150, 0.5, 5)]
    a[7, 1], b[9, 2], b[11, 0] = np.nan, np.inf, -np.inf
    ca[3], cb[4], ca[5], cb[6] = -1, -1, 150, 2 ** 31 - 1
    ca[20:24], cb[20:24] = ca[30], cb[30]                      # repeated pairs
    kw = dict(n_hypotheses=300, seed=10, inlier_distance=0.3, edge_similarity=0.9, n_best=6, refine_iterations=2)
    got, ref = both(ctx, a, b, ca, cb, "unused", **kw)
    unused = ref["info"]["n_pairs"] - ref["info"]["n_used"]
    assert 4 <= unused <= 7 and ref["info"]["n_scored"] > 0 and not got["mask"][[3, 4, 5, 6]].any()
    # strided clouds: the further columns are not read
    wa, wb = strided(a, 5), strided(b, 7)
    assert_same(ctx.align_correspondences(wa, wb, ca, cb, api.align_params(**kw)), ref, "strided")
    # the clouds reordered, the same pairs in the same order: the same records
    pa, pb = np.random.default_rng(1).permutation(150), np.random.default_rng(2).permutation(150)
    inv_a, inv_b = np.argsort(pa).astype(np.int32), np.argsort(pb).astype(np.int32)
    ok_a, ok_b = (ca >= 0) & (ca < 150), (cb >= 0) & (cb < 150)
    ca2, cb2 = np.where(ok_a, inv_a[np.clip(ca, 0, 149)], ca), np.where(ok_b, inv_b[np.clip(cb, 0, 149)], cb)
    assert_same(ctx.align_correspondences(a[pa], b[pb], ca2, cb2, api.align_params(**kw)), ref, "reordered")
    # fewer than three used pairs, and none at all
    got, ref = both(ctx, a, b, np.array([7, 1, -1, 2], np.int32), np.array([0, 1, 2, 9], np.int32), "two", **kw)
    assert ref["info"]["n_used"] == 1 and got["records"] == [] and not got["mask"].any()
    got, ref = both(ctx, a, b, np.zeros(0, np.int32), np.zeros(0, np.int32), "none", **kw)
    assert got["info"]["n_pairs"] == 0 and got["records"] == []
    empty = np.zeros((0, 3), np.float32)
    both(ctx, empty, b, ca, cb, "no points", **kw)


def test_degenerate_pairs_return_nothing(ctx):
    line = np.outer(np.arange(20, dtype=np.float32), np.array([1.0, 2.0, -1.0], np.float32))
    same = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (20, 1))
    idx = np.arange(20, dtype=np.int32)
    for cloud in (line, same):
        got, ref = both(ctx, cloud, cloud, idx, idx, "degenerate", n_hypotheses=200, inlier_distance=0.5, edge_similarity=0.9, n_best=4)
        assert got["info"]["n_degenerate"] == 200 and got["records"] == [] and not got["mask"].any()


def test_the_device_form_repeated_calls_and_a_second_context(ctx):
    a, b, ca, cb = pairs(400, 0.3, 6)
    wa, wb = strided(a, 4), strided(b, 6)
    p = api.align_params(n_hypotheses=1000, seed=12, inlier_distance=0.2, edge_similarity=0.9, n_best=7, refine_iterations=3)
    first = ctx.align_correspondences(wa, wb, ca, cb, p)
    assert first["info"]["n_returned"] == 7
    assert_same(ctx.align_correspondences(wa, wb, ca, cb, p), first, "again")
    devs = [DevCloud(wa), DevCloud(wb), DevCloud(ca.view(np.float32).reshape(-1, 1)), DevCloud(cb.view(np.float32).reshape(-1, 1)),
            DevCloud(np.ones((100, 1), np.float32))]
    other = api.Context(0)
    try:
        got = ctx.align_correspondences_device(devs[0].ptr, 400, 4, devs[1].ptr, 400, 6, devs[2].ptr, devs[3].ptr, 400, p, devs[4].ptr)
        mask = np.zeros(400, np.uint8)
        assert hip().hipMemcpy(C.c_void_p(mask.ctypes.data), C.c_void_p(devs[4].ptr), 400, D2H) == 0
        got["mask"] = mask
        assert_same(got, first, "device form")
        other.set_option("align_score_split", 100)
        tgt, src = h.scene_parkinglot(n_map=4000, n_frame=1500, extent=12.0, frame_range=5.0)
        other.set_target(tgt, 0.5)
        other.set_source(src)
        T0 = h.pose6d_matrix(**h.PK01_INIT)
        prm = api.default_lin_params(0.5, 0)

        def sums():
            lin = other.linearize(T0[:3, :3], T0[:3, 3], prm)
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"])

        before = sums()
        assert before[0] > 0
        assert_same(other.align_correspondences(wa, wb, ca, cb, p), first, "second context")
        assert sums() == before
        # a linearisation in flight: DCREG_E_STATE from both forms, nothing written
        other.linearize_begin(T0[:3, :3], T0[:3, 3], prm, slot=0)
        recs, info = (api.AlignRecord * 7)(), api.AlignInfo()
        args = (400, 4, devs[1].ptr, 400, 6, devs[2].ptr, devs[3].ptr, 400, C.byref(p), recs, None, C.byref(info))
        assert api.load().dcreg_align_correspondences_device(other._h, devs[0].ptr, *args) == -4
        assert api.load().dcreg_align_correspondences(other._h, wa.ctypes.data, 400, 4, wb.ctypes.data, 400, 6, ca.ctypes.data, cb.ctypes.data, 400,
                                                      C.byref(p), recs, None, C.byref(info)) == -4
        assert info.n_pairs == 0 and not any(recs[0].T)
        other.linearize_end(slot=0)
        assert sums() == before
    finally:
        other.close()
        for d in devs:
            d.free()


def test_the_result_does_not_depend_on_the_split():
    a, b, ca, cb = pairs(1000, 0.3, 7)
    kw = dict(n_hypotheses=600, seed=13, inlier_distance=0.2, edge_similarity=0.0, n_best=32, refine_iterations=1)
    ref = ar.align(a, b, ca, cb, **kw)
    c = api.Context(0)
    try:
        for split in (0, 1, TILE - 1, TILE, 333, 999, 1000, 5000):
            c.set_option("align_score_split", split)
            assert_same(c.align_correspondences(a, b, ca, cb, api.align_params(**kw)), ref, split)
    finally:
        c.close()


@pytest.mark.parametrize("name", sorted(sc.RECOVERY))
def test_the_recovery_scenes_are_the_references(ctx, name):
    (a, b, ca, cb, R, t, inlier), kw, ref = sc.recovery(name)
    got = ctx.align_correspondences(a, b, ca, cb, api.align_params(**kw))
    assert_same(got, ref, name)
    assert np.array_equal(got["mask"] != 0, inlier)          # (what tests/test_align_reference.py asserts of the reference)


def test_the_library_refuses_what_the_header_lists(ctx):
    L = api.load()
    a, b, ca, cb = pairs(10, 1.0, 8)
    recs = (api.AlignRecord * 32)()
    info = api.AlignInfo()

    def call(form="dcreg_align_correspondences", c=ctx._h, pa=a.ctypes.data, na=10, sa=3, pb=b.ctypes.data, nb=10, sb=3, ia=ca.ctypes.data, ib=cb.ctypes.data,
             m=10, r=recs, **fields):
        p = api.align_params(n_hypotheses=50)
        for k, v in fields.items():
            setattr(p, k, v)
        return getattr(L, form)(c, pa, na, sa, pb, nb, sb, ia, ib, m, C.byref(p), r, None, C.byref(info))

    assert call() == api.OK and info.n_used == 10 and info.n_drawn == 50
    bad = [dict(c=None), dict(r=None), dict(pa=None), dict(pb=None), dict(ia=None), dict(ib=None), dict(sa=2), dict(sb=0), dict(na=-1), dict(nb=-1),
           dict(m=-1), dict(na=2 ** 31), dict(nb=2 ** 31), dict(m=2 ** 31), dict(n_hypotheses=0), dict(n_hypotheses=(1 << 24) + 1), dict(n_best=0),
           dict(n_best=33), dict(refine_iterations=-1), dict(refine_iterations=9), dict(inlier_distance=0.0), dict(inlier_distance=-1.0),
           dict(inlier_distance=np.nan), dict(inlier_distance=np.inf), dict(edge_similarity=-0.1), dict(edge_similarity=1.0), dict(edge_similarity=np.nan)]
    for form in ("dcreg_align_correspondences", "dcreg_align_correspondences_device"):
        for kw in bad:
            assert call(form, **kw) == -1, (form, kw)
        assert getattr(L, form)(ctx._h, a.ctypes.data, 10, 3, b.ctypes.data, 10, 3, ca.ctypes.data, cb.ctypes.data, 10, None, recs, None, None) == -1
    # nothing to read: null clouds and index arrays with zero counts are fine
    assert call(na=0, pa=None) == api.OK and info.n_used == 0 and call(m=0, ia=None, ib=None) == api.OK and info.n_pairs == 0


def test_descriptors_matching_and_alignment_bring_the_lot_onto_its_moved_copy(ctx):
    cloud = lot_cloud()
    normals = ctx.normals(cloud, api.normal_params(k=16))[0]
    mc, mn = moved_copy(cloud, normals)
    fp = api.fpfh_params(k=16)
    fa, fb = ctx.fpfh(cloud, normals, params=fp)[0], ctx.fpfh(mc, mn, params=fp)[0]
    match = ctx.feature_match(fa, fb)
    ca, cb = api.correspondences_from_match(match, mutual_only=True, max_ratio=None)
    assert len(ca) >= 0.99 * len(cloud)
    d = 0.5
    kw = dict(n_hypotheses=2000, seed=1, inlier_distance=d, edge_similarity=0.9, n_best=8, refine_iterations=3)
    got = ctx.align_correspondences(cloud, mc, ca, cb, api.align_params(**kw))
    assert_same(got, ar.align(cloud, mc, ca, cb, **kw), "lot")
    T = got["records"][0]["T"]
    err = np.linalg.norm(cloud.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - mc.astype(np.float64), axis=1)
    print("lot: pairs", len(ca), "info", got["info"], "inliers", got["records"][0]["n_inliers"], "max error", err.max())
    assert err.max() <= d
    # the records' poses are start poses as the engines take them
    c = api.Context(0)
    try:
        c.set_target(mc, 0.5)
        c.set_source(cloud)
        c.keep_target_normals(api.normal_params(k=10))
        res = c.icp_run_trials_normals([r["T"] for r in got["records"]], "Ours", cfg_pk01(max_iterations=3))
        assert len(res) == len(got["records"]) == 8
    finally:
        c.close()
