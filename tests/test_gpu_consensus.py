"""The consensus pose on the device (dcreg_consensus_correspondences*) against tests/consensus_ref.py, which applies include/dcreg.h's
rule literally: records, mask, member lists, degrees, weights and counters must be the reference's bit for bit - every field, doubles as
bit patterns - across the word, wave and tile boundaries of the graph's kernels, on complete and empty graphs, with ties everywhere."""
import ctypes as C

import numpy as np
import pytest

import align_ref as ar
import align_scenes as sc
import consensus_ref as cr
import consensus_scenes as cs
import helpers as h
from dcreg_amd import api
from test_fpfh_reference import lot_cloud, moved_copy
from test_gpu_device_seam import D2H, DevCloud, hip, strided
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

INT_FIELDS = ("seed", "seed_rank", "weight", "n_members", "count", "cost", "n_inliers", "refined")
SMALL = dict(compat_distance=0.10, min_length=1.0, inlier_distance=0.10, n_seeds=64, consensus_size=16, n_best=5, refine_iterations=2)


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
    for f in ("mask", "members", "degree", "weight"):
        if got.get(f) is not None:
            assert got[f].dtype == ref[f].dtype and np.array_equal(got[f], ref[f]), (what, f)


def both(ctx, a, b, ca, cb, what="", **kw):
    got = ctx.consensus_correspondences(a, b, ca, cb, api.consensus_params(**kw), want_members=True, want_weights=True)
    ref = cr.consensus(a, b, ca, cb, **kw)
    assert_same(got, ref, what)
    return got, ref


def pairs(m, share=0.3, seed=0):
    return sc.synthetic(m, share, 0.02, 300 + seed)[:4]


@pytest.mark.parametrize("m_u", [3, 4, 63, 64, 65, 127, 128, 129, 257])
def test_used_pairs_across_the_word_wave_and_tile_boundaries(ctx, m_u):
    a, b, ca, cb = pairs(m_u, 1.0 if m_u < 5 else 0.3, m_u)
    got, ref = both(ctx, a, b, ca, cb, m_u, **SMALL)
    i = ref["info"]
    assert i["n_used"] == m_u and i["n_edges"] > 0 and i["n_scored"] > 0 and i["n_seeds"] == min(64, m_u)


def test_a_complete_graph_ties_everywhere(ctx):
    a, b, ca, cb = cs.dense(130, 50)
    got, ref = both(ctx, a, b, ca, cb, "dense", **dict(SMALL, n_seeds=130, n_best=32))
    assert ref["info"]["n_edges"] == 130 * 129 // 2 and ref["info"]["max_degree"] == 129
    assert (ref["degree"] == 129).all() and (ref["weight"] == 129 * 128).all()          # every S is M - 2
    # ascending u decides: the seeds are the first pairs, the members of each the first fifteen others
    assert [r["seed_rank"] for r in got["records"]] == list(range(32)) and all(r["count"] == 130 for r in got["records"])
    assert got["records"][0]["seed"] == 0 and list(got["members"][0]) == list(range(16))
    assert got["records"][20]["seed"] == 20 and list(got["members"][20]) == list(range(15)) + [20]


def test_an_empty_graph_returns_nothing(ctx):
    a, b, ca, cb = pairs(90, 0.0, 1)
    got, ref = both(ctx, a, b, ca, cb, "empty", **dict(SMALL, compat_distance=1e-9))
    i = got["info"]
    assert i["n_edges"] == 0 and i["n_seeds"] == 64 == i["n_skipped"] and i["n_scored"] == 0 and got["records"] == []
    assert not got["mask"].any() and not got["degree"].any() and not got["weight"].any() and (got["members"] == -1).all()


@pytest.mark.parametrize("wrong", [0, 16])
def test_ties_in_the_weights_and_the_counts(ctx, wrong):
    g, b, ia, ib = cs.rotated_lattice(48, wrong)
    got, ref = both(ctx, g, b, ia, ib, "lattice", compat_distance=1e-6, min_length=1.0, inlier_distance=0.1, n_seeds=48, consensus_size=16, n_best=32,
                    refine_iterations=1)
    w = ref["weight"]
    assert len(set(w.tolist())) < len(w) // 2 and ref["info"]["n_returned"] == 32
    assert got["records"][0]["count"] == 48 - wrong and got["records"][0]["cost"] == 0


def test_one_to_many_pairs_have_no_edge_between_them(ctx):
    a, b, ca, cb = cs.dense(60, 51)
    ca, cb = ca.copy(), cb.copy()
    ca[10:15], cb[20:25] = ca[10], cb[20]                  # one point of a matched to five of b, five of a to one of b
    ca[30:34], cb[30:34] = ca[30], cb[30]                  # one pair four times: equal lengths on both sides, zero apart
    kw = dict(SMALL, min_length=0.0)
    got, ref = both(ctx, a, b, ca, cb, "one to many", **kw)
    m_of_u, p, q = ar.used_pairs(a, b, ca, cb)
    Cm = cr.compatibility(p, q, ca.astype(np.int64), cb.astype(np.int64), 0.10, 0.0)
    assert not Cm[10:15, 10:15].any() and not Cm[20:25, 20:25].any() and not Cm[30:34, 30:34].any() and Cm[30, 0] and Cm[31, 0]
    assert got["degree"][31] == Cm[31].sum() and got["degree"][0] > got["degree"][31] > 0


@pytest.mark.parametrize("n_seeds", [1, 7, 1024])
@pytest.mark.parametrize("consensus_size", [3, 16, 64])
def test_the_numbers_of_seeds_and_members(ctx, n_seeds, consensus_size):
    a, b, ca, cb = pairs(150, 0.3, 2)
    got, ref = both(ctx, a, b, ca, cb, (n_seeds, consensus_size), **dict(SMALL, n_seeds=n_seeds, consensus_size=consensus_size, n_best=32))
    assert ref["info"]["n_seeds"] == min(n_seeds, 150) and ref["members"].shape == (32, consensus_size)
    top = ref["records"][0]["n_members"]
    assert (top == consensus_size) if consensus_size < 64 else (16 < top < 64)          # (64: more than any set has candidates)


@pytest.mark.parametrize("n_best", [1, 5, 32])
@pytest.mark.parametrize("refine", [0, 1, 8])
def test_the_number_of_records_and_the_refinement_steps(ctx, n_best, refine):
    a, b, ca, cb = pairs(150, 0.3, 3)
    got, ref = both(ctx, a, b, ca, cb, (n_best, refine), **dict(SMALL, n_best=n_best, refine_iterations=refine))
    assert len(ref["records"]) == n_best and ref["records"][0]["refined"] == refine


def test_the_minimum_length(ctx):
    rng = np.random.default_rng(9)
    a = rng.uniform(-0.25, 0.25, (70, 3)).astype(np.float32)          # a cluster: no two points a metre apart
    b = (a + np.array([3.0, 1.0, -2.0], np.float32)).astype(np.float32)
    idx = np.arange(70, dtype=np.int32)
    got, ref = both(ctx, a, b, idx, idx, "clustered", **SMALL)
    assert ref["info"]["n_edges"] == 0 and got["records"] == [] and ref["info"]["n_skipped"] == 64
    got, ref = both(ctx, a, b, idx, idx, "clustered, any length", **dict(SMALL, min_length=0.0))
    assert ref["info"]["n_edges"] == 70 * 69 // 2 and got["records"][0]["count"] == 70


def test_a_seed_skipped_in_the_middle_of_the_rank_is_not_replaced(ctx):
    a, b, ca, cb = cs.hinge(4)
    kw = dict(SMALL, n_seeds=8, n_best=32)
    # by rank: the clique's five pairs, the two pairs on the hinge's axis with one candidate each, the first of the pairs around it
    assert cs.seed_sets(a, b, ca, cb, **kw) == [5, 5, 5, 5, 5, 2, 2, 3]
    got, ref = both(ctx, a, b, ca, cb, "skipped", **kw)
    i = got["info"]
    assert (i["n_seeds"], i["n_skipped"], i["n_scored"], i["n_returned"]) == (8, 2, 6, 6)
    assert sorted(r["seed_rank"] for r in got["records"]) == [0, 1, 2, 3, 4, 7] and list(ref["weight"][:8]) == [12] * 5 + [8, 8, 2]
    # one seed fewer: the skipped ones are counted, no further seed is taken in their place
    got, ref = both(ctx, a, b, ca, cb, "skipped, seven seeds", **dict(kw, n_seeds=7))
    assert (got["info"]["n_seeds"], got["info"]["n_skipped"], got["info"]["n_scored"]) == (7, 2, 5)


def test_unused_pairs_strides_and_reordered_inputs(ctx):
    a, b, ca, cb = [x.copy() for x in pairs(150, 0.3, 5)]
    a[7, 1], b[9, 2], b[11, 0] = np.nan, np.inf, -np.inf
    ca[3], cb[4], ca[5], cb[6] = -1, -1, 150, 2 ** 31 - 1
    got, ref = both(ctx, a, b, ca, cb, "unused", **SMALL)
    unused = ref["info"]["n_pairs"] - ref["info"]["n_used"]
    assert 4 <= unused <= 7 and ref["info"]["n_scored"] > 0
    for f in ("mask", "degree", "weight"):
        assert not got[f][[3, 4, 5, 6]].any()
    # strided clouds: the further columns are not read
    wa, wb = strided(a, 5), strided(b, 7)
    p = api.consensus_params(**SMALL)
    assert_same(ctx.consensus_correspondences(wa, wb, ca, cb, p, want_members=True, want_weights=True), ref, "strided")
    # the clouds reordered, the same pairs in the same order: the same graph, the same records
    pa, pb = np.random.default_rng(1).permutation(150), np.random.default_rng(2).permutation(150)
    inv_a, inv_b = np.argsort(pa).astype(np.int32), np.argsort(pb).astype(np.int32)
    ok_a, ok_b = (ca >= 0) & (ca < 150), (cb >= 0) & (cb < 150)
    ca2, cb2 = np.where(ok_a, inv_a[np.clip(ca, 0, 149)], ca), np.where(ok_b, inv_b[np.clip(cb, 0, 149)], cb)
    assert_same(ctx.consensus_correspondences(a[pa], b[pb], ca2, cb2, p, want_members=True, want_weights=True), ref, "reordered")
    # fewer than three used pairs, and none at all
    got, ref = both(ctx, a, b, np.array([7, 1, -1, 2], np.int32), np.array([0, 1, 2, 9], np.int32), "two", **SMALL)
    assert ref["info"]["n_used"] == 1 and got["records"] == [] and not got["mask"].any() and (got["members"] == -1).all()
    got, ref = both(ctx, a, b, np.zeros(0, np.int32), np.zeros(0, np.int32), "none", **SMALL)
    assert got["info"]["n_pairs"] == 0 and got["records"] == []
    both(ctx, np.zeros((0, 3), np.float32), b, ca, cb, "no points", **SMALL)


def test_the_device_form_repeated_calls_and_a_second_context(ctx):
    a, b, ca, cb = pairs(400, 0.1, 6)
    wa, wb = strided(a, 4), strided(b, 6)
    kw = dict(SMALL, n_best=7, consensus_size=12)
    p = api.consensus_params(**kw)
    first = ctx.consensus_correspondences(wa, wb, ca, cb, p, want_members=True, want_weights=True)
    assert first["info"]["n_returned"] == 7
    assert_same(first, cr.consensus(a, b, ca, cb, **kw), "host form")
    assert_same(ctx.consensus_correspondences(wa, wb, ca, cb, p, want_members=True, want_weights=True), first, "again")
    as_f32 = lambda x: np.ascontiguousarray(x).view(np.float32).reshape(-1, 1)
    devs = [DevCloud(wa), DevCloud(wb), DevCloud(as_f32(ca)), DevCloud(as_f32(cb)), DevCloud(np.ones((100, 1), np.float32)),
            DevCloud(np.ones((7 * 12, 1), np.float32)), DevCloud(np.ones((400, 1), np.float32)), DevCloud(np.ones((400, 1), np.float32))]
    other = api.Context(0)
    try:
        got = ctx.consensus_correspondences_device(devs[0].ptr, 400, 4, devs[1].ptr, 400, 6, devs[2].ptr, devs[3].ptr, 400, p, devs[4].ptr, devs[5].ptr,
                                                   devs[6].ptr, devs[7].ptr)
        for name, dev, arr in (("mask", devs[4], np.zeros(400, np.uint8)), ("members", devs[5], np.zeros((7, 12), np.int32)),
                               ("degree", devs[6], np.zeros(400, np.uint32)), ("weight", devs[7], np.zeros(400, np.uint32))):
            assert hip().hipMemcpy(C.c_void_p(arr.ctypes.data), C.c_void_p(dev.ptr), arr.nbytes, D2H) == 0
            got[name] = arr
        assert_same(got, first, "device form")
        # without the optional outputs
        bare = ctx.consensus_correspondences_device(devs[0].ptr, 400, 4, devs[1].ptr, 400, 6, devs[2].ptr, devs[3].ptr, 400, p)
        assert_same(bare, dict(first, mask=None, members=None, degree=None, weight=None), "device form, bare")
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
        assert_same(other.consensus_correspondences(wa, wb, ca, cb, p, want_members=True, want_weights=True), first, "second context")
        assert sums() == before
        # a linearisation in flight: DCREG_E_STATE from both forms, nothing written
        other.linearize_begin(T0[:3, :3], T0[:3, 3], prm, slot=0)
        recs, info = (api.ConsensusRecord * 7)(), api.ConsensusInfo()
        tail = (400, 6, devs[2].ptr, devs[3].ptr, 400, C.byref(p), recs, None, None, None, None, C.byref(info))
        assert api.load().dcreg_consensus_correspondences_device(other._h, devs[0].ptr, 400, 4, devs[1].ptr, *tail) == -4
        assert api.load().dcreg_consensus_correspondences(other._h, wa.ctypes.data, 400, 4, wb.ctypes.data, 400, 6, ca.ctypes.data, cb.ctypes.data, 400,
                                                          C.byref(p), recs, None, None, None, None, C.byref(info)) == -4
        assert info.n_pairs == 0 and not any(recs[0].T)
        other.linearize_end(slot=0)
        assert sums() == before
    finally:
        other.close()
        for d in devs:
            d.free()


@pytest.mark.parametrize("name", sorted(cs.RECOVERY))
def test_the_recovery_scenes_are_the_references(ctx, name):
    (a, b, ca, cb, R, t, inlier), kw, ref = cs.solved("recovery", name)
    got = ctx.consensus_correspondences(a, b, ca, cb, api.consensus_params(**kw), want_members=True, want_weights=True)
    assert_same(got, ref, name)
    assert np.array_equal(got["mask"] != 0, inlier)        # (what tests/test_consensus_reference.py asserts of the reference)


def test_the_weights_clean_the_pairs_for_the_sampler(ctx):
    (a, b, ca, cb, R, t, inlier), kw, ref = cs.solved("fails", "m2000")
    got = ctx.consensus_correspondences(a, b, ca, cb, api.consensus_params(**kw), want_weights=True)
    assert_same(got, ref, "fails")
    keep = np.flatnonzero(got["weight"] > 0)
    assert inlier[keep].sum() == inlier.sum() and keep.size < 1000
    rec = ctx.align_correspondences(a, b, ca[keep], cb[keep], api.align_params(n_hypotheses=100000, seed=7, inlier_distance=0.10, edge_similarity=0.9))
    print("kept", keep.size, "of", len(ca), "true", int(inlier.sum()), "sampler inliers", rec["records"][0]["n_inliers"])
    assert (rec["mask"][inlier[keep]] != 0).all()


def test_the_library_refuses_what_the_header_lists(ctx):
    L = api.load()
    a, b, ca, cb = pairs(10, 1.0, 8)
    recs = (api.ConsensusRecord * 32)()
    info = api.ConsensusInfo()

    def call(form="dcreg_consensus_correspondences", c=ctx._h, pa=a.ctypes.data, na=10, sa=3, pb=b.ctypes.data, nb=10, sb=3, ia=ca.ctypes.data,
             ib=cb.ctypes.data, m=10, r=recs, **fields):
        p = api.consensus_params(n_seeds=5)
        for k, v in fields.items():
            setattr(p, k, v)
        return getattr(L, form)(c, pa, na, sa, pb, nb, sb, ia, ib, m, C.byref(p), r, None, None, None, None, C.byref(info))

    assert call() == api.OK and info.n_used == 10 and info.n_seeds == 5
    bad = [dict(c=None), dict(r=None), dict(pa=None), dict(pb=None), dict(ia=None), dict(ib=None), dict(sa=2), dict(sb=0), dict(na=-1), dict(nb=-1),
           dict(m=-1), dict(na=2 ** 31), dict(nb=2 ** 31), dict(m=32769), dict(m=2 ** 31), dict(compat_distance=0.0), dict(compat_distance=-1.0),
           dict(compat_distance=np.nan), dict(compat_distance=np.inf), dict(min_length=-0.5), dict(min_length=np.nan), dict(min_length=np.inf),
           dict(inlier_distance=0.0), dict(inlier_distance=-1.0), dict(inlier_distance=np.nan), dict(inlier_distance=np.inf), dict(n_seeds=0),
           dict(n_seeds=1025), dict(consensus_size=2), dict(consensus_size=65), dict(n_best=0), dict(n_best=33), dict(refine_iterations=-1),
           dict(refine_iterations=9)]
    for form in ("dcreg_consensus_correspondences", "dcreg_consensus_correspondences_device"):
        for kw in bad:
            assert call(form, **kw) == -1, (form, kw)
        assert getattr(L, form)(ctx._h, a.ctypes.data, 10, 3, b.ctypes.data, 10, 3, ca.ctypes.data, cb.ctypes.data, 10, None, recs, None, None, None, None,
                                None) == -1
    # nothing to read: null clouds and index arrays with zero counts are fine
    assert call(na=0, pa=None) == api.OK and info.n_used == 0 and call(m=0, ia=None, ib=None) == api.OK and info.n_pairs == 0


def test_descriptors_matching_and_consensus_bring_the_lot_onto_its_moved_copy(ctx):
    cloud = lot_cloud()
    normals = ctx.normals(cloud, api.normal_params(k=16))[0]
    mc, mn = moved_copy(cloud, normals)
    fp = api.fpfh_params(k=16)
    fa, fb = ctx.fpfh(cloud, normals, params=fp)[0], ctx.fpfh(mc, mn, params=fp)[0]
    match = ctx.feature_match(fa, fb)
    ca, cb = api.correspondences_from_match(match, mutual_only=True, max_ratio=None)
    assert len(ca) >= 0.99 * len(cloud)
    d = 0.5
    kw = dict(compat_distance=0.05, min_length=1.0, inlier_distance=d, n_seeds=8, consensus_size=16, n_best=8, refine_iterations=3)
    got = ctx.consensus_correspondences(cloud, mc, ca, cb, api.consensus_params(**kw), want_members=True, want_weights=True)
    assert_same(got, cr.consensus(cloud, mc, ca, cb, **kw), "lot")
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
