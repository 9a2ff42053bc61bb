"""dcreg_register_pairs: many scan pairs registered in one call, each against a target of its own.  Every pair's record is bitwise the single
registration of that pair (dcreg_set_target + dcreg_set_source + dcreg_icp_run) on a second context - targets of 3 to 200 k points
side by side, a planar target, a target 10 km from the origin, duplicate points, a source far off its target, empty clouds, identical
pairs - whatever the slots, the one-wave rule, the build batches or the order of the pairs; the context's own clouds and states are left
alone; the last iteration agrees with the CPU oracle; bad input is refused before anything runs."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from oracle import pyoracle as po
from test_gpu_configs import cfg_pair
from test_gpu_frames import _assert_record, _frame_poses, _same_sums, _single

pytestmark = pytest.mark.gpu

TGT_SIZES = [200_000, 50, 120_000, 5_000, 80_000, 30_000, 150_000, 1_000, 60_000, 100_000, 12_000, 200, 90_000, 40_000]
SRC_SIZES = [8000, 40, 12000, 500, 3000, 8000, 257, 1000, 6000, 8000, 2000, 63, 9000, 4000]
PLANAR, FAR_AWAY, DUPLICATES, TINY, OFF_TARGET, EMPTY_SRC, EMPTY_TGT, TWIN_A, TWIN_B = range(14, 23)
N_PAIRS = 23


def _pairs(tgt, gt):
    """23 pairs: 14 submap crops of the parking lot (50 - 200 k points) with frames of 40 - 12 k points, then the special cases"""
    T, T0 = _frame_poses(gt, N_PAIRS, seed=21, step=5.0)
    srcs = h.map_frames(tgt, T[:14], SRC_SIZES, seed=4)
    rng = np.random.default_rng(8)
    tgts = []
    for k, m in enumerate(TGT_SIZES):
        d = tgt[:, :2] - T[k][:2, 3].astype(np.float32)
        near = np.flatnonzero((d * d).sum(1) < np.float32(45.0 * 45.0))
        tgts.append(np.ascontiguousarray(tgt[np.sort(rng.choice(near, size=min(m, len(near)), replace=False))]))
    srcs, tgts, T0 = list(srcs), tgts, list(T0[:14])
    # a planar target with zero z-extent, its frame cut out of it
    g = np.stack(np.meshgrid(np.arange(-30, 30, 0.12), np.arange(-30, 30, 0.12)), -1).reshape(-1, 2)
    plane = np.zeros((len(g), 3), np.float32)
    plane[:, :2] = g + rng.uniform(-0.03, 0.03, g.shape)
    Tp = h.pose6d_matrix(1.0, -2.0, 1.5, 0.0, 0.0, 0.3)
    sel = rng.choice(len(plane), 5000, replace=False)
    srcs.append(((plane[sel].astype(np.float64) - Tp[:3, 3]) @ Tp[:3, :3]).astype(np.float32))
    tgts.append(plane)
    T0.append(Tp @ h.pose6d_matrix(0.05, -0.04, 0.0, 0.0, 0.0, 0.01))
    # a target 10 km from the origin (the crop of pair 3 moved there, with its frame's pose)
    shift = np.array([10_000.0, -200.0, 30.0])
    tgts.append((tgts[3].astype(np.float64) + shift).astype(np.float32))
    srcs.append(srcs[3])
    Tf = T0[3].copy()
    Tf[:3, 3] += shift
    T0.append(Tf)
    # duplicate points and exact ties: every point of a crop twice
    tgts.append(np.concatenate([tgts[5], tgts[5]], 0))
    srcs.append(srcs[5])
    T0.append(T0[5])
    # a target of 3 points: nothing to fit (status 1)
    tgts.append(tgts[9][:3].copy())
    srcs.append(srcs[9])
    T0.append(T0[9])
    # a source far off its target (status 1)
    tgts.append(tgts[0])
    srcs.append(srcs[0])
    T0.append(T0[0] @ h.pose6d_matrix(300.0, 0.0, 0.0, 0.0, 0.0, 0.0))
    # an empty source, an empty target (status 3)
    tgts.append(tgts[4]); srcs.append(np.zeros((0, 3), np.float32)); T0.append(T0[4])
    tgts.append(np.zeros((0, 3), np.float32)); srcs.append(srcs[4]); T0.append(T0[4])
    # two pairs with identical contents
    for _ in range(2):
        tgts.append(tgts[2].copy()); srcs.append(srcs[2].copy()); T0.append(T0[2].copy())
    assert len(srcs) == len(tgts) == len(T0) == N_PAIRS
    return srcs, tgts, T0


def _single_pair(ctx, tgt, src, T0, method, cfg):
    if len(src) == 0 or len(tgt) == 0:
        return None
    ctx.set_target(tgt, cfg.search_radius)
    return _single(ctx, src, T0, method, cfg)


def _check(recs, singles, order=None):
    assert len(recs) == len(singles)
    for k, tr in enumerate(recs):
        p = order[k] if order is not None else k
        s = singles[p]
        if s is None:
            assert tr.status == 3 and tr.iterations == 0, p
            continue
        _assert_record(tr, s, p)
        if s["trans_err"] is not None and tr.status == 0:
            assert tr.trans_error_m == s["trans_err"], p


@pytest.fixture(scope="module")
def scene():
    tgt, _ = h.scene_parkinglot()
    gt = h.pose6d_matrix(**h.PK01_GT)
    srcs, tgts, T0 = _pairs(tgt, gt)
    cfgs = {"thresholds": cfg_pair(0.5, 30, 0, 1e-5, 1e-3, gt.reshape(16)), "no_thresholds": cfg_pair(0.5, 12, 1)}
    return srcs, tgts, T0, cfgs


@pytest.fixture(scope="module")
def singles(scene):
    srcs, tgts, T0, cfgs = scene
    out = {}
    c = api.Context(0)
    try:
        for method in ("Ours", "ME-SR"):
            for name, (cfg, _) in cfgs.items():
                out[method, name] = [_single_pair(c, t, s, T, method, cfg) for s, t, T in zip(srcs, tgts, T0)]
    finally:
        c.close()
    ref = out["Ours", "thresholds"]
    assert ref[TINY]["status"] == 1 and ref[OFF_TARGET]["status"] == 1
    assert ref[PLANAR]["status"] != 1 and ref[TWIN_A]["iterations"] == ref[TWIN_B]["iterations"]
    return out


@pytest.mark.parametrize("method", ["Ours", "ME-SR"])
@pytest.mark.parametrize("thresholds", ["thresholds", "no_thresholds"])
def test_pairs_are_bitwise_single_registrations(scene, singles, method, thresholds):
    srcs, tgts, T0, cfgs = scene
    cfg = cfgs[thresholds][0]
    c = api.Context(0)
    try:
        recs = c.register_pairs(srcs, tgts, T0, method, cfg)
        _check(recs, singles[method, thresholds])
        assert recs[TWIN_A].status == 0 and np.array_equal(np.array(recs[TWIN_A].final_transform[:]), np.array(recs[TWIN_B].final_transform[:]))
        info = c.index_info()
        assert info.n_target == 0 and info.n_source == 0                        # nothing was ever set on this context
    finally:
        c.close()


@pytest.mark.parametrize("variant", ["slots_1", "slots_3", "slots_256", "one_wave_off", "one_wave_forced", "three_batches", "permuted"])
def test_scheduling_does_not_change_a_record(scene, singles, variant):
    srcs, tgts, T0, cfgs = scene
    cfg = cfgs["thresholds"][0]
    ref = singles["Ours", "thresholds"]
    c = api.Context(0)
    try:
        order = list(range(N_PAIRS))
        slots = 0
        if variant.startswith("slots_"):
            slots = int(variant.split("_")[1])
        elif variant == "one_wave_off":
            c.set_option("one_wave_batches", 0)
        elif variant == "one_wave_forced":
            c.set_option("one_wave", 2)
        elif variant == "three_batches":
            c.set_option("pairs_max_bytes", 3.0 * 4 * (1 << 24))       # about two pairs per build batch at the default table budget
            slots = 5
        elif variant == "permuted":
            order = list(np.random.default_rng(3).permutation(N_PAIRS))
            slots = 7
        recs = c.register_pairs([srcs[p] for p in order], [tgts[p] for p in order], [T0[p] for p in order], "Ours", cfg, slots=slots)
        _check(recs, ref, order)
    finally:
        c.close()


def test_the_context_is_left_alone(scene, singles):
    """target, source, own neighbour state and reserved warm states of the context: linearisations after the call give what they give
    without it; and the call also runs on a context that never had a target"""
    srcs, tgts, T0, cfgs = scene
    cfg = cfgs["thresholds"][0]
    tgt, src, T = tgts[0], srcs[0], T0[0]
    prm = api.default_lin_params(0.5, 0)
    D = h.pose6d_matrix(0.05, 0, 0, 0, 0, 0)
    Rs, ts = [T[:3, :3], (T @ D)[:3, :3]], [T[:3, 3], (T @ D)[:3, 3]]
    a, b = api.Context(0), api.Context(0)
    try:
        seq = {}
        for name, c in (("call", a), ("control", b)):
            c.set_target(tgt, 0.5)
            c.set_source(src)
            c.reserve_warm_states(2)
            first = c.linearize(T[:3, :3], T[:3, 3], prm)
            bfirst = c.linearize_batch_warm(Rs, ts, [0, 1], prm)
            if name == "call":
                recs = c.register_pairs(srcs[:10], tgts[:10], T0[:10], "Ours", cfg, slots=4)
                _check(recs, singles["Ours", "thresholds"][:10])
            info = c.index_info()
            assert info.n_target == len(tgt) and info.n_source == len(src)
            T2 = T @ h.pose6d_matrix(0.01, -0.02, 0.0, 0.0, 0.0, 0.001)
            second = c.linearize(T2[:3, :3], T2[:3, 3], prm)
            bsecond = c.linearize_batch_warm(Rs, ts, [0, 1], prm)
            seq[name] = (first, bfirst, second, bsecond)
        fa, ba, sa, bsa = seq["call"]
        fb, bb, sb, bsb = seq["control"]
        assert _same_sums(fa, fb) and _same_sums(sa, sb)
        assert all(_same_sums(x, y) for x, y in zip(ba + bsa, bb + bsb))
    finally:
        a.close(); b.close()


def test_a_pair_record_matches_the_oracle(scene, singles):
    """the 3000-point frame against its 80 k-point crop: its record against the last iteration of the CPU oracle's run"""
    srcs, tgts, T0, cfgs = scene
    cfg, ocfg = cfgs["thresholds"]
    k = 4
    assert singles["Ours", "thresholds"][k]["status"] == 0
    c = api.Context(0)
    try:
        tr = c.register_pairs(srcs, tgts, T0, "Ours", cfg, slots=8)[k]
    finally:
        c.close()
    ores, ologs = po.icp_run(po.KdTree(tgts[k]), srcs[k], T0[k], "Ours", ocfg)
    assert (tr.iterations, tr.converged, tr.status) == (ores.iterations, ores.converged, ores.status)
    assert tr.corr_num == ologs[-1].n_eff
    T = np.array(tr.final_transform[:]).reshape(4, 4)
    assert np.allclose(T[:3, :3].reshape(9), ores.R[:], rtol=0, atol=1e-8) and np.allclose(T[:3, 3], ores.t[:], rtol=0, atol=1e-8)
    assert h.rel_err(tr.H_upper[:], ologs[-1].H_upper[:]) < 1e-7


def _raw_call(c, src, soff, tgt, toff, T0s, cfg):
    n = len(soff) - 1
    T0s = np.asarray(T0s, np.float64).reshape(-1, 4, 4)
    R0 = np.ascontiguousarray(T0s[:, :3, :3]).reshape(-1, 9)
    t0 = np.ascontiguousarray(T0s[:, :3, 3]).reshape(-1, 3)
    res = (api.TrialResult * max(n, 1))()
    fp, i64 = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    soff, toff = np.ascontiguousarray(soff, np.int64), np.ascontiguousarray(toff, np.int64)
    return c._L.dcreg_register_pairs(c._h, n, src.ctypes.data_as(fp), soff.ctypes.data_as(i64), tgt.ctypes.data_as(fp), toff.ctypes.data_as(i64), 3,
                                     R0.ctypes.data_as(C.POINTER(C.c_double)), t0.ctypes.data_as(C.POINTER(C.c_double)), 0, 0, C.byref(cfg), 0, res)


def test_refusals(scene, singles):
    srcs, tgts, T0, cfgs = scene
    cfg = cfgs["thresholds"][0]
    c = api.Context(0)
    try:
        c.set_target(tgts[3], 0.5)
        c.set_source(srcs[3])
        before = c.launch_stats()["launches"]
        for which in ("source", "target"):
            bad_s, bad_t = [s.copy() for s in srcs[:4]], [t.copy() for t in tgts[:4]]
            (bad_s if which == "source" else bad_t)[2][5, 1] = np.nan
            with pytest.raises(api.DcregError, match=r"\(-\d+\).*non-finite"):
                c.register_pairs(bad_s, bad_t, T0[:4], "Ours", cfg)
        # a NaN in a later build batch: refused before the first batch runs
        c.set_option("pairs_max_bytes", 1.0)
        bad_t = [t.copy() for t in tgts[:4]]
        bad_t[3][0, 0] = np.inf
        with pytest.raises(api.DcregError, match="non-finite"):
            c.register_pairs(srcs[:4], bad_t, T0[:4], "Ours", cfg)
        c.set_option("pairs_max_bytes", 0.0)
        s = np.concatenate(srcs[:3], 0)
        t = np.concatenate(tgts[:3], 0)
        soff = np.concatenate([[0], np.cumsum([len(x) for x in srcs[:3]])])
        toff = np.concatenate([[0], np.cumsum([len(x) for x in tgts[:3]])])
        for so, to in ((soff, [0, 40, 30, len(t)]), ([1, 40, 50, len(s)], toff), (soff, [5, 40, 50, len(t)])):
            assert _raw_call(c, s, so, t, to, T0[:3], cfg) == -1
        assert c.launch_stats()["launches"] == before
        info = c.index_info()
        assert info.n_target == len(tgts[3]) and info.n_source == len(srcs[3])
        assert c.register_pairs([], [], np.zeros((0, 4, 4)), "Ours", cfg) == []
        assert c.launch_stats()["launches"] == before
        # a linearisation waiting for its pose: refused at once
        prm = api.default_lin_params(0.5, 0)
        c.linearize_gated_begin(prm, slot=0)
        with pytest.raises(api.DcregError, match=r"\(-4\)"):
            c.register_pairs(srcs[:2], tgts[:2], T0[:2], "Ours", cfg)
        c.gate_abort()
        _check(c.register_pairs(srcs[:2], tgts[:2], T0[:2], "Ours", cfg), singles["Ours", "thresholds"][:2])
    finally:
        c.close()
