"""The fourth engine's pairs form on the device: the batched keep (dcreg_pairs_voxels_build: one voxel map per target of a build batch)
against dcreg_target_voxels_keep on fresh contexts and against the numpy reference, the launch with a voxel map per pose
(dcreg_pairs_voxels_batch_begin, k_vlin_pairs) against single launches of dcreg_linearize_voxels on fresh contexts, the engine
dcreg_register_pairs_voxels against the serial sequence it promises, what it leaves alone and what it refuses - everything bitwise unless
said otherwise.  The scenes are those of tests/voxels_scenes.py, tests/voxels_edge_scenes.py, tests/normal_icp_scenes.py and the dense lot
of tests/test_gpu_voxels_engine.py; what a fresh context or the serial sequence gives is computed once per module and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import gicp_scenes as gs
import helpers as h
import normal_icp_scenes as sc
import sums_check as sums
import voxels_edge_scenes as ve
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api
from test_gpu_normals import OPTS_WINDOW
from test_gpu_voxels import INFO_KEYS, MAP_PARAMS, lin_params
from test_gpu_voxels_engine import REFERENCE_FINAL, dense_lot
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
PARAMS_5 = api.normal_params(k=5)
SIZES = [1, 63, 64, 65, 255, 256, 257, 523]
EMPTY3 = sc.frozen(np.zeros((0, 3), np.float32))
# five points three metres apart: every voxel holds one point at either leaf below, nothing is kept
FIVE = sc.frozen((np.arange(5, dtype=np.float32)[:, None] * np.float32(3.0) + np.float32([0.25, 0.5, 0.75])).astype(np.float32))
# bytes a target of m points is planned at with stride 3 (context.hip pair_voxel_target_bytes)
PLANNED = lambda m: 256.0 + 200.0 * m


def last_error(c):
    return c._L.dcreg_last_error(c._h).decode()


def refused(call, code, text=""):
    with pytest.raises(api.DcregError) as e:
        call()
    assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)


# ---- 1. the batched keep
PARAM_SETS = {"leaf 1.0, 6 points": (1.0, vs.EPS, 6), "leaf 0.5, 2 points": (0.5, vs.EPS, 2)}
KEEP_NAMES = ["lot", "planted", "lattice", "single", "lattice_plus", "lattice_minus", "far_lot", "five", "empty"]


def keep_target(name):
    if name == "five":
        return FIVE
    if name == "empty":
        return EMPTY3
    if name in vs.MAPS:
        return vs.MAPS[name]()["tgt"]
    return (ve.far_lot() if name == "far_lot" else ve.TABLES[name]())["tgt"]


def info_of(d):
    return {k: int(d[k]) for k in INFO_KEYS}


@functools.lru_cache(maxsize=None)
def alone(tgt_bytes, shape, params):
    """set_target + keep_target_voxels + kept_target_voxels on a fresh context, and the numpy reference: once per (target, parameters)
    -> (info, kept map or None, reference)"""
    tgt = np.frombuffer(tgt_bytes, np.float32).reshape(shape)
    ref = vr.voxel_map(tgt, *params)
    c = api.Context(0)
    try:
        c.set_target(tgt, RADIUS)
        info = c.keep_target_voxels(api.voxel_map_params(*params))
        kept = c.kept_target_voxels() if info["n_kept"] else None
        assert c.target_voxels_kept() == info["n_kept"]
    finally:
        c.close()
    return info, kept, ref


def check_batch(c, tgts, infos, params, what):
    assert len(infos) == len(tgts)
    for t, tgt in enumerate(tgts):
        if len(tgt) == 0:
            assert infos[t] == dict.fromkeys(INFO_KEYS, 0) and c.pairs_voxels_kept(t) == 0, (what, t)
            continue
        info, kept, ref = alone(np.ascontiguousarray(tgt).tobytes(), tgt.shape, params)
        assert infos[t] == info == info_of(ref), (what, t, infos[t], info)
        assert c.pairs_voxels_kept(t) == info["n_kept"], (what, t)
        got = c.pairs_kept_voxels(t)
        assert len(got["count"]) == info["n_kept"]
        if info["n_kept"]:
            vs.assert_map_bitwise(got, kept, (what, t, "fresh context"))
        vs.assert_map_bitwise(got, ref, (what, t, "reference"))
    assert c.pairs_voxels_kept(len(tgts)) == 0 and c.pairs_voxels_kept(-1) == 0
    refused(lambda: c.pairs_kept_voxels(len(tgts)), api.E_INVALID, "not in the batch")


@pytest.mark.parametrize("pname", list(PARAM_SETS))
@pytest.mark.parametrize("order", ["as listed", "permuted"])
def test_a_batch_keeps_every_targets_voxels_as_a_context_of_its_own_does(pname, order):
    params = PARAM_SETS[pname]
    names = KEEP_NAMES if order == "as listed" else [KEEP_NAMES[k] for k in np.random.default_rng(11).permutation(len(KEEP_NAMES))]
    tgts = [keep_target(n) for n in names]
    c = api.Context(0)                       # (a context that never had a target)
    try:
        refused(lambda: c.pairs_kept_voxels(0), api.E_STATE, "no pair voxel batch built")
        infos = c.pairs_voxels_build(tgts, api.voxel_map_params(*params))
        check_batch(c, tgts, infos, params, (pname, order))
        kept = dict(zip(names, [i["n_kept"] for i in infos]))
        assert kept["five"] == 0 and kept["empty"] == 0 and kept["lot"] > 0
        if params[0] == 1.0:
            assert (kept["single"], kept["lattice"], kept["lattice_plus"], kept["lattice_minus"]) == (1, 4096, 4097, 4095)
        assert c.index_info().n_target == 0 and c.target_voxels_kept() == 0
        # a build replaces the batch; a refused one leaves it
        infos2 = c.pairs_voxels_build(tgts[:3][::-1], api.voxel_map_params(*params))
        check_batch(c, tgts[:3][::-1], infos2, params, (pname, order, "second"))
        bad = [tgts[0], FIVE.copy()]
        bad[1][2, 1] = np.nan
        refused(lambda: c.pairs_voxels_build(bad, api.voxel_map_params(*params)), api.E_INVALID, "pair target 1 has non-finite coordinates")
        check_batch(c, tgts[:3][::-1], infos2, params, (pname, order, "after a refusal"))
    finally:
        c.close()


TOP = (1 << 20) - 2                          # the widest box the library takes (tests/test_gpu_voxels_edges.py)
WIDE_PARAMS = (ve.WIDE_LEAF, vs.EPS, vs.MIN_POINTS)


def wide_targets():
    """the widest target between two others: 63 bits of voxel key and two bits of cloud id - the order takes its two-sort path.  The
    planted map scaled by the leaf (a power of two: the voxels of the scaled points at leaf 2^-7 are those of the points at leaf 1)"""
    W = ve.wide(TOP)
    assert W["span"] == (ve.WIDE_SPAN_MAX,) * 3
    scaled = sc.frozen((vs.planted()["tgt"] * np.float32(ve.WIDE_LEAF)).astype(np.float32))
    return [scaled, W["tgt"], sc.frozen(W["tgt"][::-1].copy()), FIVE]


def test_a_batch_with_the_widest_target_is_ordered_by_two_sorts():
    tgts = wide_targets()
    c = api.Context(0)
    try:
        infos = c.pairs_voxels_build(tgts, api.voxel_map_params(*WIDE_PARAMS))
        check_batch(c, tgts, infos, WIDE_PARAMS, "wide")
        assert infos[0]["n_kept"] > 0 and infos[1]["n_kept"] == ve.wide(TOP)["vmap"]["n_kept"] > 0 and infos[3]["n_kept"] == 0
        # one voxel wider, in any place of the batch: refused, and the batch stays
        B = ve.wide(TOP + 1)
        for k in range(len(tgts) + 1):
            refused(lambda: c.pairs_voxels_build(tgts[:k] + [B["tgt"]] + tgts[k:], api.voxel_map_params(*WIDE_PARAMS)), api.E_INVALID,
                    "pair target %d spans 2097152 voxels" % k)
        refused(lambda: c.pairs_voxels_build(tgts, api.voxel_map_params(ve.WIDE_LEAF_ONE_MORE, vs.EPS, vs.MIN_POINTS)), api.E_INVALID, "spans 2097152 voxels")
        refused(lambda: c.pairs_voxels_build([FIVE], api.voxel_map_params(1e-19, vs.EPS, vs.MIN_POINTS)), api.E_INVALID, "2^62")
        check_batch(c, tgts, infos, WIDE_PARAMS, "wide, after the refusals")
    finally:
        c.close()


# ---- 2. the launch at block and target edges
LOT, PLANTED, PLUS, MINUS, FULL, NOTHING, SINGLE = range(7)


@functools.lru_cache(maxsize=None)
def launch_targets():
    return [vs.lot()["tgt"], vs.planted()["tgt"], ve.lattice_plus()["tgt"], ve.lattice_minus()["tgt"], ve.full()["tgt"], FIVE, ve.single()["tgt"]]


@functools.lru_cache(maxsize=None)
def launch_sources():
    """-> (sources, source normals, {name: source id}): the sized sources, the scenes' own, and the eight points of the lattice's source
    that lie in the voxel only lattice_plus has (extra) and in the one lattice_minus lacks (missing)"""
    L, P, LP, F, S = vs.lot(), vs.planted(), ve.lattice_plus(), ve.full(), ve.single()
    srcs = [sc.sized_source(n) for n in SIZES] + [L["src"], P["src"], LP["src"], F["src"], S["src"], LP["src"][-16:-8], LP["src"][-8:]]
    nrms = [gs.sized_source_normals(n) for n in SIZES] + [L["mb"], P["src_normals"], LP["src_normals"], F["src_normals"], S["src_normals"],
                                                          LP["src_normals"][-16:-8], LP["src_normals"][-8:]]
    ids = {n: i for i, n in enumerate(SIZES)}
    ids.update({name: len(SIZES) + k for k, name in enumerate(("lot", "planted", "lattice", "full", "single", "extra", "missing"))})
    assert (vr.voxel_of(srcs[ids["extra"]], vs.LEAF) == np.float64(ve.LATTICE_EXTRA)).all()
    assert (vr.voxel_of(srcs[ids["missing"]], vs.LEAF) == np.float64(ve.LATTICE_MISSING)).all()
    return [np.ascontiguousarray(s, np.float32) for s in srcs], [np.ascontiguousarray(n, np.float32) for n in nrms], ids


def launch_plan():
    """(source name, target, pose): the targets in unsorted order, the lot many times, a pose against the target that kept nothing, a
    1-point source beside the 523-point one, and the two lattice voxels against three tables each in the same launch"""
    W = sc.walk()
    I = np.eye(4)
    LP, F, S = ve.lattice_plus(), ve.full(), ve.single()
    return [(523, LOT, W[0]), (1, LOT, W[0]), ("single", SINGLE, S["T"]), (257, LOT, W[2]), ("planted", PLANTED, I), (63, LOT, W[1]),
            ("lattice", PLUS, LP["T"]), (65, NOTHING, I), (256, LOT, W[0]), ("full", FULL, F["T"]), (523, LOT, W[3]), ("lattice", MINUS, LP["T"]),
            ("extra", PLUS, I), ("extra", FULL, I), ("extra", MINUS, I), ("missing", MINUS, I), ("missing", PLUS, I), ("missing", FULL, I),
            (64, LOT, W[2]), (255, LOT, W[1]), (65, LOT, W[0]), ("lot", LOT, W[2]), ("lot", NOTHING, W[0]), (257, LOT, W[0])]


_singles = {}


def single(src_name, tgt, T, mode, opts=()):
    """linearize_voxels on a fresh context with that target's kept voxels and that source: once per (source, target, pose, mode, options)"""
    k = (src_name, tgt, np.asarray(T).tobytes(), mode, tuple(opts))
    if k not in _singles:
        srcs, nrms, ids = launch_sources()
        c = api.Context(0)
        try:
            for name, v in opts:
                c.set_option(name, v)
            c.set_option("voxels_source_cov", mode)
            c.set_target(launch_targets()[tgt], RADIUS)
            kept = c.keep_target_voxels(MAP_PARAMS)["n_kept"]
            c.set_source(srcs[ids[src_name]])
            if mode:
                c.set_source_normals(nrms[ids[src_name]])
            if kept:
                _singles[k] = c.linearize_voxels(T, lin_params())
            else:                             # (the single call refuses a map without a member: DCREG_E_STATE)
                refused(lambda: c.linearize_voxels(T, lin_params()), api.E_STATE, "no kept voxels")
                _singles[k] = None
        finally:
            c.close()
    return _singles[k]


ROBUST = (("robust_kernel", 3.0), ("gicp_robust_scale", 0.7))


@pytest.mark.parametrize("mode,opts", [(0, ()), (1, ()), (1, ROBUST)], ids=["mode 0", "mode 1", "mode 1, robust kernel 3"])
def test_a_launch_with_a_voxel_map_per_pose_is_bitwise_its_single_launches(mode, opts):
    tgts = launch_targets()
    srcs, nrms, ids = launch_sources()
    plan = launch_plan()
    c = api.Context(0)                       # (a context that never had a target)
    try:
        for name, v in opts:
            c.set_option(name, v)
        c.set_option("voxels_source_cov", mode)
        c.pairs_sources_load(srcs)
        if mode:
            c.pairs_sources_normals_set(nrms)
        infos = c.pairs_voxels_build(tgts, MAP_PARAMS)
        assert infos[NOTHING]["n_kept"] == 0 and infos[LOT]["n_kept"] == vs.lot()["vmap"]["n_kept"]
        sids, tids, Ts = [ids[s] for s, _, _ in plan], [t for _, t, _ in plan], [T for _, _, T in plan]
        got = c.pairs_voxels_batch(Ts, sids, tids, lin_params())
        assert len(got) == len(plan)
        for k, ((s, t, T), g) in enumerate(zip(plan, got)):
            want = single(s, t, T, mode, opts)
            if want is None:                  # the target that kept nothing: the zero row
                assert t == NOTHING and (g["n_eff"], g["n_pt"], g["sum_r2"], g["sum_b2"]) == (0, 0, 0.0, 0.0), k
                assert not np.any(g["H_upper"]) and not np.any(g["g"]), k
                continue
            sc.assert_sums_bitwise(g, want, (mode, k, s, t))
        again = c.pairs_voxels_batch(Ts[::-1], sids[::-1], tids[::-1], lin_params(), slot=1)      # the other slot, the other order
        for a, g in zip(again[::-1], got):
            sc.assert_sums_bitwise(a, g)
        assert got[0]["n_eff"] >= 10 and got[1]["n_pt"] <= 1
        # the planted pair's counts are those its flags imply
        flags = vs.planted()["flags1" if mode else "flags0"]
        planted = got[[s for s, _, _ in plan].index("planted")]
        assert (planted["n_eff"], planted["n_pt"]) == (sum(f == 1 for f in flags), sum(f != 0 for f in flags))
        # every target answers from its own table: the eight points in the voxel that only lattice_plus keeps, and the eight in the one
        # that lattice_minus does not keep, in the same launch (the unit source normals are finite: every point in a kept voxel counts)
        by = {(s, t): g for (s, t, _), g in zip(plan, got)}
        assert [by[("extra", t)]["n_pt"] for t in (PLUS, FULL, MINUS)] == [8, 0, 0]
        assert [by[("missing", t)]["n_pt"] for t in (PLUS, FULL, MINUS)] == [8, 0, 0]
        assert by[("extra", PLUS)]["n_eff"] == 8 and by[("missing", PLUS)]["n_eff"] == 8
        if not opts:
            # one pose against the numpy reference: the counts exactly, every sum against its own terms
            s, t, T = plan[0]
            assert (s, t) == (523, LOT)
            want = vr.linearize(vs.lot()["vmap"], sc.sized_source(s), T, mode, gs.sized_source_normals(s) if mode else None, vs.GICP_EPS)
            sc.assert_sums_close(got[0], want, "reference")
            sums.assert_sums_entrywise(got[0], want["row"], want["n_eff"], want["n_pt"], "reference")
            assert want["n_eff"] >= 10
    finally:
        c.close()


def test_the_seam_refuses_what_is_not_there():
    tgts = launch_targets()
    srcs, nrms, ids = launch_sources()
    W = sc.walk()
    c = api.Context(0)
    try:
        one = lambda s=0, t=0, T=W[0], **kw: c.pairs_voxels_batch_begin([T], [s], [t], lin_params(), **kw)
        refused(one, api.E_STATE, "no pair voxel batch built")
        c.pairs_voxels_build(tgts, MAP_PARAMS)
        refused(one, api.E_STATE, "no pair sources")
        c.pairs_sources_load(srcs + [EMPTY3])
        for bad in (len(srcs) + 1, -1, len(srcs)):
            refused(lambda: one(s=bad), api.E_INVALID, "pair source %d is not loaded or empty" % bad)
        for bad in (len(tgts), -1):
            refused(lambda: one(t=bad), api.E_INVALID, "pair target %d is not in the voxel batch" % bad)
        c.set_option("voxels_source_cov", 1)
        refused(one, api.E_STATE, "no kept pair source normals")
        c.set_option("voxels_source_cov", 0)
        bad_pose = W[0].copy()
        bad_pose[1, 3] = np.nan
        refused(lambda: one(T=bad_pose), api.E_INVALID, "a pose is not finite")
        for slot in (2, -1):
            refused(lambda: one(slot=slot), api.E_INVALID, "invalid slot %d" % slot)
        for slot in (0, 1):
            refused(lambda: c.voxels_batch_end(1, slot=slot), api.E_STATE)          # nothing was queued
        # a pending slot refuses the next launch there and every call that queues work; the other slot takes one
        n0 = one(s=ids[523], t=LOT)
        refused(lambda: one(s=ids[523], t=LOT), api.E_STATE, "slot 0")
        refused(lambda: c.pairs_voxels_build(tgts, MAP_PARAMS), api.E_STATE)
        refused(lambda: c.pairs_sources_load(srcs), api.E_STATE)
        refused(lambda: c.pairs_kept_voxels(0), api.E_STATE)
        n1 = one(s=ids[257], t=LOT, T=W[2], slot=1)
        sc.assert_sums_bitwise(c.voxels_batch_end(n1, slot=1)[0], single(257, LOT, W[2], 0))
        sc.assert_sums_bitwise(c.voxels_batch_end(n0, slot=0)[0], single(523, LOT, W[0], 0))
        # the pairs' index batch of the other engines is another member: a build of either leaves the other
        c.pairs_build(tgts[:2], RADIUS)
        sc.assert_sums_bitwise(c.pairs_voxels_batch([W[0]], [ids[523]], [LOT], lin_params())[0], single(523, LOT, W[0], 0))
    finally:
        c.close()


# ---- 3. the call against the serial sequence
PREFIXES = [1500, 523, 257, 64, 9, 1, 0]
DENSE_FIRST, LOT_PAIR, PLANTED_PAIR, EMPTY_TGT_PAIR, NOTHING_PAIR = 0, 1, 2, 9, 10


@functools.lru_cache(maxsize=None)
def pairs_scene():
    """eleven pairs: the dense lot's 1 500-point frame against its 40 000-point map, the 4 000-point lot with its frame, the planted map,
    then the prefixes 523 .. 0 of the dense frame against the dense map, an empty target and a target that keeps nothing.  Checked with the
    numpy reference engine (tests/voxels_ref.py icp) when the test was written, in both modes and with both methods, 30 iterations
    allowed: the four longest prefixes, the lot and the planted pair converge (14 / 9 / 11 / 10, 12 and 7 iterations in mode 0; 17 / 10 /
    11 / 13, 15 and 4 in mode 1), the 9-point and the 1-point prefix end with status 1 at their first launch"""
    D, L, P = dense_lot(), vs.lot(), vs.planted()
    srcs = [D["src"], L["src"], P["src"]] + [sc.frozen(np.ascontiguousarray(D["src"][:n])) for n in PREFIXES[1:]] + [L["src"], L["src"]]
    tgts = [D["tgt"], L["tgt"], P["tgt"]] + [D["tgt"]] * (len(PREFIXES) - 1) + [EMPTY3, FIVE]
    Ts = [D["INIT"], L["INIT"], np.eye(4)] + [D["INIT"]] * (len(PREFIXES) - 1) + [L["INIT"], L["INIT"]]
    assert len(srcs) == 11 and len(srcs[8]) == 0
    return srcs, tgts, [np.array(T) for T in Ts]


def cfg_of(max_iterations):
    return cfg_pk01(max_iterations=max_iterations, gt_matrix=np.ascontiguousarray(dense_lot()["GT"]).reshape(16))


def serial_record(c, src, tgt, T0, method, cfg, mode):
    """the sequence the call promises, on context c; None where it has nothing to run (the call: status 3)"""
    if len(src) == 0 or len(tgt) == 0:
        return None
    c.set_target(tgt, RADIUS)
    if c.keep_target_voxels(MAP_PARAMS)["n_kept"] == 0:
        c.set_source(src)
        refused(lambda: c.icp_run_voxels(T0, method, cfg), api.E_STATE, "no kept voxels")       # the documented departure: the call gives status 3
        return None
    c.set_source(src)
    if mode:
        c.keep_source_normals(PARAMS_5)
    res, logs = c.icp_run_voxels(T0, method, cfg)
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    last = logs[-1] if logs else None
    return dict(T=T.reshape(16), iterations=res.iterations, converged=res.converged, status=res.status,
                rmse=last.rmse if last else 0.0, fitness=last.fitness if last else 0.0, corr=last.effective_points if last else 0,
                H=np.array(last.H_upper[:]) if last else np.zeros(21), mask=list(last.analysis.degenerate_mask[:]) if last else [0] * 6,
                trans_err=last.trans_error_vs_gt if last else None, rot_err=last.rot_error_vs_gt if last else None)


@functools.lru_cache(maxsize=None)
def serial_records(method, mode, cap):
    srcs, tgts, Ts = pairs_scene()
    cfg = cfg_of(cap)
    c = api.Context(0)
    try:
        c.set_option("voxels_source_cov", mode)
        recs = [serial_record(c, s, t, T, method, cfg, mode) for s, t, T in zip(srcs, tgts, Ts)]
    finally:
        c.close()
    # not vacuous: the two kinds of status 3, the status-1 pairs, and - where the cap allows - converged pairs
    assert [k for k, r in enumerate(recs) if r is None] == [8, EMPTY_TGT_PAIR, NOTHING_PAIR]
    assert all((recs[k]["status"], recs[k]["iterations"]) == (1, 1) for k in (6, 7))
    conv = [k for k, r in enumerate(recs) if r is not None and r["converged"] == 1]
    print("%s mode %d cap %d: converged %s, iterations %s" % (method, mode, cap, conv, [r["iterations"] if r else None for r in recs]))
    if cap == 30:
        assert set(conv) >= {DENSE_FIRST, LOT_PAIR, PLANTED_PAIR, 3, 4, 5}
        if (method, mode) in REFERENCE_FINAL:                              # the dense pair ends within the cap that scene already has
            cap_t, cap_r = REFERENCE_FINAL[(method, mode)]
            t_err, r_err = vr.pose_error(recs[DENSE_FIRST]["T"].reshape(4, 4), dense_lot()["GT"])
            assert t_err < 2.0 * cap_t and r_err < 2.0 * cap_r, (t_err, r_err)
    else:
        r = recs[DENSE_FIRST]
        assert (r["status"], r["converged"], r["iterations"]) == (0, 0, cap)
    return recs


def check(recs, want, order=None):
    order = list(range(len(want))) if order is None else order
    assert len(recs) == len(order)
    for tr, p in zip(recs, order):
        s = want[p]
        if s is None:
            assert (tr.status, tr.iterations, tr.converged) == (3, 0, 0), p
            continue
        h.assert_record(tr, s, p)
        if s["trans_err"] is not None and tr.status == 0:
            assert tr.trans_error_m == s["trans_err"] and tr.rot_error_deg == s["rot_err"], p


def planned_batches(c, tgts):
    off = np.concatenate([[0], np.cumsum([len(t) for t in tgts])]).astype(np.int64)
    ends, nb = (C.c_int32 * len(tgts))(), C.c_int(0)
    assert c._L.dcreg_pairs_plan_voxels(c._h, len(tgts), off.ctypes.data_as(C.POINTER(C.c_int64)), 3, ends, C.byref(nb)) == 0
    return [int(e) for e in ends[:nb.value]]


# a budget that holds one dense target and nothing beside it: the dense pairs are batches of one pair, the small targets share theirs
SMALL_BUDGET = PLANNED(40000) + 300.0


@pytest.mark.parametrize("slots,budget", [(1, 0.0), (3, SMALL_BUDGET), (0, 0.0)], ids=["1 slot", "3 slots, small batches", "default slots"])
@pytest.mark.parametrize("cap", [1, 4, 30])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("method", ["Ours", "NONE"])
def test_pairs_are_bitwise_the_serial_sequence(method, mode, cap, slots, budget):
    srcs, tgts, Ts = pairs_scene()
    want = serial_records(method, mode, cap)
    c = api.Context(0)
    try:
        c.set_option("voxels_source_cov", mode)
        if budget:
            c.set_option("pairs_max_bytes", budget)
            ends = planned_batches(c, tgts)
            assert len(ends) >= 3 and ends[0] == 1 and ends[1] == 3, ends          # the dense pair alone, then the lot with the planted map
        recs = c.register_pairs_voxels(srcs, tgts, Ts, method, cfg_of(cap), MAP_PARAMS, PARAMS_5 if mode else None, slots=slots)
        check(recs, want)
        info = c.index_info()
        assert info.n_target == 0 and info.n_source == 0 and c.target_voxels_kept() == 0 and c.source_normals_kept() == 0
    finally:
        c.close()


def test_the_order_of_the_pairs_does_not_change_a_record():
    srcs, tgts, Ts = pairs_scene()
    want = serial_records("Ours", 0, 30)
    order = [int(p) for p in np.random.default_rng(5).permutation(len(srcs))]
    c = api.Context(0)
    try:
        c.set_option("pairs_max_bytes", 2.5 * PLANNED(40000))
        recs = c.register_pairs_voxels([srcs[p] for p in order], [tgts[p] for p in order], [Ts[p] for p in order], "Ours", cfg_of(30), MAP_PARAMS, slots=5)
        check(recs, want, order)
        assert c.register_pairs_voxels([], [], np.zeros((0, 4, 4)), "Ours", cfg_of(30), MAP_PARAMS) == []
    finally:
        c.close()


# ---- 4. what the call leaves alone
def test_the_context_is_left_alone():
    """own target with kept voxels and kept normals, a source with kept normals, loaded frames with theirs, an active window index: the
    same bits afterwards as on a control context that did not make the calls; and the pairs forms of the other engines beside this one"""
    L = gs.lot()
    W = sc.walk()
    srcs, tgts, Ts = pairs_scene()
    cfg = cfg_of(30)
    frames = [L["src"], sc.sized_source(257)]
    fnormals = [L["mb"], gs.sized_source_normals(257)]
    prm = api.default_lin_params(RADIUS, 1)
    sub = [1, 2, 5, 7, 8, 10]                 # the lot, the planted pair, a prefix, a status-1 pair and both kinds of status 3
    pick = lambda xs: [xs[p] for p in sub]

    def engines(c, T):
        R, t = np.ascontiguousarray(T[:3, :3]).reshape(9), np.ascontiguousarray(T[:3, 3])
        o = api.LinOut()
        c.linearize_raw(R, t, prm, o)
        first = dict(H_upper=np.array(o.H_upper[:]), g=np.array(o.g[:]), sum_r2=o.sum_r2, sum_b2=o.sum_b2, n_eff=o.n_eff, n_pt=o.n_pt)
        return [first, c.linearize_normals(T, prm), c.linearize_gicp(T, prm), c.linearize_voxels(T, prm)]

    def getters(c):
        roi = c.roi_info()
        vox = c.kept_target_voxels()
        arrays = list(c.kept_target_normals()) + list(c.kept_source_normals()) + [vox[k] for k in ("coords", "count", "mean", "cov")]
        info = c.index_info()
        return arrays, (info.n_target, info.n_source, c.target_normals_kept(), c.source_normals_kept(), c.frames_normals_kept(), c.target_voxels_kept(),
                        roi["active"], roi["windows_built"])

    seq = {}
    for name in ("call", "control"):
        c = api.Context(0)
        try:
            for k, v in OPTS_WINDOW:
                c.set_option(k, v)
            c.set_target(L["tgt"], RADIUS)
            c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
            c.keep_target_voxels(MAP_PARAMS)
            c.set_source(L["src"])
            c.set_source_normals(np.ascontiguousarray(L["mb"], np.float32))
            c.frames_load(frames)
            c.frames_normals_set(fnormals)
            out = engines(c, W[0])
            assert c.roi_info()["active"]
            arrays, state = getters(c)
            if name == "call":
                for mode in (0, 1):
                    c.set_option("voxels_source_cov", mode)
                    recs = c.register_pairs_voxels(pick(srcs), pick(tgts), pick(Ts), "Ours", cfg, MAP_PARAMS, PARAMS_5 if mode else None, slots=3)
                    check(recs, serial_records("Ours", mode, 30), sub)
                c.set_option("voxels_source_cov", 0)
            arrays2, state2 = getters(c)
            assert state2 == state and state[6]
            for a, b in zip(arrays2, arrays):
                assert sc.same_bits(a, b)
            out += engines(c, W[1])
            out += c.voxels_batch([W[1], W[2]], [0, 1], prm)
            out += c.gicp_batch([W[1], W[2]], None, [0, 1], prm)
            seq[name] = out
        finally:
            c.close()
    for a, b in zip(seq["call"], seq["control"]):
        sc.assert_sums_bitwise(a, b)


def test_the_pairs_forms_of_the_engines_follow_one_another():
    """register_pairs, register_pairs_gicp and register_pairs_voxels on one context, in either order: each still gives its own records"""
    srcs, tgts, Ts = pairs_scene()
    cfg = cfg_of(30)
    sub = [1, 5, 7, 9]
    s, t, T = [srcs[p] for p in sub], [tgts[p] for p in sub], [Ts[p] for p in sub]
    key = lambda recs: [(r.iterations, r.status, r.converged, bytes(bytearray(r.final_transform)), r.final_rmse, r.corr_num, bytes(bytearray(r.H_upper)))
                        for r in recs]
    a = api.Context(0)
    try:
        planes, gicp = key(a.register_pairs(s, t, T, "Ours", cfg, slots=2)), key(a.register_pairs_gicp(s, t, T, "Ours", cfg, PARAMS_5, PARAMS_5, slots=2))
    finally:
        a.close()
    c = api.Context(0)
    try:
        check(c.register_pairs_voxels(s, t, T, "Ours", cfg, MAP_PARAMS, slots=2), serial_records("Ours", 0, 30), sub)
        assert key(c.register_pairs(s, t, T, "Ours", cfg, slots=2)) == planes
        check(c.register_pairs_voxels(s, t, T, "Ours", cfg, MAP_PARAMS, slots=2), serial_records("Ours", 0, 30), sub)
        assert key(c.register_pairs_gicp(s, t, T, "Ours", cfg, PARAMS_5, PARAMS_5, slots=2)) == gicp
        c.set_option("voxels_source_cov", 1)
        check(c.register_pairs_voxels(s, t, T, "Ours", cfg, MAP_PARAMS, PARAMS_5, slots=2), serial_records("Ours", 1, 30), sub)
        assert key(c.register_pairs_gicp(s, t, T, "Ours", cfg, PARAMS_5, PARAMS_5, slots=2)) == gicp
        assert key(c.register_pairs(s, t, T, "Ours", cfg, slots=2)) == planes
    finally:
        c.close()


# ---- 5. refusals queue nothing
SENTINEL = -7


def raw_call(c, srcs, tgts, Ts, cfg, tv, sn):
    """the C call with prefilled results -> (code, every record's iterations as they come back)"""
    sxyz, soff, txyz, toff, width, R0, t0, n = api.Context._pairs_args(srcs, tgts, Ts, "test")
    res = (api.TrialResult * max(n, 1))()
    for r in res:
        r.iterations = SENTINEL
    fp, i64 = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    rc = c._L.dcreg_register_pairs_voxels(c._h, n, sxyz.ctypes.data_as(fp), soff.ctypes.data_as(i64), txyz.ctypes.data_as(fp), toff.ctypes.data_as(i64), width,
                                          None if tv is None else C.byref(tv), None if sn is None else C.byref(sn), api._dp(R0), api._dp(t0), 0, 0,
                                          C.byref(cfg), 0, res)
    return rc, [r.iterations for r in res][:n]


def test_refusals_queue_nothing():
    L = vs.lot()
    W = sc.walk()
    srcs = [L["src"], sc.sized_source(257), sc.sized_source(65), sc.sized_source(523)]
    tgts = [L["tgt"], L["tgt"], vs.planted()["tgt"], L["tgt"]]
    Ts = [W[0], W[2], np.eye(4), W[1]]
    cfg = cfg_pk01()
    wide_params = api.voxel_map_params(*WIDE_PARAMS)
    untouched = [SENTINEL] * 4
    c = api.Context(0)
    try:
        c.set_target(L["tgt"], RADIUS)
        c.set_source(L["src"])
        c.keep_target_voxels(MAP_PARAMS)
        before = c.linearize_voxels(W[1], lin_params())
        # a target of exactly 2^21 voxels on every axis, and a non-finite coordinate: in the first build batch, then in a later one
        too_wide = ve.wide(TOP + 1)["tgt"]
        assert tuple(np.subtract(*vs.box_of(too_wide, ve.WIDE_LEAF)[::-1]) + 1) == (ve.WIDE_SPAN_MAX + 1,) * 3
        nan_tgt = L["tgt"].copy()
        nan_tgt[100, 2] = np.nan
        for budget in (0.0, 1.0):             # one batch; a batch per pair
            c.set_option("pairs_max_bytes", budget)
            for place in ((0,) if budget == 0.0 else (0, 3)):
                wide_tgts = [ve.wide(TOP)["tgt"]] * 4
                assert raw_call(c, srcs, wide_tgts, Ts, cfg, wide_params, None)[0] == api.OK        # the widest that is taken runs
                wide_tgts[place] = too_wide
                assert raw_call(c, srcs, wide_tgts, Ts, cfg, wide_params, None) == (api.E_INVALID, untouched), (budget, place)
                assert "pair target %d spans 2097152 voxels" % (0 if budget == 0.0 or place == 0 else place) in last_error(c)
                bad = list(tgts)
                bad[place] = nan_tgt
                assert raw_call(c, srcs, bad, Ts, cfg, MAP_PARAMS, None) == (api.E_INVALID, untouched), (budget, place)
                assert "non-finite" in last_error(c)
        # a leaf too small for the coordinates, first and later batch
        tiny = api.voxel_map_params(1e-19, vs.EPS, vs.MIN_POINTS)
        assert raw_call(c, srcs, tgts, Ts, cfg, tiny, None) == (api.E_INVALID, untouched) and "2^62" in last_error(c)
        c.set_option("pairs_max_bytes", 0.0)
        assert raw_call(c, srcs, tgts, Ts, cfg, tiny, None) == (api.E_INVALID, untouched) and "2^62" in last_error(c)
        bad_src = [s.copy() for s in srcs]
        bad_src[2][5, 1] = np.inf
        assert raw_call(c, bad_src, tgts, Ts, cfg, MAP_PARAMS, None) == (api.E_INVALID, untouched)
        # bad parameter blocks, with pairs and without
        for field, value in (("leaf", 0.0), ("leaf", np.nan), ("leaf", np.inf), ("epsilon", 0.5e-6), ("epsilon", 1.5), ("min_points", 1)):
            p = api.voxel_map_params()
            setattr(p, field, value)
            assert raw_call(c, srcs, tgts, Ts, cfg, p, None) == (api.E_INVALID, untouched), (field, value)
            assert raw_call(c, [], [], np.zeros((0, 4, 4)), cfg, p, None)[0] == api.E_INVALID, (field, value)
        assert raw_call(c, srcs, tgts, Ts, cfg, None, None) == (api.E_INVALID, untouched) and "null voxel map parameters" in last_error(c)
        # mode 1 reads source_normals, mode 0 does not
        bad_n = api.normal_params()
        bad_n.k = 2
        assert raw_call(c, [], [], np.zeros((0, 4, 4)), cfg, MAP_PARAMS, bad_n)[0] == api.OK
        c.set_option("voxels_source_cov", 1)
        assert raw_call(c, srcs, tgts, Ts, cfg, MAP_PARAMS, bad_n) == (api.E_INVALID, untouched) and "normal k" in last_error(c)
        assert raw_call(c, srcs, tgts, Ts, cfg, MAP_PARAMS, None) == (api.E_INVALID, untouched) and "null normal parameters" in last_error(c)
        assert raw_call(c, [], [], np.zeros((0, 4, 4)), cfg, MAP_PARAMS, bad_n)[0] == api.E_INVALID            # ... before the empty call returns
        c.set_option("voxels_source_cov", 0)
        # a launch slot pending
        n = c.voxels_batch_begin([W[0]], None, lin_params(), slot=1)
        assert raw_call(c, srcs, tgts, Ts, cfg, MAP_PARAMS, None) == (api.E_STATE, untouched)
        c.voxels_batch_end(n, slot=1)
        # the context is as it was, and a good call afterwards runs
        info = c.index_info()
        assert info.n_target == 4000 and info.n_source == 523 and c.target_voxels_kept() == L["vmap"]["n_kept"]
        sc.assert_sums_bitwise(c.linearize_voxels(W[1], lin_params()), before)
        rc, its = raw_call(c, srcs, tgts, Ts, cfg, MAP_PARAMS, None)
        assert rc == api.OK and all(i > 0 for i in its)
    finally:
        c.close()


def source_normals_code(c, n):
    """dcreg_pairs_sources_normals_get with room for n points -> its code (DCREG_E_STATE: the pairs' sources keep no normals)"""
    out = np.empty((max(n, 1), 4), np.float32)
    return c._L.dcreg_pairs_sources_normals_get(c._h, out.ctypes.data, n)


def test_mode_0_runs_no_normals_pass_and_the_mode_is_read_once_per_call():
    L = vs.lot()
    W = sc.walk()
    srcs = [L["src"], sc.sized_source(257), EMPTY3]
    tgts = [L["tgt"], L["tgt"], L["tgt"]]
    Ts = [W[0], W[1], W[0]]
    cfg = cfg_pk01()
    c = api.Context(0)
    try:
        recs = c.register_pairs_voxels(srcs, tgts, Ts, "Ours", cfg, MAP_PARAMS, source_normals=None)
        assert recs[2].status == 3 and recs[0].iterations > 0
        assert source_normals_code(c, 780) == api.E_STATE                          # mode 0: no normals pass ran, none are kept
        c.set_option("voxels_source_cov", 1)
        refused(lambda: c.register_pairs_voxels(srcs, tgts, Ts, "Ours", cfg, MAP_PARAMS, source_normals=None), api.E_INVALID, "null normal parameters")
        assert source_normals_code(c, 780) == api.E_STATE
        recs1 = c.register_pairs_voxels(srcs, tgts, Ts, "Ours", cfg, MAP_PARAMS, source_normals=PARAMS_5)
        assert source_normals_code(c, 780) == api.OK and source_normals_code(c, 779) == api.E_INVALID
        assert recs1[2].status == 3 and recs1[0].iterations > 0
        assert not np.array_equal(np.array(recs1[0].H_upper[:]), np.array(recs[0].H_upper[:]))
        # all sources empty: nothing to estimate, every record status 3
        assert [r.status for r in c.register_pairs_voxels([EMPTY3] * 2, tgts[:2], Ts[:2], "Ours", cfg, MAP_PARAMS, source_normals=PARAMS_5)] == [3, 3]
        # back in mode 0 the records are mode 0's again
        c.set_option("voxels_source_cov", 0)
        again = c.register_pairs_voxels(srcs, tgts, Ts, "Ours", cfg, MAP_PARAMS)
        assert np.array_equal(np.array(again[0].H_upper[:]), np.array(recs[0].H_upper[:])) and again[0].iterations == recs[0].iterations
    finally:
        c.close()
