"""The pairs forms of the second and third engines on the device: the batched launches with a target per pose (k_nlin_batch<GRIDS>,
k_glin_batch<GRIDS>) against single launches on fresh contexts, the normals pass over a build batch (dcreg_pairs_normals_keep) against
Context.normals of every target alone, the engines dcreg_register_pairs_normals / dcreg_register_pairs_gicp against the serial sequence
they promise, what they leave alone and what they refuse - everything bitwise.  The scenes are those of tests/normal_icp_scenes.py and
tests/gicp_scenes.py; the fresh-context values are computed once per module and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import gicp_ref as gref
import gicp_scenes as gs
import helpers as h
import normal_icp_ref as nref
import normal_icp_scenes as sc
import sums_check as sums
from dcreg_amd import api
from test_gpu_frames_gicp import drive
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
PARAMS_5 = api.normal_params(k=5)
PARAMS_B = api.normal_params(k=5, search_radius=RADIUS)
SIZES = [1, 63, 64, 65, 255, 256, 257, 523]
SLOPE = 2.0                                  # the second engine's planted gates need it (normal_icp_scenes.GATE_SLOPES)
ENGINES = ["normals", "gicp"]
EMPTY3 = np.zeros((0, 3), np.float32)
THREE = sc.frozen(sc.sized_source(65)[:3].copy())     # a 3-point target: under the identity pose, three points of sized_source(65) sit on it
NAN3 = np.full((3, 3), np.nan, np.float32)


def lin_params(engine):
    p = api.default_lin_params(RADIUS, 1)
    if engine == "normals":
        p.weight_slope = SLOPE
    return p


# ---- the build batch of the kernel tests: target t = (points, normals as given); the planted map's normals are the engine's own
LOT, LATTICE, DUP, OUTSIDE, PLANT, SHORT, EMPTY = range(7)


@functools.lru_cache(maxsize=None)
def edge_targets(engine):
    L = gs.lot()
    cases = [gs.lattice_case(), gs.duplicate_case(), gs.outside_case()]
    plant = sc.gate_case() if engine == "normals" else gs.plant_case()
    tgts = [L["tgt"]] + [c["tgt"] for c in cases] + [plant["tgt"], THREE, EMPTY3]
    nrms = [L["nb"]] + [c["normals"] for c in cases] + [plant["normals"], NAN3, EMPTY3]
    return [np.ascontiguousarray(t, np.float32) for t in tgts], [np.ascontiguousarray(n, np.float32) for n in nrms]


@functools.lru_cache(maxsize=None)
def edge_sources(engine):
    """-> (sources, source normals, {name: source id}): the sized sources, then the cases' own"""
    cases = [gs.lattice_case(), gs.duplicate_case(), gs.outside_case()]
    plant = gs.plant_case() if engine == "gicp" else dict(sc.gate_case(), src_normals=sc.unit_normals(len(sc.GATE_SRC), 77))
    srcs = [sc.sized_source(n) for n in SIZES] + [c["src"] for c in cases] + [plant["src"]]
    nrms = [gs.sized_source_normals(n) for n in SIZES] + [c["src_normals"] for c in cases] + [plant["src_normals"]]
    ids = {n: i for i, n in enumerate(SIZES)}
    ids.update(lattice=len(SIZES), dup=len(SIZES) + 1, outside=len(SIZES) + 2, plant=len(SIZES) + 3)
    return [np.ascontiguousarray(s, np.float32) for s in srcs], [np.ascontiguousarray(n, np.float32) for n in nrms], ids


def edge_plan():
    """(source name, target, pose): different targets in unsorted order, the lot many times, a 1-point source beside the 523-point one"""
    W = sc.walk()
    I = np.eye(4)
    return [(523, LOT, W[0]), (1, LOT, W[0]), ("dup", DUP, I), (257, LOT, W[2]), ("plant", PLANT, I), (63, LOT, W[1]), ("lattice", LATTICE, I),
            (65, SHORT, I), (256, LOT, W[0]), ("outside", OUTSIDE, I), (523, LOT, W[3]), (64, LOT, W[2]), (255, LOT, W[1]), (65, LOT, W[0]),
            ("lattice", DUP, I), (257, LOT, W[0])]


_singles = {}


def single(engine, src_name, tgt, T):
    """linearize_normals / linearize_gicp on a fresh context with that target, those normals and that source: once, never modified"""
    k = (engine, src_name, tgt, np.asarray(T).tobytes())
    if k not in _singles:
        tgts, tn = edge_targets(engine)
        srcs, sn, ids = edge_sources(engine)
        c = api.Context(0)
        try:
            c.set_target(tgts[tgt], RADIUS)
            c.set_target_normals(tn[tgt])
            c.set_source(srcs[ids[src_name]])
            if engine == "gicp":
                c.set_source_normals(sn[ids[src_name]])
                _singles[k] = c.linearize_gicp(T, lin_params(engine))
            else:
                _singles[k] = c.linearize_normals(T, lin_params(engine))
        finally:
            c.close()
    return _singles[k]


# ---- 1. the kernels at block and target edges
@pytest.mark.parametrize("engine", ENGINES)
def test_a_launch_with_a_target_per_pose_is_bitwise_its_single_launches(engine):
    tgts, tn = edge_targets(engine)
    srcs, sn, ids = edge_sources(engine)
    plan = edge_plan()
    c = api.Context(0)                       # (a context that never had a target)
    try:
        c.pairs_sources_load(srcs)
        c.pairs_build(tgts, RADIUS)
        assert c.pairs_normals_kept() == 0
        c.pairs_normals_set(tn)
        assert c.pairs_normals_kept() == 1
        if engine == "gicp":
            c.pairs_sources_normals_set(sn)
        c.pairs_normals_reserve_slots(len(plan))
        batch = c.pairs_gicp_batch if engine == "gicp" else c.pairs_normals_batch
        sids, tids, Ts = [ids[s] for s, _, _ in plan], [t for _, t, _ in plan], [T for _, _, T in plan]
        n = len(plan)
        for state in (list(range(n)), None, [-1] * n, list(range(n))[::-1]):      # cold slots, no slots, another pair's words
            got = batch(Ts, sids, tids, state, lin_params(engine))
            assert len(got) == n
            for k, ((s, t, T), g) in enumerate(zip(plan, got)):
                sc.assert_sums_bitwise(g, single(engine, s, t, T), (engine, k, s, t))
        # the planted flags show in the counts; the 3-point target has no normals; the launch is not empty-handed
        planted = got[[s for s, _, _ in plan].index("plant")]
        assert (planted["n_eff"], planted["n_pt"]) == ((3, 6) if engine == "normals" else (2, 6))
        short = got[tids.index(SHORT)]
        assert short["n_eff"] == 0 and short["n_pt"] >= 3
        assert got[0]["n_eff"] >= 10 and got[1]["n_pt"] <= 1
        # one pose against the numpy reference: the counts exactly, every sum against its own terms
        L = gs.lot()
        s, t, T = plan[3]
        if engine == "gicp":
            want = gref.linearize(L["tgt"], L["nb"], sc.sized_source(s), gs.sized_source_normals(s), T, RADIUS, gs.EPS)
        else:
            want = nref.linearize(L["tgt"], L["nb"], sc.sized_source(s), T, RADIUS, weight_slope=SLOPE, use_weight_derivative=1)
        sc.assert_sums_close(got[3], want, "reference")
        sums.assert_sums_entrywise(got[3], want["row"], want["n_eff"], want["n_pt"], "reference")
        assert want["n_eff"] >= 10
    finally:
        c.close()


# ---- 2. the normals pass
@pytest.mark.parametrize("params", [PARAMS_5, PARAMS_B], ids=["unbounded", "bounded"])
def test_the_batch_normals_are_bitwise_normals_of_every_target_alone(params):
    tgts, _ = edge_targets("gicp")
    c, d = api.Context(0), api.Context(0)
    try:
        c.pairs_build(tgts, RADIUS)
        infos = c.pairs_normals_keep(params)
        assert c.pairs_normals_kept() == 1 and len(infos) == len(tgts)
        got = c.pairs_normals_get()
        off = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
        assert got.shape == (off[-1], 4)
        for t, tgt in enumerate(tgts):
            if len(tgt) == 0:
                assert infos[t] == {"n_in": 0, "n_finite": 0, "n_sparse": 0, "n_out": 0}
                continue
            nrm, cur, _, info = d.normals(tgt, params)
            assert infos[t] == info, t
            assert sc.same_bits(got[off[t]:off[t + 1], :3], nrm) and sc.same_bits(got[off[t]:off[t + 1], 3], cur), t
            # ... and therefore what keep_target_normals keeps
            d.set_target(tgt, RADIUS)
            assert d.keep_target_normals(params) == info, t
            kn, kc = d.kept_target_normals()
            assert sc.same_bits(got[off[t]:off[t + 1], :3], kn) and sc.same_bits(got[off[t]:off[t + 1], 3], kc), t
        assert np.isnan(got[off[SHORT]:off[SHORT + 1]]).all() and infos[SHORT]["n_out"] == 0 and infos[SHORT]["n_sparse"] == 3
        assert infos[LOT]["n_sparse"] == (1065 if params is PARAMS_B else 0) and infos[LOT]["n_out"] == 4000 - infos[LOT]["n_sparse"]
        assert infos[DUP]["n_out"] > 0
        # a build drops them
        c.pairs_build(tgts[:2], RADIUS)
        assert c.pairs_normals_kept() == 0
    finally:
        c.close(); d.close()


@pytest.mark.parametrize("params", [PARAMS_5, PARAMS_B], ids=["unbounded", "bounded"])
def test_the_pair_sources_normals_are_bitwise_the_source_form(params):
    srcs, _, _ = edge_sources("gicp")
    srcs = srcs[:len(SIZES)] + [EMPTY3, gs.lot()["src"]]
    c, d = api.Context(0), api.Context(0)
    try:
        c.pairs_sources_load(srcs)
        infos = c.pairs_sources_normals_keep(params)
        got = c.pairs_sources_normals_get()
        off = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
        d.set_target(gs.lot()["tgt"], RADIUS)
        for s, src in enumerate(srcs):
            if len(src) == 0:
                continue
            d.set_source(src)
            assert infos[s] == d.keep_source_normals(params), s
            wn, wc = d.kept_source_normals()
            assert sc.same_bits(got[off[s]:off[s + 1], :3], wn) and sc.same_bits(got[off[s]:off[s + 1], 3], wc), s
        assert infos[0]["n_out"] == 0 and infos[-1]["n_out"] > 0
    finally:
        c.close(); d.close()


# ---- 3. the engines
N_PAIRS = 16
# the rules of the parent suite's drive (test_gpu_frames_gicp): the map's normals bounded at the search radius, the frames' own k = 5 unbounded
TARGET_NORMALS, SOURCE_NORMALS = PARAMS_B, PARAMS_5
SHORT_PAIR, EMPTY_TGT_PAIR, EMPTY_SRC_PAIR, FAR_PAIR = 10, 11, 12, 13


@functools.lru_cache(maxsize=None)
def pairs_scene():
    """16 pairs from the frames of test_gpu_frames_gicp.drive(): six against the lot map itself, then every second point of it, a 12 m x 6 m
    crop, the map doubled, the map shifted 10 km with its pose, a 3-point target, an empty target, an empty source, a source started 1 km
    off, and two identical pairs"""
    L = gs.lot()
    frames, T0 = drive()
    live = [k for k, f in enumerate(frames) if len(f) >= 100 and abs(T0[k][0, 3] - L["INIT"][0, 3]) < 1.0][:12]
    lot = np.ascontiguousarray(L["tgt"], np.float32)
    mid_y = 0.5 * (lot[:, 1].min() + lot[:, 1].max())
    shift = np.array([10000.0, 0.0, 0.0])
    srcs, tgts, Ts = [], [], []
    for j in range(6):
        srcs.append(frames[live[j]]); tgts.append(lot); Ts.append(T0[live[j]])
    k = live[6]
    srcs.append(frames[k]); tgts.append(sc.frozen(lot[::2].copy())); Ts.append(T0[k])
    k = live[7]
    srcs.append(frames[k]); tgts.append(sc.frozen(lot[np.abs(lot[:, 1] - mid_y) <= 3.0].copy())); Ts.append(T0[k])
    k = live[8]
    srcs.append(frames[k]); tgts.append(sc.frozen(np.concatenate([lot, lot]))); Ts.append(T0[k])
    k = live[9]
    srcs.append(frames[k]); tgts.append(sc.frozen((lot.astype(np.float64) + shift).astype(np.float32))); Ts.append(sc.offset(T0[k], *shift))
    srcs.append(frames[live[10]]); tgts.append(THREE); Ts.append(np.eye(4))
    srcs.append(frames[live[10]]); tgts.append(EMPTY3); Ts.append(T0[live[10]])
    srcs.append(EMPTY3); tgts.append(lot); Ts.append(T0[live[10]])
    srcs.append(frames[live[11]]); tgts.append(lot); Ts.append(sc.offset(T0[live[11]], 1000.0, 0.0, 0.0))
    for _ in range(2):
        srcs.append(frames[live[0]]); tgts.append(lot); Ts.append(T0[live[1]])
    assert len(srcs) == N_PAIRS
    return srcs, tgts, [np.array(T) for T in Ts]


def engine_cfg():
    return cfg_pk01(use_weight_derivative=1)


def serial_record(c, engine, src, tgt, T0, method, cfg):
    """the sequence the calls promise, on context c"""
    if len(src) == 0 or len(tgt) == 0:
        return None
    c.set_target(tgt, cfg.search_radius)
    c.keep_target_normals(TARGET_NORMALS)
    c.set_source(src)
    if engine == "gicp":
        c.keep_source_normals(SOURCE_NORMALS)
        res, logs = c.icp_run_gicp(T0, method, cfg)
    else:
        res, logs = c.icp_run_normals(T0, method, cfg)
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    last = logs[-1] if logs else None
    return dict(T=T.reshape(16), iterations=res.iterations, converged=res.converged, status=res.status,
                rmse=last.rmse if last else 0.0, fitness=last.fitness if last else 0.0, corr=last.effective_points if last else 0,
                H=np.array(last.H_upper[:]) if last else np.zeros(21), mask=list(last.analysis.degenerate_mask[:]) if last else [0] * 6,
                trans_err=last.trans_error_vs_gt if last else None)


@functools.lru_cache(maxsize=None)
def serial_records(engine, method):
    srcs, tgts, Ts = pairs_scene()
    cfg = engine_cfg()
    c = api.Context(0)
    try:
        recs = [serial_record(c, engine, s, t, T, method, cfg) for s, t, T in zip(srcs, tgts, Ts)]
    finally:
        c.close()
    # not vacuous: registrations that converged after two or more iterations, and the status-1 cases
    done = [r for r in recs if r is not None and r["status"] == 0 and r["converged"] == 1 and r["iterations"] >= 2]
    print("%s %s: %d of %d pairs converged after two or more iterations" % (engine, method, len(done), N_PAIRS))
    assert len(done) >= 4
    assert (recs[SHORT_PAIR]["status"], recs[SHORT_PAIR]["iterations"], recs[SHORT_PAIR]["corr"]) == (1, 1, 0)
    assert (recs[FAR_PAIR]["status"], recs[FAR_PAIR]["iterations"]) == (1, 1)
    assert recs[EMPTY_TGT_PAIR] is None and recs[EMPTY_SRC_PAIR] is None
    return recs


def call(c, engine, srcs, tgts, Ts, method, cfg, slots):
    if engine == "gicp":
        return c.register_pairs_gicp(srcs, tgts, Ts, method, cfg, TARGET_NORMALS, SOURCE_NORMALS, slots=slots)
    return c.register_pairs_normals(srcs, tgts, Ts, method, cfg, TARGET_NORMALS, slots=slots)


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
            assert tr.trans_error_m == s["trans_err"], p


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("method", ["NONE", "Ours"])
@pytest.mark.parametrize("slots", [1, 3, 64])
def test_pairs_are_bitwise_the_serial_sequence(engine, method, slots):
    srcs, tgts, Ts = pairs_scene()
    want = serial_records(engine, method)
    c = api.Context(0)
    try:
        check(call(c, engine, srcs, tgts, Ts, method, engine_cfg(), slots), want)
        info = c.index_info()
        assert info.n_target == 0 and info.n_source == 0 and c.target_normals_kept() == 0 and c.source_normals_kept() == 0
    finally:
        c.close()


def planned_batches(c, tgts):
    off = np.concatenate([[0], np.cumsum([len(t) for t in tgts])]).astype(np.int64)
    ends, nb = (C.c_int32 * len(tgts))(), C.c_int(0)
    f = c._L.dcreg_pairs_plan_normals
    f.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int)]
    assert f(c._h, len(tgts), off.ctypes.data_as(C.POINTER(C.c_int64)), 3, ends, C.byref(nb)) == 0
    return nb.value


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("variant", ["three_batches", "permuted"])
def test_batches_and_order_do_not_change_a_record(engine, variant):
    srcs, tgts, Ts = pairs_scene()
    want = serial_records(engine, "Ours")
    c = api.Context(0)
    try:
        order = list(range(N_PAIRS))
        if variant == "three_batches":
            c.set_option("pairs_max_bytes", 6.5 * 4 * (1 << 24))      # six targets per build batch at the default table budget
            assert planned_batches(c, tgts) == 3
        else:
            order = [int(p) for p in np.random.default_rng(5).permutation(N_PAIRS)]
        recs = call(c, engine, [srcs[p] for p in order], [tgts[p] for p in order], [Ts[p] for p in order], "Ours", engine_cfg(), 5)
        check(recs, want, order)
    finally:
        c.close()


# ---- 4. the context is left alone
def test_the_context_is_left_alone():
    """own target, kept normals, source, kept source normals, loaded frames with kept frame normals and reserved slots: the same bits
    afterwards as on a control context"""
    L = gs.lot()
    W = sc.walk()
    srcs, tgts, Ts = pairs_scene()
    cfg = engine_cfg()
    frames = [L["src"], sc.sized_source(257)]
    fnormals = [L["mb"], gs.sized_source_normals(257)]
    prm = api.default_lin_params(RADIUS, 1)
    seq = {}
    for name in ("call", "control"):
        c = api.Context(0)
        try:
            c.set_target(L["tgt"], RADIUS)
            c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
            c.set_source(L["src"])
            c.set_source_normals(np.ascontiguousarray(L["mb"], np.float32))
            c.frames_load(frames)
            c.frames_normals_set(fnormals)
            c.normals_reserve_slots(2)
            c.reserve_warm_states(2)
            out = [c.linearize_normals(W[0], prm), c.linearize_gicp(W[0], prm)]
            out += c.gicp_batch([W[0], W[1]], [0, 1], [0, 1], prm)
            if name == "call":
                check(call(c, "normals", srcs[:8], tgts[:8], Ts[:8], "Ours", cfg, 3), serial_records("normals", "Ours")[:8])
                check(call(c, "gicp", srcs[:8], tgts[:8], Ts[:8], "Ours", cfg, 3), serial_records("gicp", "Ours")[:8])
            info = c.index_info()
            assert info.n_target == 4000 and info.n_source == 523
            assert c.target_normals_kept() == 1 and c.source_normals_kept() == 1 and c.frames_normals_kept() == 1
            out += [c.linearize_normals(W[1], prm), c.linearize_gicp(W[1], prm)]
            c.normals_reserve_slots(2)            # (the calls sized the warm slots for their own sources, as register_frames_gicp does)
            out += c.gicp_batch([W[1], W[2]], [0, 1], [0, 1], prm)
            recs = c.register_frames_gicp(frames, [W[0], W[0]], "Ours", cfg, PARAMS_5, slots=2)
            recs += c.register_pairs(srcs[:3], tgts[:3], Ts[:3], "Ours", cfg, slots=2)
            seq[name] = (out, [(r.iterations, r.status, r.converged, bytes(bytearray(r.final_transform)), r.final_rmse, r.corr_num,
                                bytes(bytearray(r.H_upper))) for r in recs])
        finally:
            c.close()
    for a, b in zip(seq["call"][0], seq["control"][0]):
        sc.assert_sums_bitwise(a, b)
    assert seq["call"][1] == seq["control"][1]


# ---- 5. refusals queue nothing
@pytest.mark.parametrize("engine", ENGINES)
def test_refusals_queue_nothing(engine):
    L = gs.lot()
    srcs, tgts, Ts = pairs_scene()
    srcs, tgts, Ts = srcs[:4], tgts[:4], Ts[:4]
    cfg = engine_cfg()
    want = serial_records(engine, "Ours")[:4]
    c = api.Context(0)
    try:
        c.set_target(L["tgt"], RADIUS)
        c.set_source(L["src"])
        before = c.launch_stats()["launches"]
        for which in ("source", "target"):
            bad_s, bad_t = [s.copy() for s in srcs], [t.copy() for t in tgts]
            (bad_s if which == "source" else bad_t)[2][5, 1] = np.nan
            with pytest.raises(api.DcregError, match=r"\(-\d+\).*non-finite"):
                call(c, engine, bad_s, bad_t, Ts, "Ours", cfg, 0)
        c.set_option("pairs_max_bytes", 1.0)                     # a NaN in a later build batch: refused before the first batch runs
        bad_t = [t.copy() for t in tgts]
        bad_t[3][0, 0] = np.inf
        with pytest.raises(api.DcregError, match="non-finite"):
            call(c, engine, srcs, bad_t, Ts, "Ours", cfg, 0)
        c.set_option("pairs_max_bytes", 0.0)
        # bad offsets and bad normal parameters through the C call
        s, t = np.concatenate(srcs[:3], 0), np.concatenate(tgts[:3], 0)
        soff = np.concatenate([[0], np.cumsum([len(x) for x in srcs[:3]])]).astype(np.int64)
        toff = np.concatenate([[0], np.cumsum([len(x) for x in tgts[:3]])]).astype(np.int64)

        def raw(so, to, tn, sn, n=3):
            T = np.asarray(Ts[:3], np.float64)
            R0, t0 = np.ascontiguousarray(T[:, :3, :3]).reshape(-1, 9), np.ascontiguousarray(T[:, :3, 3]).reshape(-1, 3)
            res = (api.TrialResult * 3)()
            fp, i64, dp = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_double)
            so, to = np.ascontiguousarray(so, np.int64), np.ascontiguousarray(to, np.int64)
            head = (c._h, n, s.ctypes.data_as(fp), so.ctypes.data_as(i64), t.ctypes.data_as(fp), to.ctypes.data_as(i64), 3)
            tail = (R0.ctypes.data_as(dp), t0.ctypes.data_as(dp), 0, 0, C.byref(cfg), 0, res)
            ref = lambda p: None if p is None else C.byref(p)
            if engine == "gicp":
                return c._L.dcreg_register_pairs_gicp(*head, ref(tn), ref(sn), *tail)
            return c._L.dcreg_register_pairs_normals(*head, ref(tn), *tail)

        for so, to in ((soff, [0, 40, 30, len(t)]), ([1, 40, 50, len(s)], toff), (soff, [5, 40, 50, len(t)])):
            assert raw(so, to, PARAMS_5, PARAMS_5) == api.E_INVALID
        bad = api.normal_params()
        bad.k = 2
        assert raw(soff, toff, bad, PARAMS_5) == api.E_INVALID and raw(soff, toff, None, PARAMS_5) == api.E_INVALID
        assert raw(soff, toff, bad, PARAMS_5, n=0) == api.E_INVALID              # checked before the empty call returns
        if engine == "gicp":
            assert raw(soff, toff, PARAMS_5, bad) == api.E_INVALID and raw(soff, toff, PARAMS_5, None, n=0) == api.E_INVALID
        assert raw(soff, toff, PARAMS_5, PARAMS_5, n=0) == 0
        assert c.launch_stats()["launches"] == before
        # a gated launch waiting, then a pending 1-NN batch slot
        prm = api.default_lin_params(RADIUS, 1)
        c.linearize_gated_begin(api.default_lin_params(RADIUS, 0), slot=0)
        with pytest.raises(api.DcregError, match=r"\(%d\)" % api.E_STATE):
            call(c, engine, srcs, tgts, Ts, "Ours", cfg, 0)
        c.gate_abort()
        c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
        n = c.normals_batch_begin([sc.walk()[0]], None, None, prm, slot=1)
        with pytest.raises(api.DcregError, match=r"\(%d\)" % api.E_STATE):
            call(c, engine, srcs, tgts, Ts, "Ours", cfg, 0)
        c.normals_batch_end(n, slot=1)
        info = c.index_info()
        assert info.n_target == 4000 and info.n_source == 523
        # a good call afterwards is still bitwise right
        check(call(c, engine, srcs, tgts, Ts, "Ours", cfg, 2), want)
    finally:
        c.close()


def test_the_seam_refuses_what_is_not_there():
    tgts, tn = edge_targets("gicp")
    srcs, sn, ids = edge_sources("gicp")
    W = sc.walk()
    prm = api.default_lin_params(RADIUS, 1)
    c = api.Context(0)
    try:
        def refused(code, text, f, *args):
            with pytest.raises(api.DcregError) as e:
                f(*args)
            assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)

        refused(api.E_STATE, "no pair batch built", c.pairs_normals_batch, [W[0]], [0], [0], None, prm)
        refused(api.E_STATE, "no pair batch built", c.pairs_normals_keep, PARAMS_5)
        c.pairs_build(tgts, RADIUS)
        refused(api.E_STATE, "no kept pair normals", c.pairs_normals_batch, [W[0]], [0], [0], None, prm)
        c.pairs_normals_set(tn)
        refused(api.E_STATE, "no pair sources", c.pairs_normals_batch, [W[0]], [0], [0], None, prm)
        c.pairs_sources_load(srcs)
        refused(api.E_STATE, "no kept pair source normals", c.pairs_gicp_batch, [W[0]], [0], [0], None, prm)
        c.pairs_sources_normals_set(sn)
        refused(api.E_INVALID, "pair target", c.pairs_gicp_batch, [W[0]], [0], [EMPTY], None, prm)
        refused(api.E_INVALID, "pair target", c.pairs_gicp_batch, [W[0]], [0], [len(tgts)], None, prm)
        refused(api.E_INVALID, "another search radius", c.pairs_gicp_batch, [W[0]], [0], [0], None, api.default_lin_params(0.7, 1))
        refused(api.E_INVALID, "warm slot", c.pairs_gicp_batch, [W[0]], [0], [0], [0], prm)                  # none reserved
        c.normals_reserve_slots(2, frames=False)
        c.pairs_normals_reserve_slots(2)
        with pytest.raises(api.DcregError, match="normals were given"):
            c.pairs_normals_set(np.concatenate(tn)[:-1])
        assert c.pairs_normals_kept() == 1
        sc.assert_sums_bitwise(c.pairs_gicp_batch([W[0]], [ids[523]], [LOT], [1], prm)[0], single("gicp", 523, LOT, W[0]))
    finally:
        c.close()
