"""The third engine's many-frames form on the device: the kept normals of loaded frames (dcreg_frames_normals_keep / _set), the batched
launch (dcreg_gicp_batch_begin / _end) against single launches of dcreg_linearize_gicp on fresh contexts, the warm slots and launch slots
it shares with the second engine, and the engines dcreg_register_frames_gicp / dcreg_icp_run_trials_gicp against the loop of
dcreg_set_source + dcreg_source_normals_keep + dcreg_icp_run_gicp - everything bitwise.  The scenes are those of tests/gicp_scenes.py
and tests/normal_icp_scenes.py; the fresh-context values are computed once per module and shared."""
import functools

import numpy as np
import pytest

import gicp_ref as gref
import gicp_scenes as gs
import helpers as h
import normal_icp_scenes as sc
import sums_check as sums
from dcreg_amd import api
from test_gpu_normals import OPTS_WINDOW
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = gs.RADIUS
PARAMS_5 = api.normal_params(k=5)
PARAMS_B = api.normal_params(k=5, search_radius=RADIUS)
SIZES = [1, 63, 64, 65, 255, 256, 257, 523]
EMPTY = 4                                   # the empty frame's place in edge_frames()


def lin_params(radius=RADIUS):
    return api.default_lin_params(radius, 1)


def context(src=None, src_normals=None, opts=(), keep=True):
    """the lot's map with its bounded normals kept"""
    L = gs.lot()
    c = api.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_target(L["tgt"], RADIUS)
    if src is not None:
        c.set_source(src)
    if keep:
        c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
    if src_normals is not None:
        c.set_source_normals(np.ascontiguousarray(src_normals, np.float32))
    return c


@functools.lru_cache(maxsize=None)
def edge_frames():
    """(frames, normals): sized_source(n) over the block edges with sized_source_normals(n), an empty frame in the middle"""
    fr = [sc.sized_source(n) for n in SIZES]
    nm = [gs.sized_source_normals(n) for n in SIZES]
    fr.insert(EMPTY, np.zeros((0, 3), np.float32))
    nm.insert(EMPTY, np.zeros((0, 3), np.float32))
    return fr, nm


def frame_of(n):
    i = SIZES.index(n)
    return i if i < EMPTY else i + 1


_singles = {}


def single(key, frame, normals, T):
    """set_source(frame) + set_source_normals(normals) + linearize_gicp(T) on a fresh context: once per (frame, pose), never modified"""
    k = (key, np.asarray(T).tobytes())
    if k not in _singles:
        c = context(frame, normals)
        try:
            _singles[k] = c.linearize_gicp(T, lin_params())
        finally:
            c.close()
    return _singles[k]


def single_edge(n, T):
    return single(n, sc.sized_source(n), gs.sized_source_normals(n), T)


def single_record(c, frame, T0, method, cfg, params=PARAMS_5):
    """the record the many-frames calls promise for one frame: set_source + keep_source_normals + icp_run_gicp"""
    if frame is not None:
        c.set_source(frame)
        c.keep_source_normals(params)
    res, logs = c.icp_run_gicp(T0, method, cfg)
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    last = logs[-1] if logs else None
    return dict(T=T.reshape(16), iterations=res.iterations, converged=res.converged, status=res.status,
                rmse=last.rmse if last else 0.0, fitness=last.fitness if last else 0.0, corr=last.effective_points if last else 0,
                H=np.array(last.H_upper[:]) if last else np.zeros(21), mask=list(last.analysis.degenerate_mask[:]) if last else [0] * 6,
                trans_err=last.trans_error_vs_gt if last else None)


PLAN_SIZES = [523, 1, 257, 63, 256, 523, 64, 255, 65, 257]
PLAN_POSES = [0, 0, 2, 1, 0, 3, 2, 1, 0, 0]                    # of the walk: the 523-point frame at two poses


# ---- 1. the kernel: the batched launch against single launches, at block edges
def test_a_batched_launch_is_bitwise_its_single_launches_at_block_edges():
    W = sc.walk()
    L = gs.lot()
    frames, normals = edge_frames()
    plan = [(n, W[p]) for n, p in zip(PLAN_SIZES, PLAN_POSES)]
    c = context()
    try:
        c.frames_load(frames)
        assert c.frames_normals_kept() == 0
        c.frames_normals_set(normals)
        assert c.frames_normals_kept() == 1
        c.normals_reserve_slots(len(plan))
        fids = [frame_of(n) for n, _ in plan]
        for ids in (list(range(len(plan))), [-1] * len(plan), list(range(len(plan)))[::-1]):     # cold slots, no slots, other frames' words
            got = c.gicp_batch([T for _, T in plan], ids, fids, lin_params())
            assert len(got) == len(plan)
            for k, ((n, T), g) in enumerate(zip(plan, got)):
                sc.assert_sums_bitwise(g, single_edge(n, T), (k, n))
        assert any(g["n_eff"] >= 10 for g in got) and got[1]["n_pt"] <= 1
        # one pose against the numpy reference, as the single launch is compared with it (tests/test_gpu_gicp.py): the counts exactly, the
        # sums to the tolerances of the exactly rounded reference sums - and the single launch's dump, whose sums these are, bitwise
        n, T = plan[2]
        want = gref.linearize(L["tgt"], L["nb"], sc.sized_source(n), gs.sized_source_normals(n), T, RADIUS, gs.EPS)
        sc.assert_sums_close(got[2], want, "reference")
        sums.assert_sums_entrywise(got[2], want["row"], want["n_eff"], want["n_pt"], "reference")      # every slot against its own terms
        assert all((want["flag"] == f).any() for f in (1, 2, 3))
        d = context(sc.sized_source(n), gs.sized_source_normals(n))
        try:
            dump = d.linearize_gicp(T, lin_params(), debug=True)
        finally:
            d.close()
        gs.assert_dump_bitwise(dump, want, "reference")
        sc.assert_sums_bitwise(got[2], dump, "dump")
    finally:
        c.close()


def test_the_planted_flags_run_as_a_frame():
    """flags 0, 1, 2, 3 and 5 in one frame, through frames_normals_set: the sums of the single launch"""
    S = gs.plant_case()
    c = api.Context(0)
    d = api.Context(0)
    try:
        for x in (c, d):
            x.set_target(S["tgt"], RADIUS)
            x.set_target_normals(S["normals"])
        d.set_source(S["src"])
        d.set_source_normals(S["src_normals"])
        want = d.linearize_gicp(S["T"], lin_params(), debug=True)
        assert list(want["flag"]) == gs.PLANT_FLAGS
        other = sc.sized_source(65)
        c.frames_load([other, S["src"]])
        c.frames_normals_set([gs.sized_source_normals(65), S["src_normals"]])
        c.normals_reserve_slots(1)
        for ids in ([0], [0], None):
            got = c.gicp_batch([S["T"]], ids, [1], lin_params())[0]
            sc.assert_sums_bitwise(got, want)
        assert got["n_eff"] == 2 and got["n_pt"] == 6
    finally:
        c.close(); d.close()


@pytest.mark.parametrize("params", [PARAMS_5, PARAMS_B], ids=["unbounded", "bounded"])
def test_frames_normals_keep_is_bitwise_the_source_form_per_frame(params):
    L = gs.lot()
    frames, _ = edge_frames()
    frames = frames + [L["src"]]
    c, d = context(), context()
    try:
        c.frames_load(frames)
        infos = c.frames_normals_keep(params)
        assert c.frames_normals_kept() == 1 and len(infos) == len(frames)
        live = [f for f in range(len(frames)) if f != EMPTY]
        got = {T: c.gicp_batch([L[T]] * len(live), None, live, lin_params()) for T in ("INIT", "GT")}
        for k, f in enumerate(live):
            d.set_source(frames[f])
            assert infos[f] == d.keep_source_normals(params), f
            # the kept frame normals are what the source form keeps: the same sums at two poses (at the truth nearly every point is
            # inside the radius, and its normal - or its lack of one - enters them), and - below - the same values
            for T in ("INIT", "GT"):
                sc.assert_sums_bitwise(got[T][k], d.linearize_gicp(L[T], lin_params()), (f, T))
        assert infos[EMPTY] == {"n_in": 0, "n_finite": 0, "n_sparse": 0, "n_out": 0}
        assert infos[0]["n_out"] == 0 and infos[0]["n_sparse"] == 1            # the 1-point frame: fewer than k points, no index
        assert infos[-1]["n_out"] > 0 and got["GT"][-1]["n_eff"] > 50 and got["GT"][-1]["n_pt"] > 400
        # the values themselves: normals_clouds is the pass behind frames_normals_keep, kept_source_normals what the source form keeps
        nrm, cur, off, infos2 = c.normals_clouds(frames, params)
        assert infos2 == infos
        for f, frame in enumerate(frames):
            if len(frame) == 0:
                continue
            d.set_source(frame)
            d.keep_source_normals(params)
            wn, wc = d.kept_source_normals()
            assert sc.same_bits(nrm[off[f]:off[f + 1]], wn) and sc.same_bits(cur[off[f]:off[f + 1]], wc), f
    finally:
        c.close(); d.close()


def test_the_own_source_form_is_bitwise_the_single_launch():
    """frame_ids = None: every pose linearises the context's own source with its kept source normals"""
    L = gs.lot()
    W = sc.walk()
    c = context(L["src"], L["mb"])
    try:
        c.normals_reserve_slots(3, frames=False)
        for ids in ([0, 1, 2], [2, 0, 1], None):
            got = c.gicp_batch([W[0], W[3], W[1]], ids, None, lin_params())
            for g, T in zip(got, (W[0], W[3], W[1])):
                sc.assert_sums_bitwise(g, single("lot", L["src"], L["mb"], T))
        assert got[0]["n_eff"] > 100
    finally:
        c.close()


# ---- 2. the seam
def test_refusals_queue_nothing():
    L = gs.lot()
    W = sc.walk()
    frames, normals = edge_frames()
    c = context(L["src"])
    try:
        def refused(code, text, *args, **kw):
            with pytest.raises(api.DcregError) as e:
                c.gicp_batch_begin(*args, **kw)
            assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)

        refused(api.E_STATE, "no kept source normals", [W[0]], None, None, lin_params())          # frame_ids == None: the own source's
        refused(api.E_STATE, "no frames", [W[0]], None, [0], lin_params())
        c.frames_load(frames)
        refused(api.E_STATE, "no kept frame normals", [W[0]], None, [0], lin_params())
        c.frames_normals_set(normals)
        c.normals_reserve_slots(4)
        for bad in (EMPTY, len(frames), -1):
            refused(api.E_INVALID, "frame", [W[0], W[0]], [0, 1], [0, bad], lin_params())
        for ids in ([0, 0], [0, 4]):
            refused(api.E_INVALID, "warm slot", [W[0], W[0]], ids, [0, 1], lin_params())
        for slot in (-1, 2):
            refused(api.E_INVALID, "slot", [W[0]], [0], [0], lin_params(), slot=slot)
        bad_pose = W[0].copy()
        bad_pose[1, 3] = np.inf
        refused(api.E_INVALID, "finite", [W[0], bad_pose], [0, 1], [0, 1], lin_params())
        for slot in (0, 1):
            with pytest.raises(api.DcregError) as e:
                c.gicp_batch_end(1, slot=slot)
            assert "(%d)" % api.E_STATE in str(e.value)                                           # nothing is in flight on either slot
        # frames_normals_set wants the load's point count; a refused call keeps what was kept
        with pytest.raises(api.DcregError) as e:
            c.frames_normals_set(np.concatenate(normals)[:-1])
        assert "(%d)" % api.E_INVALID in str(e.value) and c.frames_normals_kept() == 1
        assert c._L.dcreg_frames_normals_keep(c._h, None, None) == api.E_INVALID and c.frames_normals_kept() == 1      # null parameters
        # without kept MAP normals nothing runs either
        n = context(L["src"], keep=False)
        try:
            n.frames_load(frames)
            n.frames_normals_set(normals)
            with pytest.raises(api.DcregError) as e:
                n.gicp_batch_begin([W[0]], None, [0], lin_params())
            assert "(%d)" % api.E_STATE in str(e.value) and "no kept normals" in str(e.value)
        finally:
            n.close()
        # after all of that the slot takes a launch
        sc.assert_sums_bitwise(c.gicp_batch([W[0]], [0], [frame_of(523)], lin_params())[0], single_edge(523, W[0]))
        # a load drops the kept frame normals; so does the load a many-frames call performs
        c.frames_load(frames)
        assert c.frames_normals_kept() == 0
        refused(api.E_STATE, "no kept frame normals", [W[0]], None, [0], lin_params())
        c.frames_normals_set(normals)
        c.register_frames_normals(frames[:2], [W[0], W[0]], "NONE", cfg_pk01(max_iterations=1))
        assert c.frames_normals_kept() == 0
        assert c.source_normals_kept() == 0 and c.index_info().n_source == 523
    finally:
        c.close()


def test_both_launch_slots_in_flight_and_either_engine_refuses_the_other():
    L = gs.lot()
    W = sc.walk()
    frames = [L["src"], sc.sized_source(257), sc.sized_source(65)]
    normals = [L["mb"], gs.sized_source_normals(257), gs.sized_source_normals(65)]
    keys = ["lot", 257, 65]
    c = context(L["src"], L["mb"])
    only_n = context()
    try:
        before = c.linearize_gicp(W[1], lin_params())
        c.frames_load(frames)
        c.frames_normals_set(normals)
        c.normals_reserve_slots(5)
        set0 = [(0, W[0]), (1, W[2]), (2, W[1])]
        set1 = [(2, W[3]), (0, W[2])]
        n0 = c.gicp_batch_begin([T for _, T in set0], [0, 1, 2], [f for f, _ in set0], lin_params(), slot=0)
        n1 = c.gicp_batch_begin([T for _, T in set1], [3, 4], [f for f, _ in set1], lin_params(), slot=1)
        # while one is pending, the calls that queue work are refused and change nothing - the second engine's launch on the same slot among them
        for call in (lambda: c.set_source(frames[1]), lambda: c.linearize_gicp(W[1], lin_params()), lambda: c.set_target(L["tgt"], RADIUS),
                     lambda: c.gicp_batch_begin([W[0]], [0], [0], lin_params(), slot=1), lambda: c.normals_batch_begin([W[0]], [0], [0], lin_params(), slot=1),
                     lambda: c.frames_load(frames), lambda: c.frames_normals_keep(PARAMS_5), lambda: c.frames_normals_set(normals),
                     lambda: c.normals_clouds(frames), lambda: c.normals_reserve_slots(2)):
            with pytest.raises(api.DcregError) as e:
                call()
            assert "(%d)" % api.E_STATE in str(e.value)
        got0 = c.gicp_batch_end(n0, slot=0)
        with pytest.raises(api.DcregError) as e:                       # slot 1 is still pending
            c.set_source(frames[1])
        assert "(%d)" % api.E_STATE in str(e.value)
        got1 = c.gicp_batch_end(n1, slot=1)
        for got, plan in ((got0, set0), (got1, set1)):
            for g, (f, T) in zip(got, plan):
                sc.assert_sums_bitwise(g, single(keys[f], frames[f], normals[f], T), f)
        # the other way round: a pending launch of the second engine refuses this one, and the two share their slots' results correctly
        m0 = c.normals_batch_begin([W[0]], [0], [0], lin_params(), slot=0)
        with pytest.raises(api.DcregError) as e:
            c.gicp_batch_begin([W[0]], [1], [1], lin_params(), slot=0)
        assert "(%d)" % api.E_STATE in str(e.value)
        m1 = c.gicp_batch_begin([W[0]], [1], [1], lin_params(), slot=1)           # the other slot is free: both engines in flight together
        only_n.frames_load(frames)
        want_n = only_n.normals_batch([W[0]], None, [0], lin_params())[0]
        sc.assert_sums_bitwise(c.normals_batch_end(m0, slot=0)[0], want_n)
        sc.assert_sums_bitwise(c.gicp_batch_end(m1, slot=1)[0], single(257, frames[1], normals[1], W[0]))
        assert c.index_info().n_source == 523 and c.target_normals_kept() == 1 and c.source_normals_kept() == 1
        sc.assert_sums_bitwise(c.linearize_gicp(W[1], lin_params()), before)
    finally:
        c.close(); only_n.close()


# ---- 3. independence
def test_the_two_engines_share_warm_slots_and_neither_moves_the_other():
    """gicp_batch and normals_batch interleaved on the same warm slots: each bitwise a context that ran only one; linearize,
    linearize_normals and linearize_gicp of the own source do not move a bit"""
    L = gs.lot()
    W = sc.walk()
    frames = [L["src"], sc.sized_source(257)]
    normals = [L["mb"], gs.sized_source_normals(257)]
    prm1 = api.default_lin_params(RADIUS, 1)
    R, t = np.ascontiguousarray(W[1][:3, :3]).reshape(9), np.ascontiguousarray(W[1][:3, 3])

    def own(ctx):
        out = api.LinOut()
        ctx.linearize_raw(R, t, prm1, out)
        first = (np.array(out.H_upper[:]).tobytes(), np.array(out.g[:]).tobytes(), out.sum_r2, out.sum_b2, out.n_eff, out.n_pt)
        n, g = ctx.linearize_normals(W[1], lin_params()), ctx.linearize_gicp(W[1], lin_params())
        return first, tuple(np.asarray(n[k]).tobytes() for k in sc.SUM_KEYS), tuple(np.asarray(g[k]).tobytes() for k in sc.SUM_KEYS)

    both, only_g, only_n = context(L["src"], L["mb"]), context(), context()
    try:
        before = own(both)
        for x in (both, only_g, only_n):
            x.frames_load(frames)
            x.normals_reserve_slots(2)
        for x in (both, only_g):
            x.frames_normals_set(normals)
        for step, T in enumerate(W):
            poses, ids, fids = [T, W[(step + 2) % 5]], [step % 2, 1 - step % 2], [0, 1]
            g = both.gicp_batch(poses, ids, fids, lin_params())
            n = both.normals_batch(poses, ids[::-1], fids, lin_params())              # the words the other engine left, swapped
            g2 = both.gicp_batch(poses, ids, fids, lin_params())
            wg = only_g.gicp_batch(poses, ids, fids, lin_params())
            wn = only_n.normals_batch(poses, ids[::-1], fids, lin_params())
            for k in range(2):
                sc.assert_sums_bitwise(g[k], wg[k], (step, k))
                sc.assert_sums_bitwise(g2[k], wg[k], (step, k))
                sc.assert_sums_bitwise(n[k], wn[k], (step, k))
                sc.assert_sums_bitwise(g[k], single(("lot", 257)[k], frames[k], normals[k], poses[k]), (step, k))
        assert own(both) == before
    finally:
        both.close(); only_g.close(); only_n.close()


def test_an_active_window_index_stays_active_and_invisible():
    L = gs.lot()
    W = sc.walk()
    c = context(L["src"], L["mb"], opts=OPTS_WINDOW)
    try:
        sc.assert_sums_bitwise(c.linearize_gicp(W[0], lin_params()), single("lot", L["src"], L["mb"], W[0]))
        info = c.roi_info()
        assert info["active"]
        c.normals_reserve_slots(2, frames=False)
        for ids in ([0, 1], [1, 0]):
            got = c.gicp_batch([W[1], W[3]], ids, None, lin_params())             # W[3] lies outside the window's box
            sc.assert_sums_bitwise(got[0], single("lot", L["src"], L["mb"], W[1]))
            sc.assert_sums_bitwise(got[1], single("lot", L["src"], L["mb"], W[3]))
        frames, T0 = drive()
        want = drive_singles("Ours")[:6]
        recs = c.register_frames_gicp(frames[:6], T0[:6], "Ours", cfg_pk01(use_weight_derivative=1), PARAMS_5, slots=2)
        for k, (tr, s) in enumerate(zip(recs, want)):
            h.assert_record(tr, s, k)
        after = c.roi_info()
        assert after["active"] and after["windows_built"] == info["windows_built"]
        sc.assert_sums_bitwise(c.linearize_gicp(W[1], lin_params()), single("lot", L["src"], L["mb"], W[1]))
        assert c.roi_info()["windows_built"] == info["windows_built"]
    finally:
        c.close()


# ---- 4. the engine, frames
N_FRAMES, EMPTY_FRAME, ONE_FRAME, FAR_FRAME = 70, 33, 12, 51


@functools.lru_cache(maxsize=None)
def drive():
    """70 frames of a few hundred points cut from the lot - the lot frame and sized sources moved by seeded small offsets, one empty, one
    of a single point, one started 1 km outside the map - and their start poses near INIT"""
    L = gs.lot()
    rng = np.random.default_rng(17)
    sizes = [523, 300, 257, 256, 255, 400, 129, 200, 333, 150]
    frames, T0 = [], []
    for k in range(N_FRAMES):
        n = 1 if k == ONE_FRAME else sizes[k % len(sizes)]
        base = L["src"] if n == 523 else sc.sized_source(n)
        f = (base + rng.normal(0.0, 0.01, 3).astype(np.float32)).astype(np.float32)
        frames.append(np.zeros((0, 3), np.float32) if k == EMPTY_FRAME else sc.frozen(f))
        T0.append(sc.offset(L["INIT"], *rng.uniform(-0.05, 0.05, 3), yaw=rng.uniform(-0.01, 0.01)))
    T0[FAR_FRAME] = sc.offset(T0[FAR_FRAME], 1000.0, 0.0, 0.0)
    return frames, T0


@functools.lru_cache(maxsize=None)
def drive_singles(method):
    frames, T0 = drive()
    cfg = cfg_pk01(use_weight_derivative=1)
    c = context()
    try:
        return [None if len(f) == 0 else single_record(c, f, T, method, cfg) for f, T in zip(frames, T0)]
    finally:
        c.close()


@pytest.mark.parametrize("method", ["NONE", "Ours"])
@pytest.mark.parametrize("slots", [1, 3, 64])
def test_frames_are_bitwise_the_loop_of_single_registrations(method, slots):
    frames, T0 = drive()
    cfg = cfg_pk01(use_weight_derivative=1)
    want = drive_singles(method)
    c = context()
    try:
        recs = c.register_frames_gicp(frames, T0, method, cfg, PARAMS_5, slots=slots)
        assert len(recs) == N_FRAMES
        for k, (tr, s) in enumerate(zip(recs, want)):
            if s is None:
                assert (tr.status, tr.iterations, tr.converged) == (3, 0, 0), k
                continue
            h.assert_record(tr, s, (k, len(frames[k])))
            if s["trans_err"] is not None and tr.status == 0:
                assert tr.trans_error_m == s["trans_err"], k
        # not vacuous: registrations that converged after two or more iterations, aborts with status 1 (the frame outside the map; the
        # 1-point frame, none of whose points has a normal) and the empty frame's status 3
        assert recs[FAR_FRAME].status == 1 and recs[FAR_FRAME].iterations == 1
        assert (recs[ONE_FRAME].status, recs[ONE_FRAME].iterations, recs[ONE_FRAME].corr_num) == (1, 1, 0)
        assert recs[EMPTY_FRAME].status == 3
        done = [tr for tr in recs if tr.status == 0 and tr.converged == 1 and tr.iterations >= 2]
        print("%s, %d slots: %d of %d frames converged after two or more iterations (at most %d)" % (method, slots, len(done), N_FRAMES, max(tr.iterations for tr in recs)))
        assert len(done) > 0
        assert c.index_info().n_source == 0 and c.target_normals_kept() == 1 and c.source_normals_kept() == 0
        assert c.frames_normals_kept() == 1
    finally:
        c.close()


# ---- 5. the engine, trials
def test_trials_are_bitwise_single_runs():
    L = gs.lot()
    rng = np.random.default_rng(11)
    T0 = [sc.offset(L["INIT"], *rng.uniform(-0.08, 0.08, 3), yaw=rng.uniform(-0.02, 0.02)) for _ in range(40)]
    cfg = cfg_pk01(use_weight_derivative=1)
    c, d = context(L["src"]), context(L["src"])
    try:
        with pytest.raises(api.DcregError) as e:                       # no kept source normals yet
            c.icp_run_trials_gicp(T0, "Ours", cfg)
        assert "(%d)" % api.E_STATE in str(e.value) and "no kept source normals" in str(e.value)
        c.keep_source_normals(PARAMS_5)
        d.keep_source_normals(PARAMS_5)
        recs = c.icp_run_trials_gicp(T0, "Ours", cfg)
        assert len(recs) == 40
        for k, (tr, T) in enumerate(zip(recs, T0)):
            h.assert_record(tr, single_record(d, None, T, "Ours", cfg), k)
        assert all(tr.status == 0 for tr in recs) and max(tr.iterations for tr in recs) > 2
        assert c.icp_run_trials_gicp(np.zeros((0, 4, 4)), "Ours", cfg) == []
        assert c.source_normals_kept() == 1 and c.index_info().n_source == 523
    finally:
        c.close(); d.close()


# ---- 6. nothing else moves
def test_the_call_leaves_the_context_alone():
    L = gs.lot()
    W = sc.walk()
    frames, T0 = drive()
    frames, T0 = frames[:12], T0[:12]
    cfg = cfg_pk01(use_weight_derivative=1)
    prm1 = api.default_lin_params(RADIUS, 1)
    R, t = np.ascontiguousarray(W[1][:3, :3]).reshape(9), np.ascontiguousarray(W[1][:3, 3])

    def first_engine(ctx):
        out = api.LinOut()
        ctx.linearize_raw(R, t, prm1, out)
        return np.array(out.H_upper[:]).tobytes(), np.array(out.g[:]).tobytes(), out.sum_r2, out.sum_b2, out.n_eff, out.n_pt

    c, fresh = context(L["src"], L["mb"]), context(L["src"], L["mb"])
    try:
        c.linearize_gicp(W[0], lin_params())                           # the own warm words now hold the positions of W[0]
        lin0 = first_engine(c)
        recs = c.register_frames_gicp(frames, T0, "Ours", cfg, PARAMS_5, slots=4)
        assert sum(tr.status == 0 for tr in recs) > 6 and max(tr.iterations for tr in recs) > 2
        # a pose near the last one: it reads the own warm words, which the call must not have touched
        sc.assert_sums_bitwise(c.linearize_gicp(W[1], lin_params()), single("lot", L["src"], L["mb"], W[1]))
        sc.assert_sums_bitwise(c.linearize_normals(W[1], lin_params()), fresh.linearize_normals(W[1], lin_params()))
        assert first_engine(c) == lin0 == first_engine(fresh)
        assert c.index_info().n_source == 523 and c.target_normals_kept() == 1 and c.source_normals_kept() == 1
        assert sc.same_bits(c.kept_source_normals()[0], L["mb"])
        # the other engines' many-frames calls after it, on the same frames: what they give on a fresh context - and this one again
        for name in ("register_frames", "register_frames_normals"):
            a = getattr(c, name)(frames, T0, "Ours", cfg, slots=4)
            b = getattr(fresh, name)(frames, T0, "Ours", cfg, slots=4)
            for x, y in zip(a, b):
                assert (x.iterations, x.converged, x.status, x.corr_num) == (y.iterations, y.converged, y.status, y.corr_num)
                assert np.array_equal(np.array(x.final_transform[:]), np.array(y.final_transform[:])) and np.array_equal(np.array(x.H_upper[:]), np.array(y.H_upper[:]))
        again = c.register_frames_gicp(frames, T0, "Ours", cfg, PARAMS_5, slots=4)
        for x, y in zip(again, recs):
            assert (x.iterations, x.converged, x.status, x.corr_num) == (y.iterations, y.converged, y.status, y.corr_num)
            assert np.array_equal(np.array(x.final_transform[:]), np.array(y.final_transform[:])) and np.array_equal(np.array(x.H_upper[:]), np.array(y.H_upper[:]))
    finally:
        c.close(); fresh.close()


# ---- 7. state refusals of the engine
def test_without_kept_map_normals_nothing_runs():
    frames, T0 = drive()
    frames, T0 = frames[:4], T0[:4]
    cfg = cfg_pk01()
    L = gs.lot()
    c = context(L["src"], keep=False)
    try:
        with pytest.raises(api.DcregError) as e:
            c.register_frames_gicp(frames, T0, "Ours", cfg)
        assert "(%d)" % api.E_STATE in str(e.value) and "no kept normals" in str(e.value)
        with pytest.raises(api.DcregError) as e:
            c.icp_run_trials_gicp(T0, "Ours", cfg)
        assert "(%d)" % api.E_STATE in str(e.value)
        bare = api.Context(0)
        try:
            with pytest.raises(api.DcregError) as e:
                bare.register_frames_gicp(frames, T0, "Ours", cfg)
            assert "(%d)" % api.E_STATE in str(e.value) and "target" in str(e.value)
        finally:
            bare.close()
        # all frames empty: nothing to estimate, every record status 3
        c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
        recs = c.register_frames_gicp([np.zeros((0, 3), np.float32)] * 3, T0[:3], "Ours", cfg)
        assert [r.status for r in recs] == [3, 3, 3]
    finally:
        c.close()
