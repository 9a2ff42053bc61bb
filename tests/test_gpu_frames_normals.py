"""The second engine's many-frames form on the device: the batched launch (dcreg_normals_batch_begin / _end) against single launches of
dcreg_linearize_normals on fresh contexts, the warm slots, the two launch slots, and the engines dcreg_register_frames_normals /
dcreg_icp_run_trials_normals against the loop of dcreg_set_source + dcreg_icp_run_normals - everything bitwise.  The scenes are those of
tests/normal_icp_scenes.py; the fresh-context values are computed once per module and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as h
import normal_icp_ref as ref
import normal_icp_scenes as sc
import sums_check as sums
from dcreg_amd import api
from test_gpu_normals import OPTS_WINDOW
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
PARAMS_B = api.normal_params(k=5, search_radius=RADIUS)
SIZES = [1, 63, 64, 65, 255, 256, 257, 523]
EMPTY = 4                                   # the empty frame's place in the set of test 1
RECORD = ("final_transform", "iterations", "converged", "status", "final_rmse", "final_fitness", "corr_num", "H_upper", "degenerate_mask")


def lin_params(radius=RADIUS, wd=1):
    return api.default_lin_params(radius, wd)


def context(src=None, keep=True):
    L = sc.lot()
    c = api.Context(0)
    c.set_target(L["tgt"], RADIUS)
    if src is not None:
        c.set_source(src)
    if keep:
        c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
    return c


@functools.lru_cache(maxsize=None)
def edge_frames():
    """sized_source(n) over the block edges, with an empty frame in the middle"""
    fr = [sc.sized_source(n) for n in SIZES]
    fr.insert(EMPTY, np.zeros((0, 3), np.float32))
    return fr


def frame_of(n):
    """index in edge_frames() of the frame with n points"""
    i = SIZES.index(n)
    return i if i < EMPTY else i + 1


_singles = {}


def single(frame_key, frame, T):
    """set_source(frame) + linearize_normals(T) on a fresh context: computed once per (frame, pose), never modified"""
    key = (frame_key, np.asarray(T).tobytes())
    if key not in _singles:
        c = context(frame)
        try:
            _singles[key] = c.linearize_normals(T, lin_params())
        finally:
            c.close()
    return _singles[key]


def bits(tr):
    """the record fields the call promises, as bytes"""
    out = []
    for k in RECORD:
        v = getattr(tr, k)
        out.append(np.array(v[:] if hasattr(v, "__len__") else v).tobytes())
    return tuple(out)


def single_record(c, frame, T0, method, cfg):
    """the record the many-frames calls promise for one frame: set_source + icp_run_normals"""
    if frame is not None:
        c.set_source(frame)
    res, logs = c.icp_run_normals(T0, method, cfg)
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    last = logs[-1] if logs else None
    return dict(T=T.reshape(16), iterations=res.iterations, converged=res.converged, status=res.status,
                rmse=last.rmse if last else 0.0, fitness=last.fitness if last else 0.0, corr=last.effective_points if last else 0,
                H=np.array(last.H_upper[:]) if last else np.zeros(21), mask=list(last.analysis.degenerate_mask[:]) if last else [0] * 6,
                trans_err=last.trans_error_vs_gt if last else None)


# ---- 1. the batched launch against single launches, at block edges
def test_a_batched_launch_is_bitwise_its_single_launches_at_block_edges():
    W = sc.walk()
    frames = edge_frames()
    # ten poses: not in frame order, the 523-point frame twice at two poses of the walk
    plan = [(523, W[0]), (1, W[0]), (257, W[2]), (63, W[1]), (256, W[0]), (523, W[3]), (64, W[2]), (255, W[1]), (65, W[0]), (257, W[0])]
    c = context()
    try:
        c.frames_load(frames)
        c.normals_reserve_slots(len(plan))
        fids = [frame_of(n) for n, _ in plan]
        for ids in (list(range(len(plan))), [-1] * len(plan), list(range(len(plan)))[::-1]):     # cold slots, no slots, other frames' words
            got = c.normals_batch([T for _, T in plan], ids, fids, lin_params())
            assert len(got) == len(plan)
            for k, ((n, T), g) in enumerate(zip(plan, got)):
                sc.assert_sums_bitwise(g, single(n, sc.sized_source(n), T), (k, n))
        assert any(g["n_eff"] >= 10 for g in got) and got[1]["n_pt"] <= 1
        # one pose against the numpy reference, as the single launch is compared with it (tests/test_gpu_normal_icp.py): the counts exactly,
        # the sums to the tolerances of the exactly rounded reference sums, and every slot against its own terms
        n, T = plan[2]
        L = sc.lot()
        want = ref.linearize(L["tgt"], L["nb"], sc.sized_source(n), T, RADIUS, use_weight_derivative=1)
        assert want["n_eff"] >= 10
        sc.assert_sums_close(got[2], want, "reference")
        sums.assert_sums_entrywise(got[2], want["row"], want["n_eff"], want["n_pt"], "reference")
        # naming the empty frame (or one that is not there): refused, nothing queued - the next begin on the same slot is accepted
        for bad in (EMPTY, len(frames), -1):
            with pytest.raises(api.DcregError) as e:
                c.normals_batch_begin([W[0], W[0]], [0, 1], [0, bad], lin_params())
            assert "(%d)" % api.E_INVALID in str(e.value)
        with pytest.raises(api.DcregError) as e:
            c.normals_batch_end(2)
        assert "(%d)" % api.E_STATE in str(e.value)                                              # nothing is in flight
        for ids in ([0, 0], [0, len(plan)]):                                                     # a slot twice, a slot that was not reserved
            with pytest.raises(api.DcregError) as e:
                c.normals_batch_begin([W[0], W[0]], ids, [0, 1], lin_params())
            assert "(%d)" % api.E_INVALID in str(e.value)
        for slot in (-1, 2):
            with pytest.raises(api.DcregError) as e:
                c.normals_batch_begin([W[0]], [0], [0], lin_params(), slot=slot)
            assert "(%d)" % api.E_INVALID in str(e.value)
        bad_pose = W[0].copy()
        bad_pose[1, 3] = np.inf
        with pytest.raises(api.DcregError) as e:
            c.normals_batch_begin([W[0], bad_pose], [0, 1], [0, 1], lin_params())
        assert "(%d)" % api.E_INVALID in str(e.value)
        again = c.normals_batch([plan[0][1]], [0], [fids[0]], lin_params())
        sc.assert_sums_bitwise(again[0], single(523, sc.sized_source(523), plan[0][1]))
    finally:
        c.close()


# ---- 2. warm slots decide nothing
def test_warm_slots_only_bound_the_search():
    L = sc.lot()
    W = sc.walk()
    other = sc.sized_source(257)
    c = context()
    try:
        c.frames_load([L["src"], other])
        c.normals_reserve_slots(2)
        for step, T in enumerate(W):                      # a small step, halfway, a jump of many cells, the way back
            want = single("lot", L["src"], T)
            warm = c.normals_batch([T], [0], [0], lin_params())[0]
            cold = c.normals_batch([T], [-1], [0], lin_params())[0]
            none = c.normals_batch([T], None, [0], lin_params())[0]
            for g in (warm, cold, none):
                sc.assert_sums_bitwise(g, want, step)
        c.normals_reset_slot(0)
        sc.assert_sums_bitwise(c.normals_batch([W[1]], [0], [0], lin_params())[0], single("lot", L["src"], W[1]), "after reset")
        # two frames swap their slots between launches without a reset: a stale position from another frame is only a bound
        a = c.normals_batch([W[0], W[2]], [0, 1], [0, 1], lin_params())
        b = c.normals_batch([W[1], W[3]], [1, 0], [0, 1], lin_params())
        d = c.normals_batch([W[3], W[0]], [0, 1], [0, 1], lin_params())
        for got, poses in ((a, (W[0], W[2])), (b, (W[1], W[3])), (d, (W[3], W[0]))):
            sc.assert_sums_bitwise(got[0], single("lot", L["src"], poses[0]), "swap")
            sc.assert_sums_bitwise(got[1], single(257, other, poses[1]), "swap")
    finally:
        c.close()


def test_the_own_source_form_is_bitwise_the_single_launch():
    """frame_ids = None: every pose linearises the context's own source"""
    L = sc.lot()
    W = sc.walk()
    c = context(L["src"])
    try:
        c.normals_reserve_slots(3, frames=False)
        for ids in ([0, 1, 2], [2, 0, 1], None):
            got = c.normals_batch([W[0], W[3], W[1]], ids, None, lin_params())
            for g, T in zip(got, (W[0], W[3], W[1])):
                sc.assert_sums_bitwise(g, single("lot", L["src"], T))
        # slots reserved for the own source do not serve frames
        c.frames_load([L["src"]])
        with pytest.raises(api.DcregError) as e:
            c.normals_batch_begin([W[0]], [0], [0], lin_params())
        assert "(%d)" % api.E_INVALID in str(e.value)
    finally:
        c.close()


# ---- 3. both launch slots in flight
def test_both_launch_slots_in_flight():
    L = sc.lot()
    W = sc.walk()
    frames = [L["src"], sc.sized_source(257), sc.sized_source(65)]
    keys = ["lot", 257, 65]
    c = context(L["src"])
    try:
        before = c.linearize_normals(W[1], lin_params())
        c.frames_load(frames)
        c.normals_reserve_slots(5)
        set0 = [(0, W[0]), (1, W[2]), (2, W[1])]
        set1 = [(2, W[3]), (0, W[2])]
        n0 = c.normals_batch_begin([T for _, T in set0], [0, 1, 2], [f for f, _ in set0], lin_params(), slot=0)
        n1 = c.normals_batch_begin([T for _, T in set1], [3, 4], [f for f, _ in set1], lin_params(), slot=1)
        # while one is pending, the calls that queue work are refused and change nothing
        for call in (lambda: c.set_source(frames[1]), lambda: c.linearize_normals(W[1], lin_params()), lambda: c.set_target(L["tgt"], RADIUS),
                     lambda: c.normals_batch_begin([W[0]], [0], [0], lin_params(), slot=1), lambda: c.frames_load(frames),
                     lambda: c.normals_reserve_slots(2)):
            with pytest.raises(api.DcregError) as e:
                call()
            assert "(%d)" % api.E_STATE in str(e.value)
        got0 = c.normals_batch_end(n0, slot=0)
        with pytest.raises(api.DcregError) as e:                       # slot 1 is still pending
            c.set_source(frames[1])
        assert "(%d)" % api.E_STATE in str(e.value)
        got1 = c.normals_batch_end(n1, slot=1)
        for got, plan in ((got0, set0), (got1, set1)):
            for g, (f, T) in zip(got, plan):
                sc.assert_sums_bitwise(g, single(keys[f], frames[f], T), f)
        assert c.index_info().n_source == 523 and c.target_normals_kept() == 1
        sc.assert_sums_bitwise(c.linearize_normals(W[1], lin_params()), before)
    finally:
        c.close()


# ---- 4. the engine, frames
N_FRAMES, EMPTY_FRAME, FAR_FRAME = 70, 33, 51


@functools.lru_cache(maxsize=None)
def drive():
    """70 frames - the lot frame and sized sources moved by seeded small offsets, one empty, one started 1 km outside the map - and their
    start poses near INIT"""
    L = sc.lot()
    rng = np.random.default_rng(7)
    sizes = [523, 1, 63, 64, 65, 255, 256, 257, 300, 100]
    frames, T0 = [], []
    for k in range(N_FRAMES):
        n = sizes[k % len(sizes)]
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
        recs = c.register_frames_normals(frames, T0, method, cfg, slots=slots)
        assert len(recs) == N_FRAMES
        for k, (tr, s) in enumerate(zip(recs, want)):
            if s is None:
                assert (tr.status, tr.iterations, tr.converged) == (3, 0, 0), k
                continue
            h.assert_record(tr, s, (k, len(frames[k])))
            if s["trans_err"] is not None and tr.status == 0:
                assert tr.trans_error_m == s["trans_err"], k
        assert recs[FAR_FRAME].status == 1 and recs[FAR_FRAME].iterations == 1
        assert sum(tr.status == 0 for tr in recs) > N_FRAMES // 2 and max(tr.iterations for tr in recs) > 2
        assert c.index_info().n_source == 0 and c.target_normals_kept() == 1
    finally:
        c.close()


# ---- 5. the engine, trials
def test_trials_are_bitwise_single_runs():
    L = sc.lot()
    rng = np.random.default_rng(11)
    T0 = [sc.offset(L["INIT"], *rng.uniform(-0.08, 0.08, 3), yaw=rng.uniform(-0.02, 0.02)) for _ in range(40)]
    cfg = cfg_pk01(use_weight_derivative=1)
    c, d = context(L["src"]), context(L["src"])
    try:
        recs = c.icp_run_trials_normals(T0, "Ours", cfg)
        assert len(recs) == 40
        for k, (tr, T) in enumerate(zip(recs, T0)):
            h.assert_record(tr, single_record(d, None, T, "Ours", cfg), k)
        assert all(tr.status == 0 for tr in recs) and max(tr.iterations for tr in recs) > 2
        assert c.icp_run_trials_normals(np.zeros((0, 4, 4)), "Ours", cfg) == []
    finally:
        c.close(); d.close()


# ---- 6. nothing else moves
def test_the_call_leaves_the_context_alone():
    L = sc.lot()
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

    c, fresh = context(L["src"]), context(L["src"])
    try:
        c.linearize_normals(W[0], lin_params())                        # the own warm words now hold the positions of W[0]
        lin0 = first_engine(c)
        recs = c.register_frames_normals(frames, T0, "Ours", cfg, slots=4)
        assert sum(tr.status == 0 for tr in recs) > 6 and max(tr.iterations for tr in recs) > 2
        # a pose near the last one: it reads the own warm words, which the call must not have touched
        sc.assert_sums_bitwise(c.linearize_normals(W[1], lin_params()), single("lot", L["src"], W[1]))
        assert first_engine(c) == lin0 == first_engine(fresh)
        assert c.index_info().n_source == 523 and c.target_normals_kept() == 1
        # the first engine's many-frames call after it, on the same frames: what it gives on a fresh context
        a = c.register_frames(frames, T0, "Ours", cfg, slots=4)
        b = fresh.register_frames(frames, T0, "Ours", cfg, slots=4)
        assert [bits(x) for x in a] == [bits(x) for x in b]
        # ... and the other way round
        again = c.register_frames_normals(frames, T0, "Ours", cfg, slots=4)
        assert [bits(x) for x in again] == [bits(x) for x in recs]
        assert c.target_normals_kept() == 1
    finally:
        c.close(); fresh.close()


def test_an_active_window_index_stays_active_and_invisible():
    """a capped map whose single-pose launches search the window: the batched launches and the engine search the whole map's index where
    it is kept meanwhile - same bits, no swap, no rebuild, and the own warm words (the window's positions) still serve"""
    L = sc.lot()
    W = sc.walk()
    frames, T0 = drive()
    frames, T0 = frames[:6], T0[:6]
    cfg = cfg_pk01(use_weight_derivative=1)
    want = drive_singles("Ours")[:6]
    c = api.Context(0)
    try:
        for k, v in OPTS_WINDOW:
            c.set_option(k, v)
        c.set_target(L["tgt"], RADIUS)
        c.set_source(L["src"])
        c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
        sc.assert_sums_bitwise(c.linearize_normals(W[0], lin_params()), single("lot", L["src"], W[0]))
        info = c.roi_info()
        assert info["active"]
        c.normals_reserve_slots(2, frames=False)
        for ids in ([0, 1], [1, 0]):
            got = c.normals_batch([W[1], W[3]], ids, None, lin_params())          # W[3] lies outside the window's box
            sc.assert_sums_bitwise(got[0], single("lot", L["src"], W[1]))
            sc.assert_sums_bitwise(got[1], single("lot", L["src"], W[3]))
        recs = c.register_frames_normals(frames, T0, "Ours", cfg, slots=2)
        for k, (tr, s) in enumerate(zip(recs, want)):
            h.assert_record(tr, s, k)
        after = c.roi_info()
        assert after["active"] and after["windows_built"] == info["windows_built"]
        sc.assert_sums_bitwise(c.linearize_normals(W[1], lin_params()), single("lot", L["src"], W[1]))
        assert c.roi_info()["windows_built"] == info["windows_built"]
    finally:
        c.close()


# ---- 7. state refusals
def test_without_kept_normals_nothing_runs():
    L = sc.lot()
    frames, T0 = drive()
    frames, T0 = frames[:4], T0[:4]
    cfg = cfg_pk01()
    Lib = api.load()
    c = context(L["src"], keep=False)
    try:
        def refused():
            assert c.target_normals_kept() == 0
            with pytest.raises(api.DcregError) as e:
                c.register_frames_normals(frames, T0, "Ours", cfg)
            assert "(%d)" % api.E_STATE in str(e.value) and "no kept normals" in str(e.value)
            with pytest.raises(api.DcregError) as e:
                c.icp_run_trials_normals(T0, "Ours", cfg)
            assert "(%d)" % api.E_STATE in str(e.value)
            # the records are left as they were
            res = (api.TrialResult * 4)()
            for r in res:
                r.iterations, r.status, r.final_rmse = 77, 9, 1.5
            xyz = np.ascontiguousarray(np.concatenate(frames, 0))
            off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
            R0 = np.ascontiguousarray(np.array(T0)[:, :3, :3]).reshape(4, 9)
            t0 = np.ascontiguousarray(np.array(T0)[:, :3, 3]).reshape(4, 3)
            rc = Lib.dcreg_register_frames_normals(c._h, 4, xyz.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)), 3,
                                                   api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), 0, res)
            assert rc == api.E_STATE and all((r.iterations, r.status, r.final_rmse) == (77, 9, 1.5) for r in res)
        refused()                                                      # nothing kept yet
        for change in (lambda: c.insert_source(L["GT"], 0.05), lambda: c.crop(L["tgt"].min(axis=0) + 1.0, L["tgt"].max(axis=0) - 1.0),
                       lambda: c.set_target(L["tgt"], RADIUS)):
            c.keep_target_normals(PARAMS_B)
            assert c.register_frames_normals(frames, T0, "Ours", cfg)[0].iterations > 0
            change()
            refused()
        bare = api.Context(0)
        try:
            with pytest.raises(api.DcregError) as e:
                bare.register_frames_normals(frames, T0, "Ours", cfg)
            assert "(%d)" % api.E_STATE in str(e.value) and "target" in str(e.value)
        finally:
            bare.close()
    finally:
        c.close()
