"""The fourth engine's many-frames form on the device: the batched launch (dcreg_voxels_batch_begin / _end, k_vlin_batch) against single
launches of dcreg_linearize_voxels on fresh contexts, the launch slots it shares with the 1-NN engines, its refusals, and the engines
dcreg_register_frames_voxels / dcreg_icp_run_trials_voxels against the loop of dcreg_set_source [+ dcreg_source_normals_keep] +
dcreg_icp_run_voxels - everything bitwise, in both modes of "voxels_source_cov".  The scenes are those of tests/voxels_scenes.py,
tests/normal_icp_scenes.py, tests/gicp_scenes.py and the dense lot of tests/test_gpu_voxels_engine.py; what a fresh context or the serial
loop gives is computed once per module and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import gicp_scenes as gs
import helpers as h
import normal_icp_scenes as sc
import sums_check as sums
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api
from test_gpu_frames_gicp import EMPTY, PLAN_POSES, PLAN_SIZES, edge_frames, frame_of
from test_gpu_voxels import MAP_PARAMS, context, lin_params
from test_gpu_voxels_engine import dense_lot
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
PARAMS_5 = api.normal_params(k=5)
I32P = C.POINTER(C.c_int32)


def lot_context(src=None, src_normals=None, mode=0, keep=True):
    L = vs.lot()
    return context(L["tgt"], src, src_normals, mode, keep)


_singles = {}


def single(key, frame, normals, mode, T, opts=()):
    """set_source(frame) [+ set_source_normals(normals)] + linearize_voxels(T) on a fresh context: once per (cloud, mode, pose, options)"""
    k = (key, mode, np.asarray(T).tobytes(), tuple(opts))
    if k not in _singles:
        c = lot_context(frame, normals if mode else None, mode)
        try:
            for name, v in opts:
                c.set_option(name, v)
            _singles[k] = c.linearize_voxels(T, lin_params())
        finally:
            c.close()
    return _singles[k]


def single_edge(n, mode, T, opts=()):
    return single(n, sc.sized_source(n), gs.sized_source_normals(n), mode, T, opts)


def single_lot(mode, T):
    L = vs.lot()
    return single("lot", L["src"], L["mb"], mode, T)


def last_error(c):
    return c._L.dcreg_last_error(c._h).decode()


def refused(call, code, text=""):
    with pytest.raises(api.DcregError) as e:
        call()
    assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)


# ---- 1. the kernel: the batched launch against single launches, at block edges
@pytest.mark.parametrize("mode", [0, 1])
def test_a_batched_launch_is_bitwise_its_single_launches_at_block_edges(mode):
    W = sc.walk()
    L = vs.lot()
    frames, normals = edge_frames()
    plan = [(n, W[p]) for n, p in zip(PLAN_SIZES, PLAN_POSES)]
    c = lot_context(mode=mode)
    try:
        c.frames_load(frames)
        if mode:
            c.frames_normals_set(normals)
        fids = [frame_of(n) for n, _ in plan]
        got = c.voxels_batch([T for _, T in plan], fids, lin_params())
        assert len(got) == len(plan)
        for k, ((n, T), g) in enumerate(zip(plan, got)):
            sc.assert_sums_bitwise(g, single_edge(n, mode, T), (k, n))
        again = c.voxels_batch([T for _, T in plan][::-1], fids[::-1], lin_params(), slot=1)          # the other slot, the other order
        for a, g in zip(again[::-1], got):
            sc.assert_sums_bitwise(a, g)
        assert any(g["n_eff"] >= 10 for g in got) and got[1]["n_pt"] <= 1
        # one pose against the numpy reference, as the single launch is compared with it (tests/test_gpu_voxels.py): the counts exactly, the
        # sums to the tolerances of the exactly rounded reference sums - and the single launch's dump, whose sums these are, bitwise
        n, T = plan[0]
        assert n == 523
        src, m = sc.sized_source(n), gs.sized_source_normals(n)
        want = vr.linearize(L["vmap"], src, T, mode, m if mode else None, vs.GICP_EPS)
        sc.assert_sums_close(got[0], want, "reference")
        sums.assert_sums_entrywise(got[0], want["row"], want["n_eff"], want["n_pt"], "reference")      # every slot against its own terms
        assert all((want["flag"] == f).any() for f in ((0, 1, 3) if mode else (0, 1)))
        d = lot_context(src, m if mode else None, mode)
        try:
            dump = d.linearize_voxels(T, lin_params(), debug=True)
        finally:
            d.close()
        vs.assert_dump_bitwise(dump, want, "reference")
        sc.assert_sums_bitwise(got[0], dump, "dump")
    finally:
        c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_own_source_form_is_bitwise_the_single_launch(mode):
    """frame_ids = None: every pose linearises the context's own source (mode 1: with its kept source normals)"""
    L = vs.lot()
    W = sc.walk()
    c = lot_context(L["src"], L["mb"], mode)
    try:
        poses = [W[0], W[3], W[1], W[2]]
        for slot in (0, 1):
            got = c.voxels_batch(poses, None, lin_params(), slot=slot)
            for g, T in zip(got, poses):
                sc.assert_sums_bitwise(g, single_lot(mode, T))
        assert got[0]["n_eff"] > 100
        # loaded frames beside it change nothing, and the frames form reads them, not the source
        c.frames_load([sc.sized_source(65), L["src"]])
        if mode:
            c.frames_normals_set([gs.sized_source_normals(65), L["mb"]])
        sc.assert_sums_bitwise(c.voxels_batch([W[2]], None, lin_params())[0], single_lot(mode, W[2]))
        both = c.voxels_batch([W[2], W[2]], [0, 1], lin_params())
        sc.assert_sums_bitwise(both[0], single_edge(65, mode, W[2]))
        sc.assert_sums_bitwise(both[1], single_lot(mode, W[2]))
    finally:
        c.close()


# ---- 2. two slots and the refusals around them
def test_both_launch_slots_in_flight_and_what_is_refused_meanwhile():
    L = vs.lot()
    W = sc.walk()
    frames = [L["src"], sc.sized_source(257), sc.sized_source(65)]
    keys = ["lot", 257, 65]
    c = lot_context(L["src"])
    try:
        before = c.linearize_voxels(W[1], lin_params())
        vox = c.kept_target_voxels()
        c.frames_load(frames)
        set0 = [(0, W[0]), (1, W[2]), (2, W[1])]
        set1 = [(2, W[3]), (0, W[2])]
        n0 = c.voxels_batch_begin([T for _, T in set0], [f for f, _ in set0], lin_params(), slot=0)
        n1 = c.voxels_batch_begin([T for _, T in set1], [f for f, _ in set1], lin_params(), slot=1)
        # while either is pending, the calls that queue work are refused and change nothing - the other engines' launches on the same slot among them
        calls = (lambda: c.set_source(frames[1]), lambda: c.linearize_voxels(W[1], lin_params()), lambda: c.keep_target_voxels(MAP_PARAMS),
                 lambda: c.drop_target_voxels(), lambda: c.frames_load(frames), lambda: c.set_target(L["tgt"], RADIUS),
                 lambda: c.normals_batch_begin([W[0]], None, [0], lin_params(), slot=1), lambda: c.gicp_batch_begin([W[0]], None, [0], lin_params(), slot=0),
                 lambda: c.voxels_batch_begin([W[0]], [0], lin_params(), slot=0), lambda: c.voxels_batch_begin([W[0]], None, lin_params(), slot=1),
                 lambda: c.register_frames_voxels(frames, [W[0]] * 3, "Ours", cfg_pk01()), lambda: c.icp_run_trials_voxels([W[0]], "Ours", cfg_pk01()))
        for k, call in enumerate(calls):
            with pytest.raises(api.DcregError) as e:
                call()
            assert "(%d)" % api.E_STATE in str(e.value), k
        got1 = c.voxels_batch_end(n1, slot=1)
        for k, call in enumerate(calls[:5]):                               # slot 0 is still pending
            with pytest.raises(api.DcregError) as e:
                call()
            assert "(%d)" % api.E_STATE in str(e.value), k
        got0 = c.voxels_batch_end(n0, slot=0)
        for got, plan in ((got0, set0), (got1, set1)):
            for g, (f, T) in zip(got, plan):
                sc.assert_sums_bitwise(g, single(keys[f], frames[f], None, 0, T), f)
        for slot in (0, 1):                                                # a second _end: nothing is in flight
            refused(lambda: c.voxels_batch_end(1, slot=slot), api.E_STATE)
        assert c.index_info().n_source == 523 and c.target_voxels_kept() == vs.lot()["vmap"]["n_kept"]
        vs.assert_map_bitwise(c.kept_target_voxels(), vox)
        sc.assert_sums_bitwise(c.linearize_voxels(W[1], lin_params()), before)
        # a pending launch of another engine on a slot refuses this one there; the other slot takes it, and both come back right
        c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
        m0 = c.normals_batch_begin([W[0]], None, [0], lin_params(), slot=0)
        refused(lambda: c.voxels_batch_begin([W[0]], [1], lin_params(), slot=0), api.E_STATE, "slot 0")
        m1 = c.voxels_batch_begin([W[0]], [1], lin_params(), slot=1)
        only_n = api.Context(0)
        try:
            only_n.set_target(L["tgt"], RADIUS)
            only_n.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
            only_n.frames_load(frames)
            want_n = only_n.normals_batch([W[0]], None, [0], lin_params())[0]
        finally:
            only_n.close()
        sc.assert_sums_bitwise(c.normals_batch_end(m0, slot=0)[0], want_n)
        sc.assert_sums_bitwise(c.voxels_batch_end(m1, slot=1)[0], single(257, frames[1], None, 0, W[0]))
    finally:
        c.close()


# ---- 3. the state refusals of _begin, each with its code and text; after each a valid launch returns the right bits
def test_refusals_queue_nothing():
    L = vs.lot()
    W = sc.walk()
    frames, normals = edge_frames()
    c = lot_context(L["src"], keep=False)

    def raw(n, Ts, fids, prm, slot=0):
        Rs, ts, _ = api._poses_arg(Ts)
        f = None if fids is None else np.ascontiguousarray(fids, np.int32)
        return c._L.dcreg_voxels_batch_begin(c._h, slot, n, api._dp(Rs), api._dp(ts), None if f is None else f.ctypes.data_as(I32P), C.byref(prm))

    def own_ok():
        sc.assert_sums_bitwise(c.voxels_batch([W[0], W[1]], None, lin_params())[1], single_lot(0, W[1]))

    def frames_ok():
        sc.assert_sums_bitwise(c.voxels_batch([W[0]], [frame_of(523)], lin_params())[0], single_edge(523, 0, W[0]))

    try:
        refused(lambda: c.voxels_batch_begin([W[0]], None, lin_params()), api.E_STATE, "no kept voxels: dcreg_target_voxels_keep first")
        c.keep_target_voxels(MAP_PARAMS)
        own_ok()
        c.drop_target_voxels()
        refused(lambda: c.voxels_batch_begin([W[0]], None, lin_params()), api.E_STATE, "no kept voxels")
        c.keep_target_voxels(MAP_PARAMS)
        own_ok()
        c.set_target(L["tgt"], RADIUS)                                    # the member is dropped with the map's points
        assert c.target_voxels_kept() == 0
        refused(lambda: c.voxels_batch_begin([W[0]], None, lin_params()), api.E_STATE, "no kept voxels")
        c.keep_target_voxels(MAP_PARAMS)
        c.set_source(L["src"])
        own_ok()
        refused(lambda: c.voxels_batch_begin([W[0]], [0], lin_params()), api.E_STATE, "no frames")
        own_ok()
        c.frames_load(frames)
        for bad in (len(frames), -1, EMPTY):
            refused(lambda: c.voxels_batch_begin([W[0], W[0]], [0, bad], lin_params()), api.E_INVALID, "frame %d is not loaded or empty" % bad)
            frames_ok()
        c.set_option("voxels_source_cov", 1)
        refused(lambda: c.voxels_batch_begin([W[0]], [0], lin_params()), api.E_STATE, "no kept frame normals")
        refused(lambda: c.voxels_batch_begin([W[0]], None, lin_params()), api.E_STATE, "no kept source normals")
        c.frames_normals_set(normals)
        sc.assert_sums_bitwise(c.voxels_batch([W[0]], [frame_of(257)], lin_params())[0], single_edge(257, 1, W[0]))
        refused(lambda: c.voxels_batch_begin([W[0]], None, lin_params()), api.E_STATE, "no kept source normals")       # the frames' are not the source's
        c.set_option("voxels_source_cov", 0)
        frames_ok()
        euler = api.default_lin_params(RADIUS, euler_rpy=(0.0, 0.0, 0.0))
        assert raw(1, [W[0]], [0], euler) == api.E_INVALID and "SO(3) row only" in last_error(c)
        frames_ok()
        bad_pose = W[0].copy()
        bad_pose[1, 3] = np.nan
        refused(lambda: c.voxels_batch_begin([W[0], bad_pose, W[1]], [0, 1, 2], lin_params()), api.E_INVALID, "a pose is not finite")
        bad_pose = W[0].copy()
        bad_pose[0, 0] = np.inf
        refused(lambda: c.voxels_batch_begin([W[0], W[1], bad_pose], None, lin_params()), api.E_INVALID, "a pose is not finite")
        own_ok()
        for slot in (2, -1):
            refused(lambda: c.voxels_batch_begin([W[0]], [0], lin_params(), slot=slot), api.E_INVALID, "invalid slot %d" % slot)
        assert raw(0, [W[0]], [0], lin_params()) == api.E_INVALID
        refused(lambda: c.voxels_batch_begin(np.zeros((0, 4, 4)), None, lin_params()), api.E_INVALID)
        for slot in (0, 1):
            refused(lambda: c.voxels_batch_end(1, slot=slot), api.E_STATE)                                              # nothing was queued
        frames_ok()
        own_ok()
        # a context without a target, and one without a source
        bare = api.Context(0)
        try:
            refused(lambda: bare.voxels_batch_begin([W[0]], None, lin_params()), api.E_STATE, "no target")
        finally:
            bare.close()
        n = lot_context()
        try:
            refused(lambda: n.voxels_batch_begin([W[0]], None, lin_params()), api.E_STATE, "no source")
            n.frames_load(frames)
            sc.assert_sums_bitwise(n.voxels_batch([W[0]], [frame_of(523)], lin_params())[0], single_edge(523, 0, W[0]))
        finally:
            n.close()
    finally:
        c.close()


# ---- 4. nothing else moves
def test_the_launches_leave_every_other_engine_alone():
    L = vs.lot()
    W = sc.walk()
    frames, normals = edge_frames()
    prm1 = api.default_lin_params(RADIUS, 1)

    def others(ctx):
        out = []
        for T in (W[1], W[2]):
            R, t = np.ascontiguousarray(T[:3, :3]).reshape(9), np.ascontiguousarray(T[:3, 3])
            o = api.LinOut()
            ctx.linearize_raw(R, t, prm1, o)
            out.append((np.array(o.H_upper[:]).tobytes(), np.array(o.g[:]).tobytes(), o.sum_r2, o.sum_b2, o.n_eff, o.n_pt))
            for lin in (ctx.linearize_normals, ctx.linearize_gicp):
                g = lin(T, lin_params())
                out.append(tuple(np.asarray(g[k]).tobytes() for k in sc.SUM_KEYS))
        return out

    c = lot_context(L["src"], L["mb"])
    try:
        c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
        others(c)                                                          # the warm words and the neighbour state now hold W[2]'s
        before = others(c)
        tn, sn, vox = c.kept_target_normals(), c.kept_source_normals(), c.kept_target_voxels()
        c.frames_load(frames)
        c.frames_normals_set(normals)
        for mode in (0, 1):
            c.set_option("voxels_source_cov", mode)
            got = c.voxels_batch([W[0], W[3], W[2]], [frame_of(523), frame_of(257), frame_of(1)], lin_params(), slot=mode)
            sc.assert_sums_bitwise(got[1], single_edge(257, mode, W[3]))
            own = c.voxels_batch([W[3], W[0]], None, lin_params(), slot=1 - mode)
            sc.assert_sums_bitwise(own[0], single_lot(mode, W[3]))
        c.set_option("voxels_source_cov", 0)
        assert others(c) == before
        for a, b in zip(c.kept_target_normals() + c.kept_source_normals(), tn + sn):
            assert sc.same_bits(a, b)
        vs.assert_map_bitwise(c.kept_target_voxels(), vox)
        assert c.index_info().n_source == 523 and c.target_normals_kept() == 1 and c.source_normals_kept() == 1
    finally:
        c.close()


# ---- 5. the options are read at _begin
def test_the_robust_kernel_and_epsilon_are_read_at_begin():
    W = sc.walk()
    frames, normals = edge_frames()
    opts = (("robust_kernel", 3.0), ("gicp_robust_scale", 0.7), ("gicp_epsilon", 1e-2))
    plan = [(523, W[0]), (257, W[2]), (65, W[1])]
    c = lot_context(mode=1)
    try:
        c.frames_load(frames)
        c.frames_normals_set(normals)
        for k, v in opts:
            c.set_option(k, v)
        n = c.voxels_batch_begin([T for _, T in plan], [frame_of(m) for m, _ in plan], lin_params())
        for k, v in (("robust_kernel", 0.0), ("gicp_robust_scale", 1.0), ("gicp_epsilon", 1e-3)):          # back to the defaults, launch in flight
            c.set_option(k, v)
        got = c.voxels_batch_end(n)
        for g, (m, T) in zip(got, plan):
            sc.assert_sums_bitwise(g, single_edge(m, 1, T, opts), m)
            plain = single_edge(m, 1, T)
            assert g["n_eff"] == plain["n_eff"] and not np.array_equal(g["H_upper"], plain["H_upper"])
        for g, (m, T) in zip(c.voxels_batch([T for _, T in plan], [frame_of(m) for m, _ in plan], lin_params()), plan):
            sc.assert_sums_bitwise(g, single_edge(m, 1, T), m)            # the next launch reads the options as they are now
    finally:
        c.close()


# ---- 6. the engine, frames: every record bitwise the serial loop's on the same context
N_REG = 70
PREFIXES = [1500, 523, 257, 256, 64, 9, 1, 0]


@functools.lru_cache(maxsize=None)
def drive():
    """70 registrations: prefixes of the dense lot's 1 500-point frame (1500 .. 1 points and an empty frame) cycling against five start
    poses - INIT, GT, two small offsets of INIT, a pose 500 m away"""
    D = dense_lot()
    starts = [D["INIT"], D["GT"], sc.offset(D["INIT"], 0.05, -0.04, 0.02, 0.01), sc.offset(D["INIT"], -0.08, 0.06, -0.01, -0.015),
              sc.offset(D["INIT"], 500.0, 0.0, 0.0)]
    sizes = [PREFIXES[k % len(PREFIXES)] for k in range(N_REG)]
    frames = [sc.frozen(np.ascontiguousarray(D["src"][:n])) for n in sizes]
    return frames, [starts[k % len(starts)] for k in range(N_REG)], sizes


@pytest.fixture(scope="module")
def dense_ctx():
    D = dense_lot()
    c = api.Context(0)
    c.set_target(D["tgt"], RADIUS)
    assert c.keep_target_voxels(MAP_PARAMS)["n_kept"] == D["vmap"]["n_kept"]
    yield c
    c.set_option("voxels_source_cov", 0)
    c.close()


def single_record(c, frame, T0, method, cfg, mode):
    """the record the many-frames calls promise for one frame: set_source [+ keep_source_normals] + icp_run_voxels (the fields of
    tests/test_gpu_frames_gicp.py's single_record)"""
    if frame is not None:
        c.set_source(frame)
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


_serial = {}


def cfg_of(max_iterations):
    return cfg_pk01(max_iterations=max_iterations, gt_matrix=np.ascontiguousarray(dense_lot()["GT"]).reshape(16))


def serial_records(c, method, mode, max_iterations):
    """the serial loop over the drive on the context c, once per (method, mode, cap)"""
    key = (method, mode, max_iterations)
    if key not in _serial:
        frames, T0, _ = drive()
        c.set_option("voxels_source_cov", mode)
        cfg = cfg_of(max_iterations)
        _serial[key] = [None if len(f) == 0 else single_record(c, f, T, method, cfg, mode) for f, T in zip(frames, T0)]
    return _serial[key]


@pytest.mark.parametrize("slots", [0, 3, 64])
@pytest.mark.parametrize("method,mode,cap", [("Ours", 0, 30), ("NONE", 0, 30), ("Ours", 1, 30), ("NONE", 1, 30), ("Ours", 0, 3)])
def test_frames_are_bitwise_the_loop_of_single_registrations(dense_ctx, method, mode, cap, slots):
    """Measured on the device: see the printed line of every case (converged, capped, aborted and empty records of the 70)."""
    frames, T0, sizes = drive()
    c = dense_ctx
    want = serial_records(c, method, mode, cap)
    # the scene is not vacuous, on the serial records: converged runs, runs of five or more iterations, status 1 (the far pose, the
    # 9-point and the 1-point frame), status 3 for the empty frame and only for it; with the cap of 3, runs that stop there unconverged
    live = [s for s in want if s is not None]
    assert [s is None for s in want] == [n == 0 for n in sizes]
    assert all(s["status"] == 1 for s, n, k in zip(want, sizes, range(N_REG)) if s is not None and (n in (9, 1) or k % 5 == 4))
    assert any(s["status"] == 1 and n >= 64 for s, n in zip(want, sizes) if s is not None)
    capped = sum(s["status"] == 0 and s["converged"] == 0 and s["iterations"] == cap for s in live)
    conv = sum(s["converged"] == 1 for s in live)
    print("%s mode %d cap %d, %d slots: %d converged, %d at the cap, %d status 1, at most %d iterations"
          % (method, mode, cap, slots, conv, capped, sum(s["status"] == 1 for s in live), max(s["iterations"] for s in live)))
    if cap == 3:
        assert capped > 0
        first = want[0]                                                    # the 1 500-point frame from INIT: the cap leaves it unconverged
        assert (first["status"], first["converged"], first["iterations"]) == (0, 0, 3)
    else:
        assert conv > 0 and any(s["iterations"] >= 5 for s in live)
        assert want[0]["converged"] == 1                                   # the 1 500-point frame from INIT (the numpy engine's result)
    c.set_option("voxels_source_cov", mode)
    recs = c.register_frames_voxels(frames, T0, method, cfg_of(cap), PARAMS_5 if mode else None, slots=slots)
    assert len(recs) == N_REG
    for k, (tr, s) in enumerate(zip(recs, want)):
        if s is None:
            assert (tr.status, tr.iterations, tr.converged) == (3, 0, 0), k
            continue
        assert tr.status != 3, k
        h.assert_record(tr, s, (k, sizes[k]))
        if s["trans_err"] is not None and tr.status == 0:
            assert tr.trans_error_m == s["trans_err"] and tr.rot_error_deg == s["rot_err"], k
    assert c.frames_normals_kept() == mode
    assert c.target_voxels_kept() == dense_lot()["vmap"]["n_kept"]


# ---- 7. the engine, trials
@pytest.mark.parametrize("mode", [0, 1])
def test_trials_are_bitwise_single_runs(dense_ctx, mode):
    D = dense_lot()
    rng = np.random.default_rng(23)
    T0 = [sc.offset(D["INIT"], *rng.uniform(-0.1, 0.1, 3), yaw=rng.uniform(-np.pi / 180.0, np.pi / 180.0)) for _ in range(66)]
    T0[37] = sc.offset(D["INIT"], 500.0, 0.0, 0.0)
    cfg = cfg_of(30)
    c = dense_ctx
    c.set_option("voxels_source_cov", mode)
    c.set_source(D["src"])
    if mode:
        refused(lambda: c.icp_run_trials_voxels(T0, "Ours", cfg), api.E_STATE, "no kept source normals")
        c.set_source_normals(np.ascontiguousarray(D["m5"], np.float32))
    before = c.linearize_voxels(D["INIT"], lin_params())
    recs = c.icp_run_trials_voxels(T0, "Ours", cfg)
    assert len(recs) == 66
    for k, (tr, T) in enumerate(zip(recs, T0)):
        h.assert_record(tr, single_record(c, None, T, "Ours", cfg, mode), k)
    assert recs[37].status == 1 and sum(tr.status == 0 and tr.converged == 1 for tr in recs) > 30 and max(tr.iterations for tr in recs) >= 5
    assert c.icp_run_trials_voxels(np.zeros((0, 4, 4)), "Ours", cfg) == []
    assert c.index_info().n_source == 1500 and c.source_normals_kept() == mode
    sc.assert_sums_bitwise(c.linearize_voxels(D["INIT"], lin_params()), before)


# ---- 8. call-level refusals: results untouched, the frames loaded before still usable
def test_call_level_refusals_leave_results_and_frames_alone():
    L = vs.lot()
    W = sc.walk()
    frames = [L["src"], sc.sized_source(257)]
    T0 = [W[0], W[1]]
    cfg = cfg_pk01()

    def call(ctx, fr, prm=None):
        """the raw call: (code, results as they come back)"""
        xyz, off, n = api._frames_arg(fr, "test")
        R0, t0, _ = api._poses_arg(T0)
        res = (api.TrialResult * n)()
        for r in res:
            r.iterations = -7
        rc = ctx._L.dcreg_register_frames_voxels(ctx._h, n, xyz.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int64)), xyz.shape[1],
                                                 None if prm is None else C.byref(prm), api._dp(R0), api._dp(t0), 0, 0, C.byref(cfg), 0, res)
        return rc, [r.iterations for r in res]

    def loaded_ok(ctx):
        sc.assert_sums_bitwise(ctx.voxels_batch([W[0]], [1], lin_params())[0], single_edge(257, 0, W[0]))

    c = lot_context(keep=False)
    try:
        c.frames_load(frames)
        assert call(c, frames) == (api.E_STATE, [-7, -7]) and "no kept voxels: dcreg_target_voxels_keep first" in last_error(c)
        refused(lambda: c.icp_run_trials_voxels(T0, "Ours", cfg), api.E_STATE, "no kept voxels")
        c.keep_target_voxels(MAP_PARAMS)
        loaded_ok(c)                                                       # the refused call loaded nothing
        c.set_option("voxels_source_cov", 1)
        bad = api.normal_params()
        bad.k = 2
        assert call(c, frames, bad) == (api.E_INVALID, [-7, -7]) and "normal k" in last_error(c)
        assert call(c, frames, None) == (api.E_INVALID, [-7, -7]) and "null normal parameters" in last_error(c)
        assert call(c, [], bad)[0] == api.E_INVALID                        # ... before the empty call returns
        c.set_option("voxels_source_cov", 0)
        assert call(c, [], bad)[0] == api.OK                               # mode 0: not read
        loaded_ok(c)
        nan = [frames[0], frames[1].copy()]
        nan[1][100, 2] = np.nan
        assert call(c, nan) == (api.E_INVALID, [-7, -7])
        loaded_ok(c)                                                       # a load refused for its frames leaves the loaded ones
        recs = c.register_frames_voxels(frames, T0, "Ours", cfg)
        assert [r.status for r in recs] in ([0, 0], [0, 1], [1, 0], [1, 1]) and all(r.iterations > 0 for r in recs)
    finally:
        c.close()
    bare = api.Context(0)
    try:
        assert call(bare, frames) == (api.E_STATE, [-7, -7]) and "target" in last_error(bare)
        refused(lambda: bare.icp_run_trials_voxels(T0, "Ours", cfg), api.E_STATE, "target")
    finally:
        bare.close()


# ---- 9. mode 0 skips the normals pass
def test_mode_0_runs_no_normals_pass_and_mode_1_needs_its_parameters():
    L = vs.lot()
    W = sc.walk()
    frames = [L["src"], sc.sized_source(257), np.zeros((0, 3), np.float32)]
    T0 = [W[0], W[1], W[0]]
    cfg = cfg_pk01()
    c = lot_context()
    try:
        recs = c.register_frames_voxels(frames, T0, "Ours", cfg, frame_normals=None)
        assert [r.status for r in recs][2] == 3 and recs[0].iterations > 0 and c.frames_normals_kept() == 0
        assert c.target_normals_kept() == 0                               # the map needs no normals
        c.set_option("voxels_source_cov", 1)
        refused(lambda: c.register_frames_voxels(frames, T0, "Ours", cfg, frame_normals=None), api.E_INVALID, "null normal parameters")
        assert c.frames_normals_kept() == 0
        recs1 = c.register_frames_voxels(frames, T0, "Ours", cfg, frame_normals=PARAMS_5)
        assert c.frames_normals_kept() == 1 and recs1[2].status == 3 and recs1[0].iterations > 0
        assert not np.array_equal(np.array(recs1[0].H_upper[:]), np.array(recs[0].H_upper[:]))
        # all frames empty: nothing to estimate, every record status 3
        assert [r.status for r in c.register_frames_voxels([frames[2]] * 2, T0[:2], "Ours", cfg, frame_normals=PARAMS_5)] == [3, 3]
    finally:
        c.close()
