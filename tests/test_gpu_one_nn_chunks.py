"""The two 1-NN engines (dcreg_linearize_normals, dcreg_linearize_gicp and their batched forms) PAST ONE CHUNK of the reduction: block rows
are added in chunks of 64 (kChunk: 16 384 points), the chunk sums into the pose's result row (k_finalize).  Sources of 16 384 points
(exactly one chunk), 16 385 (a second chunk of one block holding one point), 16 897 (67 blocks) and 32 769 (three chunks, the last
holding one point) on the lot of tests/normal_icp_scenes.py: the dump is bitwise the numpy reference's, every one of the 31 sums lies
within the derived bound of the exact sum over the reference's rows (tests/sums_check.py), the plain call, the warm call and the dump
call agree bit for bit.  The batched launches - long frames beside frames of one point, the grid (blocks, poses) more than 64 blocks wide
while the short frames' blocks leave early - and the many-frames engines are bitwise their single forms.  The references are computed
once per module and never modified."""
import functools

import numpy as np
import pytest

import gicp_ref as gref
import gicp_scenes as gs
import helpers as h
import normal_icp_ref as ref
import normal_icp_scenes as sc
import sums_check as sums
import test_gpu_frames_gicp as fg
import test_gpu_frames_normals as fn
from dcreg_amd import api
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
PARAMS_5 = api.normal_params(k=5)
SIZES = [16384, 16385, 16897, 32769]
POSE_OF = {16384: 0, 16385: 2, 16897: 0, 32769: 2}          # of the walk: the start (0.23 m, 2.5 degrees off) and halfway to the truth
ENGINES = ["normals", "gicp"]

# the batched launch: frames in load order (an empty one among them, loaded and never launched), and (frame size, pose of the walk) per
# pose of the launch - every live frame, the 16 897-point frame at two poses, long and short frames interleaved
FRAME_SIZES = [16897, 1, 257, 0, 16385, 523]
PLAN = [(16897, 0), (1, 0), (257, 2), (16385, 1), (523, 0), (16897, 3)]


def lin_params():
    return api.default_lin_params(RADIUS, 1)


def frame(n):
    return sc.sized_source(n) if n else np.zeros((0, 3), np.float32)


def frame_normals(n):
    return gs.sized_source_normals(n) if n else np.zeros((0, 3), np.float32)


def context(engine, src=None):
    """the lot's map with its bounded normals kept; src = a size: sized_source(src) as the own source, with its normals for the third engine"""
    if engine == "normals":
        return fn.context(None if src is None else frame(src))
    return fg.context(None if src is None else frame(src), None if src is None else frame_normals(src))


def linearize(c, engine, T, debug=False):
    return (c.linearize_normals if engine == "normals" else c.linearize_gicp)(T, lin_params(), debug=debug)


def batch(c, engine, Ts, ids, fids):
    return (c.normals_batch if engine == "normals" else c.gicp_batch)(Ts, ids, fids, lin_params())


@functools.lru_cache(maxsize=None)
def reference(engine, n):
    L = gs.lot()
    T = sc.walk()[POSE_OF[n]]
    if engine == "normals":
        want = ref.linearize(L["tgt"], L["nb"], sc.sized_source(n), T, RADIUS, use_weight_derivative=1)
    else:
        want = gref.linearize(L["tgt"], L["nb"], sc.sized_source(n), gs.sized_source_normals(n), T, RADIUS, gs.EPS)
    for v in want.values():
        if isinstance(v, np.ndarray):
            sc.frozen(v)
    return want


_singles = {}


def single(engine, n, pose):
    """the plain single launch of sized_source(n) at walk()[pose] on a fresh context: once per module"""
    key = (engine, n, pose)
    if key not in _singles:
        c = context(engine, n)
        try:
            _singles[key] = linearize(c, engine, sc.walk()[pose])
        finally:
            c.close()
    return _singles[key]


# ---- 1. single launches: one chunk exactly, a second chunk of one point, 67 blocks, three chunks
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("engine", ENGINES)
def test_a_source_past_one_chunk_is_the_reference_entry_by_entry(engine, n):
    T = sc.walk()[POSE_OF[n]]
    want = reference(engine, n)
    eff = np.flatnonzero(want["flag"] == 1)
    assert len(eff) > n // 4 and (want["flag"] != 1).any()
    c = context(engine, n)
    try:
        cold = linearize(c, engine, T)                          # the first call of a fresh context
        warm = linearize(c, engine, T)                          # from the words the first one left
        got = linearize(c, engine, T, debug=True)
    finally:
        c.close()
    (sc if engine == "normals" else gs).assert_dump_bitwise(got, want, (engine, n))
    sc.assert_sums_close(got, want, (engine, n))
    worst = sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], (engine, n))
    print("%s, %d points: n_eff %d, the largest error is %.3g of its bound" % (engine, n, want["n_eff"], worst))
    sc.assert_sums_bitwise(cold, got, (engine, n, "plain"))
    sc.assert_sums_bitwise(warm, cold, (engine, n, "warm"))
    _singles.setdefault((engine, n, POSE_OF[n]), cold)


# ---- 2. the batched launch: long frames beside short ones
@pytest.mark.parametrize("engine", ENGINES)
def test_a_batched_launch_of_long_and_short_frames_is_bitwise_its_single_launches(engine):
    W = sc.walk()
    c = context(engine)
    try:
        c.frames_load([frame(n) for n in FRAME_SIZES])
        if engine == "gicp":
            c.frames_normals_set([frame_normals(n) for n in FRAME_SIZES])
        c.normals_reserve_slots(len(PLAN))
        fids = [FRAME_SIZES.index(n) for n, _ in PLAN]
        Ts = [W[p] for _, p in PLAN]
        for ids in (list(range(len(PLAN))), [-1] * len(PLAN), list(range(len(PLAN)))[::-1]):     # cold slots, no slots, other frames' words
            got = batch(c, engine, Ts, ids, fids)
            assert len(got) == len(PLAN)
            for k, ((n, p), g) in enumerate(zip(PLAN, got)):
                sc.assert_sums_bitwise(g, single(engine, n, p), (engine, k, n))
        assert got[0]["n_eff"] > 4000 and got[3]["n_eff"] > 4000 and got[1]["n_pt"] <= 1
        assert got[5]["n_pt"] < got[0]["n_pt"]                  # (the jump of the walk: most points leave the radius)
        with pytest.raises(api.DcregError) as e:               # the empty frame is there, and cannot be launched
            batch(c, engine, [W[0]], [0], [FRAME_SIZES.index(0)])
        assert "(%d)" % api.E_INVALID in str(e.value)
    finally:
        c.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_the_own_source_form_past_one_chunk_is_bitwise_the_single_launch(engine):
    W = sc.walk()
    c = context(engine, 16897)
    try:
        c.normals_reserve_slots(3, frames=False)
        for ids in ([0, 1, 2], [2, 0, 1], None):
            got = batch(c, engine, [W[0], W[3], W[1]], ids, None)
            for g, p in zip(got, (0, 3, 1)):
                sc.assert_sums_bitwise(g, single(engine, 16897, p), (engine, p))
        assert got[0]["n_eff"] > 4000
    finally:
        c.close()


# ---- 3. the many-frames engines
@pytest.mark.parametrize("engine", ENGINES)
def test_registering_a_long_and_a_short_frame_is_bitwise_the_single_registrations(engine):
    L = sc.lot()
    frames = [frame(16897), frame(257)]
    T0 = [sc.offset(L["INIT"], 0.02, -0.01, 0.01, 0.002), sc.offset(L["INIT"], -0.03, 0.02, 0.0, -0.004)]
    cfg = cfg_pk01(max_iterations=4, use_weight_derivative=1)
    c, d = context(engine), context(engine)
    try:
        if engine == "normals":
            want = [fn.single_record(d, f, T, "Ours", cfg) for f, T in zip(frames, T0)]
        else:
            want = [fg.single_record(d, f, T, "Ours", cfg, PARAMS_5) for f, T in zip(frames, T0)]
        assert want[0]["status"] == 0 and want[0]["iterations"] >= 2 and want[0]["corr"] > 4000
        for slots in (1, 2):
            if engine == "normals":
                recs = c.register_frames_normals(frames, T0, "Ours", cfg, slots=slots)
            else:
                recs = c.register_frames_gicp(frames, T0, "Ours", cfg, PARAMS_5, slots=slots)
            assert len(recs) == 2
            for k, (tr, s) in enumerate(zip(recs, want)):
                h.assert_record(tr, s, (engine, slots, k))
    finally:
        c.close(); d.close()
