"""The fourth engine (dcreg_linearize_voxels, dcreg_voxels_batch_begin / _end, dcreg_register_frames_voxels, dcreg_icp_run_trials_voxels)
PAST ONE CHUNK of the reduction, as tests/test_gpu_one_nn_chunks.py checks the two 1-NN engines: block rows are added in chunks of 64
(kChunk: 16 384 points), the chunk sums into the pose's result row (k_finalize).  Sources of 16 384 points (exactly one chunk), 16 385 (a
second chunk of one block holding one point), 16 897 (67 blocks) and 32 769 (three chunks, the last holding one point) against the lot's
kept voxel map, in both modes of "voxels_source_cov": the dump is bitwise the numpy reference's (tests/voxels_ref.py), every one of the
31 sums lies within the derived bound of the exact sum over the reference's rows (tests/sums_check.py), the plain call, the second call
and the dump call agree bit for bit.  The batched launches - long frames beside frames of one point, the grid (blocks, poses) more than
64 blocks wide while the short frames' blocks leave early - and the many-frames engines are bitwise their single forms.  The references
are computed once per module and never modified."""
import functools

import numpy as np
import pytest

import gicp_scenes as gs
import helpers as h
import normal_icp_scenes as sc
import sums_check as sums
import test_gpu_frames_voxels as fv
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api
from test_gpu_voxels import lin_params
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

SIZES = [16384, 16385, 16897, 32769]
POSE_OF = {16384: 0, 16385: 2, 16897: 0, 32769: 2}          # of the walk: the start (0.23 m, 2.5 degrees off) and halfway to the truth
N_EFF = {0: {16384: 10442, 16385: 11278, 16897: 10529, 32769: 22762},          # the reference's effective points, per mode
         1: {16384: 8936, 16385: 9686, 16897: 9033, 32769: 19511}}
ROBUST = (3, 0.7)                                           # a robust kernel and its "gicp_robust_scale", at one size

# the batched launch: frames in load order (an empty one among them, loaded and never launched), and (frame size, pose of the walk) per
# pose of the launch - every live frame, the 16 897-point frame at two poses, long and short frames interleaved
FRAME_SIZES = [16897, 1, 257, 0, 16385, 523]
PLAN = [(16897, 0), (1, 0), (257, 2), (16385, 1), (523, 0), (16897, 3)]


def frame(n):
    return sc.sized_source(n) if n else np.zeros((0, 3), np.float32)


def frame_normals(n):
    return gs.sized_source_normals(n) if n else np.zeros((0, 3), np.float32)


def context(n=None, mode=0):
    """the lot's map with its voxels kept; n: sized_source(n) as the own source, with its normals in mode 1"""
    return fv.lot_context(None if n is None else frame(n), frame_normals(n) if n is not None and mode else None, mode)


@functools.lru_cache(maxsize=None)
def reference(n, mode, robust=False):
    kind, scale = ROBUST if robust else (0, 1.0)
    want = vr.linearize(vs.lot()["vmap"], frame(n), sc.walk()[POSE_OF[n]], mode, frame_normals(n) if mode else None, vs.GICP_EPS, kind, scale)
    for v in want.values():
        if isinstance(v, np.ndarray):
            sc.frozen(v)
    return want


def single(n, mode, pose):
    """the plain single launch of sized_source(n) at walk()[pose] on a fresh context: once per module (tests/test_gpu_frames_voxels.py)"""
    return fv.single_edge(n, mode, sc.walk()[pose])


def check(c, n, mode, want, what):
    T = sc.walk()[POSE_OF[n]]
    cold = c.linearize_voxels(T, lin_params())                 # the first call of a fresh context
    second = c.linearize_voxels(T, lin_params())
    got = c.linearize_voxels(T, lin_params(), debug=True)
    vs.assert_dump_bitwise(got, want, what)
    worst = sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], what)
    print("voxels mode %d, %d points: n_eff %d, the largest error is %.3g of its bound" % (mode, n, want["n_eff"], worst))
    sc.assert_sums_bitwise(cold, got, (what, "plain"))
    sc.assert_sums_bitwise(second, cold, (what, "second"))
    return cold


# ---- 1. single launches: one chunk exactly, a second chunk of one point, 67 blocks, three chunks
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", [0, 1])
def test_a_source_past_one_chunk_is_the_reference_entry_by_entry(mode, n):
    want = reference(n, mode)
    assert want["n_eff"] == N_EFF[mode][n] and want["n_eff"] > n // 4 and (want["flag"] != 1).any()          # a zeroed chunk cannot hide
    assert all((want["flag"] == f).any() for f in ((0, 1, 3) if mode else (0, 1)))
    c = context(n, mode)
    try:
        cold = check(c, n, mode, want, (mode, n))
    finally:
        c.close()
    sc.assert_sums_bitwise(single(n, mode, POSE_OF[n]), cold, (mode, n, "another fresh context"))


@pytest.mark.parametrize("mode", [0, 1])
def test_a_robust_kernel_past_one_chunk_is_the_reference_entry_by_entry(mode):
    n = 16385
    want, plain = reference(n, mode, robust=True), reference(n, mode)
    assert want["n_eff"] == plain["n_eff"] > n // 4 and (want["k"] < 1.0).sum() > n // 4          # (the kernel is at work on most rows)
    c = context(n, mode)
    try:
        c.set_robust(ROBUST[0], gicp_scale=ROBUST[1])
        check(c, n, mode, want, (mode, n, "robust"))
    finally:
        c.close()


# ---- 2. the batched launch: long frames beside short ones
@pytest.mark.parametrize("mode", [0, 1])
def test_a_batched_launch_of_long_and_short_frames_is_bitwise_its_single_launches(mode):
    W = sc.walk()
    c = context(mode=mode)
    try:
        c.frames_load([frame(n) for n in FRAME_SIZES])
        if mode:
            c.frames_normals_set([frame_normals(n) for n in FRAME_SIZES])
        fids = [FRAME_SIZES.index(n) for n, _ in PLAN]
        Ts = [W[p] for _, p in PLAN]
        for slot in (0, 1, 0):                                  # both launch slots, the first one again over the words it left
            got = c.voxels_batch(Ts, fids, lin_params(), slot=slot)
            assert len(got) == len(PLAN)
            for k, ((n, p), g) in enumerate(zip(PLAN, got)):
                sc.assert_sums_bitwise(g, single(n, mode, p), (mode, slot, k, n))
        assert got[0]["n_eff"] > 4000 and got[3]["n_eff"] > 4000 and got[1]["n_pt"] <= 1
        assert got[5]["n_pt"] < got[0]["n_pt"]                  # (the jump of the walk: most points leave the map)
        if mode == 0:
            assert got[5]["n_pt"] == 8599 and got[0]["n_pt"] == N_EFF[0][16897]
        with pytest.raises(api.DcregError) as e:               # the empty frame is there, and cannot be launched
            c.voxels_batch([W[0]], [FRAME_SIZES.index(0)], lin_params())
        assert "(%d)" % api.E_INVALID in str(e.value)
        again = c.voxels_batch(Ts[::-1], fids[::-1], lin_params(), slot=1)          # a refusal queues nothing; the other order
        for a, g in zip(again[::-1], got):
            sc.assert_sums_bitwise(a, g, mode)
    finally:
        c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_own_source_form_past_one_chunk_is_bitwise_the_single_launch(mode):
    W = sc.walk()
    c = context(16897, mode)
    try:
        for slot in (0, 1):
            got = c.voxels_batch([W[0], W[3], W[1]], None, lin_params(), slot=slot)
            for g, p in zip(got, (0, 3, 1)):
                sc.assert_sums_bitwise(g, single(16897, mode, p), (mode, slot, p))
        assert got[0]["n_eff"] == N_EFF[mode][16897] and got[1]["n_pt"] < got[0]["n_pt"]
    finally:
        c.close()


# ---- 3. the many-frames engines
def starts():
    L = vs.lot()
    return [sc.offset(L["INIT"], 0.02, -0.01, 0.01, 0.002), sc.offset(L["INIT"], -0.03, 0.02, 0.0, -0.004)]


@pytest.mark.parametrize("mode", [0, 1])
def test_registering_a_long_and_a_short_frame_is_bitwise_the_single_registrations(mode):
    """The long frame's serial record: status 0 and at least 2 iterations - the numpy reference engine (vr.icp with max_iterations = 4 and
    the frame's planted normals) takes all 4 from this start without converging, in either mode: 10 581 to 12 189 effective points per
    iteration in mode 0, 9 083 to 10 300 in mode 1."""
    frames = [frame(16897), frame(257)]
    T0 = starts()
    cfg = cfg_pk01(max_iterations=4)
    c, d = context(mode=mode), context(mode=mode)
    try:
        want = [fv.single_record(d, f, T, "Ours", cfg, mode) for f, T in zip(frames, T0)]
        assert want[0]["status"] == 0 and want[0]["iterations"] >= 2 and want[0]["corr"] > 4000
        for slots in (1, 2):
            recs = c.register_frames_voxels(frames, T0, "Ours", cfg, fv.PARAMS_5 if mode else None, slots=slots)
            assert len(recs) == 2
            for k, (tr, s) in enumerate(zip(recs, want)):
                h.assert_record(tr, s, (mode, slots, k))
    finally:
        c.close(); d.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_trials_on_a_source_past_one_chunk_are_bitwise_single_runs(mode):
    T0 = starts()
    cfg = cfg_pk01(max_iterations=4)
    c = context(16897, mode)
    try:
        recs = c.icp_run_trials_voxels(T0, "Ours", cfg)
        assert len(recs) == 2
        for k, (tr, T) in enumerate(zip(recs, T0)):
            s = fv.single_record(c, None, T, "Ours", cfg, mode)
            h.assert_record(tr, s, (mode, k))
            assert s["status"] == 0 and s["iterations"] >= 2 and s["corr"] > 4000
    finally:
        c.close()
