"""dcreg_register_frames: many frames registered against one resident map in a single batched call.  Every frame's record is bitwise the
single registration of that frame (dcreg_set_source + dcreg_icp_run) on a context holding the same map - frames of very different sizes
side by side in one launch, slots refilled as frames finish, one-wave blocks or not, a frame that aborts, an empty frame - the context's
own source and states are left alone, a capped map's window index stays invisible, and the last iteration agrees with the CPU oracle."""
import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from oracle import pyoracle as po
from test_gpu_configs import cfg_pair
from test_gpu_round6 import _window_pair

pytestmark = pytest.mark.gpu

SIZES = [40, 63, 257, 1000, 8000, 12000, 3000, 500, 5000, 2000, 8000, 700, 6000, 150, 9000, 4000, 1500, 8000, 300, 2500, 7000, 100, 10000, 8000]
OFF_MAP = 7             # this frame starts 300 m away from the map: no correspondences (n_eff < 10), status 1


def _frame_poses(gt, n, seed, step=6.0):
    """sensor poses around the PK01 position (true) and the perturbed starts of their registrations"""
    rng = np.random.default_rng(seed)
    T, T0 = [], []
    for k in range(n):
        Tk = gt @ h.pose6d_matrix(rng.uniform(-step, step), rng.uniform(-step, step), 0.0, 0.0, 0.0, h.deg2rad(rng.uniform(-20, 20)))
        d = h.pose6d_matrix(*rng.uniform(-0.15, 0.15, 3), *h.deg2rad(rng.uniform(-0.5, 0.5, 3)))
        T.append(Tk)
        T0.append(Tk @ d)
    return T, T0


_single = h.single_registration          # (test_gpu_pairs imports these two from here)
_assert_record = h.assert_record


@pytest.fixture(scope="module")
def scene():
    tgt, _ = h.scene_parkinglot()
    gt = h.pose6d_matrix(**h.PK01_GT)
    T, T0 = _frame_poses(gt, len(SIZES), seed=5)
    frames = h.map_frames(tgt, T, SIZES, seed=3)
    assert [len(f) for f in frames] == SIZES
    T0[OFF_MAP] = T0[OFF_MAP] @ h.pose6d_matrix(300.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    cfg, ocfg = cfg_pair(0.5, 30, 0, 1e-5, 1e-3, gt.reshape(16))
    return tgt, frames, T0, cfg, ocfg


@pytest.fixture(scope="module")
def singles(scene):
    tgt, frames, T0, cfg, _ = scene
    out = {}
    c = api.Context(0)
    try:
        c.set_target(tgt, 0.5)
        for method in ("Ours", "ME-TSVD"):
            out[method] = [_single(c, f, T, method, cfg) for f, T in zip(frames, T0)]
    finally:
        c.close()
    return out


@pytest.mark.parametrize("method", ["Ours", "ME-TSVD"])
@pytest.mark.parametrize("slots", [8, 0])
@pytest.mark.parametrize("one_wave", [0, 2])
def test_frames_are_bitwise_single_registrations(scene, singles, method, slots, one_wave):
    tgt, frames, T0, cfg, _ = scene
    c = api.Context(0)
    try:
        c.set_option("one_wave", one_wave)
        c.set_target(tgt, 0.5)
        recs = c.register_frames(frames, T0, method, cfg, slots=slots)
        assert len(recs) == len(frames)
        for k, (tr, s) in enumerate(zip(recs, singles[method])):
            _assert_record(tr, s, (k, SIZES[k]))
            if s["trans_err"] is not None and tr.status == 0:
                assert tr.trans_error_m == s["trans_err"], k
        assert recs[OFF_MAP].status == 1
        assert c.index_info().n_source == 0                                  # no source was ever set on this context
    finally:
        c.close()


def test_frames_in_one_buffer_with_offsets(scene, singles):
    """the (xyz, offsets) form: the same records as the list form"""
    tgt, frames, T0, cfg, _ = scene
    c = api.Context(0)
    try:
        c.set_target(tgt, 0.5)
        off = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
        recs = c.register_frames((np.concatenate(frames, 0), off), T0, "Ours", cfg, slots=5)
        for k, (tr, s) in enumerate(zip(recs, singles["Ours"])):
            _assert_record(tr, s, k)
    finally:
        c.close()


def _same_sums(a, b):
    return (a["n_eff"] == b["n_eff"] and a["n_pt"] == b["n_pt"] and np.array_equal(a["H_upper"], b["H_upper"]) and np.array_equal(a["g"], b["g"])
            and a["sum_r2"] == b["sum_r2"] and a["sum_b2"] == b["sum_b2"])


def test_the_context_is_left_alone(scene):
    """source, own neighbour state and reserved warm states of the context: linearisations after the call give what they give without it"""
    tgt, frames, T0, cfg, _ = scene
    src = frames[4]
    T = T0[4]
    prm = api.default_lin_params(0.5, 0)
    Rs = [T[:3, :3], (T @ h.pose6d_matrix(0.05, 0, 0, 0, 0, 0))[:3, :3]]
    ts = [T[:3, 3], (T @ h.pose6d_matrix(0.05, 0, 0, 0, 0, 0))[:3, 3]]
    a, b = api.Context(0), api.Context(0)
    try:
        seq = {}
        for name, c in (("call", a), ("control", b)):
            c.set_target(tgt, 0.5)
            c.set_source(src)
            c.reserve_warm_states(2)
            first = c.linearize(T[:3, :3], T[:3, 3], prm)
            bfirst = c.linearize_batch_warm(Rs, ts, [0, 1], prm)
            n_src = c.index_info().n_source
            if name == "call":
                recs = c.register_frames(frames[:10], T0[:10], "Ours", cfg, slots=4)
                assert len(recs) == 10
            assert c.index_info().n_source == n_src == len(src)
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


@pytest.mark.timeout(900)
def test_frames_on_a_capped_map_match_its_single_registrations():
    """a map whose table budget binds (the window index engages for single registrations): the frames, searched on the whole map's index,
    give bitwise what the capped context's single registrations give"""
    tgt, _, gt, _ = _window_pair()
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1, gt_matrix=gt.reshape(16))
    T, T0 = _frame_poses(gt, 6, seed=9, step=4.0)
    frames = h.map_frames(tgt, T, 8000, seed=4)
    c = api.Context(0)
    try:
        c.set_option("max_table_entries", 1 << 21)
        c.set_target(tgt, 0.5)
        recs = c.register_frames(frames, T0, "Ours", cfg, slots=4)
        singles = [_single(c, f, T_, "Ours", cfg) for f, T_ in zip(frames, T0)]
        assert c.roi_info()["whole_map_capped"] and c.roi_info()["windows_built"] >= 1
        for k, (tr, s) in enumerate(zip(recs, singles)):
            _assert_record(tr, s, k)
    finally:
        c.close()


def test_a_frame_record_matches_the_oracle(scene, singles):
    """the 1000-point frame: its record against the last iteration of the CPU oracle's run"""
    tgt, frames, T0, cfg, ocfg = scene
    k = SIZES.index(1000)
    c = api.Context(0)
    try:
        c.set_target(tgt, 0.5)
        tr = c.register_frames(frames, T0, "Ours", cfg, slots=8)[k]
    finally:
        c.close()
    ores, ologs = po.icp_run(po.KdTree(tgt), frames[k], T0[k], "Ours", ocfg)
    assert (tr.iterations, tr.converged, tr.status) == (ores.iterations, ores.converged, ores.status)
    assert tr.corr_num == ologs[-1].n_eff
    T = np.array(tr.final_transform[:]).reshape(4, 4)
    assert np.allclose(T[:3, :3].reshape(9), ores.R[:], rtol=0, atol=1e-8) and np.allclose(T[:3, 3], ores.t[:], rtol=0, atol=1e-8)
    assert h.rel_err(tr.H_upper[:], ologs[-1].H_upper[:]) < 1e-7


def test_refusals_and_empty_frames(scene, singles):
    tgt, frames, T0, cfg, _ = scene
    c, bare = api.Context(0), api.Context(0)
    try:
        c.set_target(tgt, 0.5)
        before = c.launch_stats()["launches"]
        bad = [f.copy() for f in frames[:4]]
        bad[2][5, 1] = np.nan
        with pytest.raises(api.DcregError, match=r"\(-\d+\).*non-finite"):
            c.register_frames(bad, T0[:4], "Ours", cfg)
        xyz = np.concatenate(frames[:3], 0)
        with pytest.raises(api.DcregError, match="decrease"):
            c.register_frames((xyz, np.array([0, 40, 30, len(xyz)])), T0[:3], "Ours", cfg)
        assert c.launch_stats()["launches"] == before
        with pytest.raises(api.DcregError, match="target"):
            bare.register_frames(frames[:3], T0[:3], "Ours", cfg)
        assert bare.launch_stats()["launches"] == 0
        assert c.register_frames([], np.zeros((0, 4, 4)), "Ours", cfg) == []
        # an empty frame: status 3, the others run as they would alone
        mixed = [frames[3], np.zeros((0, 3), np.float32), frames[4]]
        recs = c.register_frames(mixed, [T0[3], T0[0], T0[4]], "Ours", cfg, slots=2)
        assert recs[1].status == 3 and recs[1].iterations == 0
        _assert_record(recs[0], singles["Ours"][3], 0)
        _assert_record(recs[2], singles["Ours"][4], 2)
    finally:
        c.close(); bare.close()
