"""Updates of the resident map (dcreg_target_insert / _insert_device / _insert_source / dcreg_target_crop).  Context A holds the map being
updated; context B is given dcreg_set_target of the cloud the update should produce, computed here on the host (the linearisation's transform:
double arithmetic, products and sums rounded one by one, float store; the thinning rule evaluated with B's dcreg_knn).  After every update
A's map equals that cloud bitwise, its index equals a full build of its grid entry for entry (dcreg_debug_index_check), and registrations,
k-NN, p2p errors and register_frames records equal B's bitwise - on the merged path and on the re-derived one."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from oracle import pyoracle as po
from test_gpu_configs import cfg_pair
from test_gpu_device_seam import DevCloud
from test_gpu_frames import _frame_poses
from test_gpu_round6 import _run_record, _window_pair

pytestmark = pytest.mark.gpu

RADIUS = 0.5
ZERO = {"points": 0, "table": 0, "row_words": 0, "gap": 0, "owner": 0}


def transform(xyz, T):
    """the map-frame points of an insert, as the device computes them (search.hpp body_to_global)"""
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    R, t = np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3]
    cols = [R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1] + R[a, 2] * p[:, 2] + t[a] for a in range(3)]
    return np.stack(cols, 1).astype(np.float32)


def thinned(ref_map, q, min_spacing):
    """the points of q the rule appends: no point of ref_map with float d2 < (float)(min_spacing^2), d2 from dcreg_knn k = 1"""
    if min_spacing <= 0.0:
        return q
    b = api.Context(0)
    try:
        b.set_target(ref_map, RADIUS)
        _, d2 = b.knn(q, k=1, max_radius=min_spacing)
    finally:
        b.close()
    return q[~(d2[:, 0] < np.float32(min_spacing * min_spacing))]


def crop_ref(cloud, lo, hi):
    p = cloud.astype(np.float64)
    keep = np.all((p >= np.asarray(lo, np.float64)) & (p <= np.asarray(hi, np.float64)), 1)
    return cloud[keep]


def _records(recs):
    return [(r.iterations, r.converged, r.status, tuple(r.final_transform[:]), r.final_rmse, r.final_fitness, r.corr_num, tuple(r.H_upper[:]))
            for r in recs]


def assert_same_as_fresh(A, expected, probe, T0, cfg, frames=None, options=()):
    """A's map is `expected` bitwise, its index exact, and it answers as a context given set_target(expected)"""
    got = A.target_points()
    assert got.shape == expected.shape and np.array_equal(got.view(np.uint32), expected.view(np.uint32))
    assert A.index_check() == ZERO
    B = api.Context(0)
    try:
        for k, v in options:
            B.set_option(k, v)
        B.set_target(expected, RADIUS)
        for c in (A, B):
            c.set_source(probe)
        assert _run_record(A, T0, cfg) == _run_record(B, T0, cfg)
        q = transform(probe, T0)
        ia, da = A.knn(q, k=5, max_radius=1.0)
        ib, db = B.knn(q, k=5, max_radius=1.0)
        assert np.array_equal(ia, ib) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
        assert A.p2p_error(T0, 0.3) == B.p2p_error(T0, 0.3)
        if frames is not None:
            T0s = np.stack([T0] * len(frames))
            assert _records(A.register_frames(frames, T0s, "Ours", cfg, slots=4)) == _records(B.register_frames(frames, T0s, "Ours", cfg, slots=4))
    finally:
        B.close()


@pytest.fixture(scope="module")
def park():
    tgt, src = h.scene_parkinglot()
    gt = h.pose6d_matrix(**h.PK01_GT)
    T, T0 = _frame_poses(gt, 6, seed=31, step=8.0)
    frames = h.map_frames(tgt, T, 8000, seed=9)
    cfg, ocfg = cfg_pair(RADIUS, 30, 0, 1e-5, 1e-3, gt.reshape(16))
    return tgt, src, gt, T, T0, frames, cfg, ocfg


def test_inserts_from_host_device_and_source(park):
    tgt, src, gt, T, T0, frames, cfg, _ = park
    base = tgt[:150_000]
    A = api.Context(0)
    try:
        A.set_target(base, RADIUS)
        expected = base
        # host, with an extra column (the real row stride), a pose that shifts the frame a little
        xyzi = np.concatenate([frames[0], np.ones((len(frames[0]), 1), np.float32)], 1)
        info = A.insert(xyzi, T[0])
        expected = np.concatenate([expected, transform(frames[0], T[0])])
        assert info == {"n_offered": len(frames[0]), "n_added": len(frames[0]), "n_removed": 0, "n_target": len(expected), "rebuilt": 0}
        assert_same_as_fresh(A, expected, src, T0[0], cfg, frames=frames[:3])
        # device memory, stride 4
        d = DevCloud(np.concatenate([frames[1], np.ones((len(frames[1]), 1), np.float32)], 1))
        try:
            info = A.insert_device(d.ptr, d.n, d.stride, T[1])
        finally:
            d.free()
        expected = np.concatenate([expected, transform(frames[1], T[1])])
        assert info["n_added"] == len(frames[1]) and info["n_target"] == len(expected)
        assert_same_as_fresh(A, expected, src, T0[1], cfg)
        # the source: set_source + icp_run + insert_source(result)
        A.set_source(frames[2])
        res, _ = A.icp_run(T0[2], "Ours", cfg)
        Tr = np.eye(4)
        Tr[:3, :3] = np.array(res.R[:]).reshape(3, 3)
        Tr[:3, 3] = res.t[:]
        info = A.insert_source(Tr)
        expected = np.concatenate([expected, transform(frames[2], Tr)])
        assert info["n_added"] == len(frames[2])
        assert_same_as_fresh(A, expected, src, T0[2], cfg, frames=frames[3:])
    finally:
        A.close()


def _drive_run(world, options):
    poses, frames = h.drive(world, 30, step=1.5, n_frame=6000, seed=12)
    cfg, _ = cfg_pair(RADIUS, 30, 0, 1e-5, 1e-3)
    A = api.Context(0)
    infos, runs, checks = [], [], 0
    try:
        for k, v in options:
            A.set_option(k, v)
        expected = transform(frames[0], poses[0])
        A.set_target(expected, RADIUS)
        for k in range(1, len(poses)):
            A.set_source(frames[k])
            T0 = poses[k] @ h.pose6d_matrix(0.05, -0.04, 0.02, 0.0, 0.0, 0.005)
            run = _run_record(A, T0, cfg)
            runs.append(run)
            Tr = np.eye(4)
            Tr[:3, :3] = np.array(run[0]).reshape(3, 3)
            Tr[:3, 3] = run[1]
            infos.append(A.insert_source(Tr))
            expected = np.concatenate([expected, transform(frames[k], Tr)])
            assert A.index_check() == ZERO, ("insert", k, infos[-1])
            if k in (12, 22):         # drop what lies more than 25 m behind the vehicle (in x)
                lo = [poses[k][0, 3] - 25.0, -1e9, -1e9]
                hi = [1e9, 1e9, 1e9]
                infos.append(dict(A.crop(lo, hi), crop=True))
                expected = crop_ref(expected, lo, hi)
                assert infos[-1]["n_removed"] > 0 and infos[-1]["n_target"] == len(expected)
                assert A.index_check() == ZERO, ("crop", k, infos[-1])
            if k % 5 == 0:
                assert_same_as_fresh(A, expected, frames[k], T0, cfg, options=options)
                checks += 1
        return infos, runs, checks
    finally:
        A.close()


def test_a_drive_with_inserts_and_crops_merges_and_rebuilds():
    world, _ = h.scene_parkinglot(n_map=400_000, extent=60.0)
    infos, runs, checks = _drive_run(world, [("map_grow_margin", 8.0)])
    assert checks >= 5
    assert any(i["rebuilt"] == 0 for i in infos) and any(i["rebuilt"] == 1 for i in infos)
    assert any(i.get("crop") and i["rebuilt"] == 0 for i in infos)           # a crop took the merged path
    infos0, runs0, _ = _drive_run(world, [("map_grow_margin", 8.0), ("map_update", 0)])
    assert all(i["rebuilt"] == 1 for i in infos0 if i["n_added"] or i["n_removed"])
    assert runs0 == runs
    assert [i["n_target"] for i in infos0] == [i["n_target"] for i in infos]


def test_thinning_keeps_what_the_rule_keeps(park):
    tgt, src, gt, T, T0, frames, cfg, _ = park
    base = tgt[:100_000]
    Tb = T[3]
    Tinv = np.linalg.inv(Tb)
    rng = np.random.default_rng(3)
    spacing = 0.1
    # duplicates of map points (d = 0), points just inside / outside the spacing, and ordinary frame points
    dup = transform(base[rng.choice(len(base), 500, replace=False)], Tinv)
    dirs = rng.normal(size=(600, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    anchors = base[rng.choice(len(base), 600, replace=False)].astype(np.float64)
    near = np.concatenate([anchors[:300] + dirs[:300] * spacing * 0.999, anchors[300:] + dirs[300:] * spacing * 1.001]).astype(np.float32)
    body = np.concatenate([dup, transform(near, Tinv), frames[3][:3000]])
    A = api.Context(0)
    try:
        A.set_target(base, RADIUS)
        q = transform(body, Tb)
        keep = thinned(base, q, spacing)
        info = A.insert(body, Tb, min_spacing=spacing)
        assert info["n_offered"] == len(body) and info["n_added"] == len(keep)
        assert 0 < len(keep) < len(body) - 500
        assert_same_as_fresh(A, np.concatenate([base, keep]), src, T0[3], cfg)
        # everything thinned: nothing changes and no state is dropped
        A.set_option("count_searches", 1)
        A.set_source(src)
        prm = api.default_lin_params(RADIUS, 0)
        ref = A.linearize(T0[3][:3, :3], T0[3][:3, 3], prm)
        A.launch_stats(reset=True)
        info = A.insert(transform(base[:2000], np.linalg.inv(Tb)), Tb, min_spacing=spacing)
        assert info["n_added"] == 0 and info["n_target"] == len(base) + len(keep)
        again = A.linearize(T0[3][:3, :3], T0[3][:3, 3], prm)
        assert A.launch_stats()["points_searched"] == 0          # the neighbour state of the first launch still serves
        assert np.array_equal(again["H_upper"], ref["H_upper"]) and np.array_equal(again["g"], ref["g"])
        assert A.index_check() == ZERO
    finally:
        A.close()


@pytest.mark.timeout(900)
def test_an_insert_into_a_capped_map_with_its_window():
    tgt, src, gt, T0 = _window_pair(n_map=2_000_000, extent=90.0)
    cfg, _ = cfg_pair(RADIUS, 30, 0, 1e-5, 1e-3, gt.reshape(16))
    opts = [("max_table_entries", 1 << 20), ("roi_index", 2)]
    A = api.Context(0)
    try:
        for k, v in opts:
            A.set_option(k, v)
        A.set_target(tgt, RADIUS)
        A.set_source(src)
        A.icp_run(T0, "Ours", cfg)
        assert A.roi_info()["active"]
        rebuilds = A.roi_info()["windows_built"]
        frame = h.map_frames(tgt, [gt @ h.pose6d_matrix(4.0, 2.0, 0.0, 0.0, 0.0, 0.1)], 8000, seed=2)[0]
        Ti = gt @ h.pose6d_matrix(4.0, 2.0, 0.0, 0.0, 0.0, 0.1)
        A.insert(frame, Ti)
        assert not A.roi_info()["active"]
        expected = np.concatenate([tgt, transform(frame, Ti)])
        assert_same_as_fresh(A, expected, src, T0, cfg, options=opts)
        assert A.roi_info()["windows_built"] > rebuilds
    finally:
        A.close()


def test_refusals_leave_the_map_as_it_was(park):
    tgt, src, gt, T, T0, frames, cfg, _ = park
    base = tgt[:80_000]
    prm = api.default_lin_params(RADIUS, 0)
    A, empty = api.Context(0), api.Context(0)
    try:
        A.set_target(base, RADIUS)
        A.insert(frames[0], T[0])
        A.set_source(src)
        ref_pts, ref_lin = A.target_points(), A.linearize(T0[0][:3, :3], T0[0][:3, 3], prm)
        bad = frames[1].copy()
        bad[7, 2] = np.nan
        nan_pose = T[1].copy()
        nan_pose[0, 3] = np.inf
        calls = [lambda: A.insert(bad, T[1]), lambda: A.insert(frames[1], nan_pose), lambda: A.insert_source(nan_pose),
                 lambda: A.insert(frames[1], T[1], min_spacing=float("nan")), lambda: A.crop([1e6, 1e6, 1e6], [1e6 + 1, 1e6 + 1, 1e6 + 1]),
                 lambda: A.crop([np.nan, 0, 0], [1, 1, 1])]
        for call in calls:
            with pytest.raises(api.DcregError):
                call()
            assert np.array_equal(A.target_points().view(np.uint32), ref_pts.view(np.uint32))
            assert A.index_check() == ZERO
            lin = A.linearize(T0[0][:3, :3], T0[0][:3, 3], prm)
            assert all(np.array_equal(lin[k], ref_lin[k]) for k in ("H_upper", "g")) and lin["n_eff"] == ref_lin["n_eff"]
        with pytest.raises(api.DcregError, match=r"\(-?\d+\).*(target|source)"):
            empty.insert(frames[1], T[1])
        with pytest.raises(api.DcregError):
            empty.crop([0, 0, 0], [1, 1, 1])
        empty.set_target(base, RADIUS)
        with pytest.raises(api.DcregError, match="source"):
            empty.insert_source(T[1])
        # through the C-ABI: stride below 3, null pointers, more than 2^31 - 1 points
        L, R9, t3 = A._L, np.ascontiguousarray(T[1][:3, :3]).reshape(9), np.ascontiguousarray(T[1][:3, 3])
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        f = np.ascontiguousarray(frames[1])
        raw = [lambda: L.dcreg_target_insert(A._h, f.ctypes.data_as(fp), len(f) * 3 // 2, 2, R9.ctypes.data_as(dp), t3.ctypes.data_as(dp), 0.0, None),
               lambda: L.dcreg_target_insert(A._h, None, len(f), 3, R9.ctypes.data_as(dp), t3.ctypes.data_as(dp), 0.0, None),
               lambda: L.dcreg_target_insert(A._h, f.ctypes.data_as(fp), len(f), 3, None, t3.ctypes.data_as(dp), 0.0, None),
               lambda: L.dcreg_target_insert(A._h, f.ctypes.data_as(fp), len(f), 3, R9.ctypes.data_as(dp), None, 0.0, None),
               lambda: L.dcreg_target_insert(A._h, f.ctypes.data_as(fp), -1, 3, R9.ctypes.data_as(dp), t3.ctypes.data_as(dp), 0.0, None),
               lambda: L.dcreg_target_insert(A._h, f.ctypes.data_as(fp), 1 << 31, 3, R9.ctypes.data_as(dp), t3.ctypes.data_as(dp), 0.0, None),
               lambda: L.dcreg_target_insert_source(A._h, None, t3.ctypes.data_as(dp), 0.0, None),
               lambda: L.dcreg_target_crop(A._h, None, t3.ctypes.data_as(dp), None),
               lambda: L.dcreg_target_get(A._h, None, len(ref_pts)),
               lambda: L.dcreg_target_get(A._h, np.empty(3 * len(ref_pts), np.float32).ctypes.data_as(fp), len(ref_pts) - 1)]
        for call in raw:
            assert call() == api.E_INVALID
            assert np.array_equal(A.target_points().view(np.uint32), ref_pts.view(np.uint32))
            assert A.index_check() == ZERO
        # a linearisation in flight: every update is refused at once, and the launch completes as if nothing had been called
        A.linearize(T0[0][:3, :3], T0[0][:3, 3], prm)
        A.linearize_begin(T0[1][:3, :3], T0[1][:3, 3], prm, slot=0)
        for call in (lambda: A.insert(frames[1], T[1]), lambda: A.insert_source(T[1]), lambda: A.crop([-1e9] * 3, [1e9] * 3),
                     lambda: A.target_points(), lambda: A.index_check()):
            with pytest.raises(api.DcregError, match=r"\(-4\)"):
                call()
        inflight = A.linearize_end(slot=0)
        assert np.array_equal(A.target_points().view(np.uint32), ref_pts.view(np.uint32))
        assert A.index_check() == ZERO
        want = A.linearize(T0[1][:3, :3], T0[1][:3, 3], prm)
        assert np.array_equal(inflight["H_upper"], want["H_upper"]) and np.array_equal(inflight["g"], want["g"])
        # a crop that removes nothing changes nothing
        info = A.crop([-1e9] * 3, [1e9] * 3)
        assert info["n_removed"] == 0 and info["n_target"] == len(ref_pts)
    finally:
        A.close()
        empty.close()


def test_the_last_iteration_after_three_inserts_matches_the_oracle(park):
    tgt, src, gt, T, T0, frames, cfg, ocfg = park
    base = tgt[:120_000]
    A = api.Context(0)
    try:
        A.set_target(base, RADIUS)
        expected = base
        for k in range(3):
            A.insert(frames[k], T[k])
            expected = np.concatenate([expected, transform(frames[k], T[k])])
        A.set_source(src)
        res, logs = A.icp_run(T0[4], "Ours", cfg)
    finally:
        A.close()
    ores, ologs = po.icp_run(po.KdTree(expected), src, T0[4], "Ours", ocfg)
    assert (res.iterations, res.converged, res.status) == (ores.iterations, ores.converged, ores.status)
    assert logs[-1].effective_points == ologs[-1].n_eff
    assert np.allclose(np.array(res.R[:]), ores.R[:], rtol=0, atol=1e-8) and np.allclose(np.array(res.t[:]), ores.t[:], rtol=0, atol=1e-8)
    assert h.rel_err(logs[-1].H_upper[:], ologs[-1].H_upper[:]) < 1e-7
