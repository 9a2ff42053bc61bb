"""The device seam of the C-ABI (include/dcreg.h): clouds handed over as raw device pointers (dcreg_set_target_device /
dcreg_set_source_device), at strides 3, 4 and 7 and from an unaligned start, give bitwise what the same clouds give from host buffers
(dcreg_set_target / dcreg_set_source) - index, linearisations with their per-point neighbours, ICP runs, batched frames, k-NN and the
point-to-point error - and the float64 oracle agrees with them.  The two ways a cloud's bounding box is taken (host_bounds for small
host frames, k_bounds for everything else) are compared at the small-frame limit and at the edges of a box (signed zeros, zero extent).
A caller's device buffer is consumed when the call returns; a refused cloud leaves the context as it was.

Clouds, strided rows in host arrays (api.py passes the real stride): frames and k-NN queries with extra columns.

Calls made while a linearisation is in flight (gated or not) are refused at once with DCREG_E_STATE, and the launch still gives its result.

Device memory is allocated through the HIP runtime the library is bound to (torch is not imported here: the torch cases run in child
processes, tests/test_gpu_torch_seam.py)."""
import ctypes as C
import time

import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from oracle import pyoracle as po
from test_gpu_parity import assert_debug_equal, assert_lin_equal

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2          # hipMemcpyHostToDevice, hipMemcpyDeviceToHost
_HIP = []


def hip():
    """the HIP runtime libdcreg_hip.so is bound to: after api.load() the soname resolves to the object already mapped"""
    if not _HIP:
        api.load()
        L = C.CDLL("libamdhip64.so.7")
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        for f in ("hipMalloc", "hipFree", "hipMemcpy", "hipMemset"):
            getattr(L, f).restype = C.c_int
        _HIP.append(L)
    return _HIP[0]


def strided(xyz, stride, fill=np.nan):
    """xyz in the first three columns of an [n, stride] float32 array, `fill` in the others (NaN: a stride read wrong is refused)"""
    a = np.full((len(xyz), stride), fill, np.float32)
    a[:, :3] = xyz
    return a


class DevCloud:
    """an [n, stride] float32 array copied to device memory, starting `offset` bytes into its allocation"""

    def __init__(self, a, offset=0):
        a = np.ascontiguousarray(a, np.float32)
        assert a.ndim == 2 and offset % 4 == 0
        self.n, self.stride, self.nbytes = a.shape[0], a.shape[1], a.nbytes
        p = C.c_void_p()
        assert hip().hipMalloc(C.byref(p), max(a.nbytes + offset, 4)) == 0
        self.base = p.value
        self.ptr = self.base + offset
        self.write(a)

    def write(self, a):
        a = np.ascontiguousarray(a, np.float32)
        assert a.nbytes == self.nbytes
        if a.nbytes:
            assert hip().hipMemcpy(C.c_void_p(self.ptr), C.c_void_p(a.ctypes.data), a.nbytes, H2D) == 0

    def free(self):
        if self.base:
            assert hip().hipFree(C.c_void_p(self.base)) == 0
            self.base = None


def _lin_equal(a, b):
    assert a["n_eff"] == b["n_eff"] and a["n_pt"] == b["n_pt"]
    assert np.array_equal(a["H_upper"], b["H_upper"]) and np.array_equal(a["g"], b["g"])
    assert a["sum_r2"] == b["sum_r2"] and a["sum_b2"] == b["sum_b2"]
    if "flag" in a:
        assert np.array_equal(a["flag"], b["flag"]) and np.array_equal(a["nn_idx"], b["nn_idx"])
        assert np.array_equal(a["nn_d2"].view(np.uint32), b["nn_d2"].view(np.uint32))


def _info(ctx):
    i = ctx.index_info()
    return (i.cell, tuple(i.origin), tuple(i.dims), i.n_cells, i.n_target, i.n_source)


def _icp(ctx, T0, cfg):
    res, logs = ctx.icp_run(T0, "Ours", cfg)
    return ((res.converged, res.iterations, res.status), np.array(res.R[:]), np.array(res.t[:]), np.array(res.icp_cov[:]),
            [np.array(L.H_upper[:]) for L in logs], [np.array(L.update_dx[:]) for L in logs])


def _icp_equal(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(x, y)
    assert len(a[4]) == len(b[4]) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))
    assert all(np.array_equal(x, y) for x, y in zip(a[5], b[5]))


def _snapshot(ctx, poses, q, prm, T_err):
    """everything a later call can observe of the context's clouds"""
    return dict(info=_info(ctx), lin=[ctx.linearize(T[:3, :3], T[:3, 3], prm, debug=True) for T in poses],
                knn=ctx.knn(q, 5, 0.0), p2p=ctx.p2p_error(T_err, 0.3))


def _snap_equal(a, b):
    assert a["info"] == b["info"]
    for x, y in zip(a["lin"], b["lin"]):
        _lin_equal(x, y)
    assert np.array_equal(a["knn"][0], b["knn"][0]) and np.array_equal(a["knn"][1].view(np.uint32), b["knn"][1].view(np.uint32))
    assert a["p2p"] == b["p2p"]


def _poses(T, scale=1.0):
    return [T @ h.pose6d_matrix(*(scale * np.array(d))) for d in
            ([0, 0, 0, 0, 0, 0], [0.05, -0.03, 0.02, 2e-3, -1e-3, 3e-3], [-0.2, 0.1, -0.05, -4e-3, 2e-3, 8e-3])]


CFG = dict(search_radius=1.0, max_iterations=20, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, use_weight_derivative=1, always_compute_schur=1)


@pytest.fixture(scope="module")
def parking():
    tgt, src = h.scene_parkinglot()
    return np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32), h.pose6d_matrix(**h.PK01_GT)


@pytest.fixture(scope="module")
def big():
    tgt = h.scene_planes(1_000_000, seed=21)
    rng = np.random.default_rng(4)
    src = tgt[rng.choice(len(tgt), 300_000, replace=False)] + rng.normal(0, 0.01, (300_000, 3))
    return np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32), h.pose6d_matrix(0.1, -0.05, 0.02, 1e-3, -2e-3, 3e-3)


LAYOUTS = [(3, 0), (4, 0), (7, 0), (3, 4), (7, 4)]      # (stride in floats, bytes from the start of the allocation)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["s%d+%d" % l for l in LAYOUTS])
@pytest.mark.parametrize("scene", ["parking", "big"])
def test_device_clouds_equal_host_clouds(scene, layout, request):
    """an 8 k-point frame on a 200 k map and a 300 k source on a 1 M map, both clouds as device pointers: index, three debug
    linearisations, an ICP run, k-NN and p2p error bitwise those of the host path; the map's origin is its float32 minimum"""
    tgt, src, T = request.getfixturevalue(scene)
    stride, off = layout
    prm = api.default_lin_params(1.0, 1)
    poses = _poses(T)
    q = (src[::17].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    host, dev = api.Context(0), api.Context(0)
    dt, ds = DevCloud(strided(tgt, stride), off), DevCloud(strided(src, stride), off)
    try:
        host.set_target(tgt, 1.0); host.set_source(src)
        dev.set_target_device(dt.ptr, len(tgt), stride, 1.0); dev.set_source_device(ds.ptr, len(src), stride)
        a, b = _info(host), _info(dev)
        assert a == b
        assert a[1] == tuple(float(v) for v in tgt.min(axis=0))
        want = _snapshot(host, poses, q, prm, poses[1])
        _snap_equal(_snapshot(dev, poses, q, prm, poses[1]), want)
        cfg = api.default_config(**CFG)
        _icp_equal(_icp(dev, poses[2], cfg), _icp(host, poses[2], cfg))
        if scene == "parking" and layout == (3, 0):       # and the float64 reference of the same linearisation
            ref = po.linearize(po.KdTree(tgt), src, poses[1][:3, :3], poses[1][:3, 3], po.default_lin_params(1.0, 1), debug=True)
            assert_lin_equal(want["lin"][1], ref)
            assert_debug_equal(want["lin"][1], ref)
    finally:
        host.close(); dev.close(); dt.free(); ds.free()


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 65_536, 65_537])
def test_device_sources_of_every_size(n):
    """sources around a wave (64), the small-frame limit (65 536) and a single point: stride 7 from an unaligned start against the
    host path (at stride 3, and at stride 7 too), bitwise"""
    tgt = h.scene_cylinder(120_000, seed=2, noise=0.01)
    rng = np.random.default_rng(n)
    src = (tgt[rng.choice(len(tgt), n, replace=n > len(tgt))] + rng.normal(0, 0.02, (n, 3))).astype(np.float32)
    T = h.pose6d_matrix(0.02, -0.01, 0.0, 1e-3, 0.0, -2e-3)
    prm = api.default_lin_params(1.0, 1)
    poses = _poses(T)
    q = src[:: max(1, n // 500)].copy()
    host, wide, dev = api.Context(0), api.Context(0), api.Context(0)
    ds = DevCloud(strided(src, 7), 4)
    try:
        for c in (host, wide, dev):
            c.set_target(tgt, 1.0)
        host.set_source(src)
        wide.set_source(strided(src, 7, fill=1e30))
        dev.set_source_device(ds.ptr, n, 7)
        want = _snapshot(host, poses, q, prm, poses[1])
        _snap_equal(_snapshot(wide, poses, q, prm, poses[1]), want)
        _snap_equal(_snapshot(dev, poses, q, prm, poses[1]), want)
    finally:
        host.close(); wide.close(); dev.close(); ds.free()


def test_small_host_frame_limit_and_box_edges():
    """host_bounds (a host frame of at most 65 536 points and 2^20 floats) against k_bounds (everything else): 65 536 points at
    stride 16 (exactly 2^20 floats) and 3 take the pinned block and host bounds, at stride 17 the device bounds, 65 537 points the
    device bounds; a minimum shared by -0.0 and +0.0 points (in both orders) and a cloud of one repeated point (extent 0) - every
    path bitwise the others and the device pointer"""
    tgt = h.scene_cylinder(150_000, seed=8, noise=0.01)
    rng = np.random.default_rng(12)
    T = h.pose6d_matrix(0.01, 0.02, -0.01, -1e-3, 2e-3, 1e-3)
    prm = api.default_lin_params(1.0, 1)
    poses = _poses(T)
    base = (tgt[rng.choice(len(tgt), 65_537, replace=False)] + rng.normal(0, 0.02, (65_537, 3))).astype(np.float32)
    zeros = base[:4000].copy()
    zeros[:, 0] = np.abs(zeros[:, 0] - zeros[:, 0].min())      # x >= 0 ...
    zeros[::97, 0] = 0.0                                        # ... the minimum 0, held by +0.0 and -0.0 points
    zeros[1::97, 0] = -0.0
    tgt_z = np.concatenate([tgt, zeros]).astype(np.float32)
    clouds = {"65536": base[:65_536], "65537": base, "zeros+-": zeros, "zeros-+": np.roll(zeros, -1, axis=0),
              "one point": np.repeat(base[:1], 300, axis=0)}
    for name, src in clouds.items():
        n = len(src)
        layouts = [(3, None), (16, None), (17, None)] if n == 65_536 else [(3, None), (5, None)]
        q = src[:: max(1, n // 400)].copy()
        ctxs, bufs = [], []
        try:
            for stride, _ in layouts + [(7, "dev")]:
                c = api.Context(0)
                ctxs.append(c)
                c.set_target(tgt_z, 1.0)
                a = strided(src, stride, fill=-1e30)
                if len(ctxs) == len(layouts) + 1:
                    bufs.append(DevCloud(a))
                    c.set_source_device(bufs[-1].ptr, n, stride)
                else:
                    c.set_source(a)
            want = _snapshot(ctxs[0], poses, q, prm, poses[1])
            for c in ctxs[1:]:
                _snap_equal(_snapshot(c, poses, q, prm, poses[1]), want)
        finally:
            for c in ctxs:
                c.close()
            for b in bufs:
                b.free()
    # the same edges as maps: index origin = the float32 minimum, signed zero included in ==, extent 0 gives a one-cell grid
    for name in ("zeros+-", "one point"):
        src = clouds[name]
        host, dev = api.Context(0), api.Context(0)
        d = DevCloud(strided(src, 4), 4)
        try:
            host.set_target(src, 1.0); dev.set_target_device(d.ptr, len(src), 4, 1.0)
            assert _info(host)[:4] == _info(dev)[:4]
            assert _info(host)[1] == tuple(float(v) for v in src.min(axis=0))
            q = src[::7] + np.float32(0.05)
            for c in (host, dev):
                c.set_source(src[::3].copy())
            _snap_equal(_snapshot(dev, poses, q, prm, poses[0]), _snapshot(host, poses, q, prm, poses[0]))
        finally:
            host.close(); dev.close(); d.free()


def test_device_buffers_are_consumed_when_the_call_returns(parking):
    """dcreg.h: the caller's buffer is consumed when the call returns - overwriting the device buffers with another valid cloud at
    once changes no later result"""
    tgt, src, T = parking
    other = (src * np.float32(0.5) + np.float32(3.0)).astype(np.float32)
    prm = api.default_lin_params(1.0, 1)
    poses = _poses(T)
    q = src[::13].copy()
    host, dev = api.Context(0), api.Context(0)
    dt, ds = DevCloud(strided(tgt, 4)), DevCloud(strided(src, 4))
    try:
        host.set_target(tgt, 1.0); host.set_source(src)
        dev.set_target_device(dt.ptr, len(tgt), 4, 1.0)
        dt.write(strided(tgt[::-1] + np.float32(7.0), 4))
        dev.set_source_device(ds.ptr, len(src), 4)
        ds.write(strided(other, 4))
        _snap_equal(_snapshot(dev, poses, q, prm, poses[1]), _snapshot(host, poses, q, prm, poses[1]))
        cfg = api.default_config(**CFG)
        _icp_equal(_icp(dev, poses[2], cfg), _icp(host, poses[2], cfg))
    finally:
        host.close(); dev.close(); dt.free(); ds.free()


def test_refused_device_clouds_leave_the_context_unchanged(parking):
    """a null pointer, stride 2, n = 0 and a non-finite coordinate on each axis (k_bounds' check) are refused, for the map and the
    source alike, and the context gives bitwise what it gave before - the refused cloud is not half taken"""
    tgt, src, T = parking
    prm = api.default_lin_params(1.0, 1)
    poses = _poses(T)
    q = src[::13].copy()
    ctx = api.Context(0)
    dt, ds = DevCloud(strided(tgt, 4)), DevCloud(strided(src, 4))
    bad = []
    try:
        ctx.set_target_device(dt.ptr, len(tgt), 4, 1.0); ctx.set_source_device(ds.ptr, len(src), 4)
        before = _snapshot(ctx, poses, q, prm, poses[1])
        for set_target in (True, False):
            cloud, buf = (tgt, dt) if set_target else (src, ds)

            def put(ptr, n, stride):
                if set_target:
                    ctx.set_target_device(ptr, n, stride, 1.0)
                else:
                    ctx.set_source_device(ptr, n, stride)
            for args in ((0, len(cloud), 4), (buf.ptr, len(cloud), 2), (buf.ptr, 0, 4)):
                with pytest.raises(api.DcregError):
                    put(*args)
            for axis in range(3):
                for v in (np.nan, np.inf, -np.inf):
                    a = strided(cloud, 4)
                    a[len(a) // 3, axis] = v
                    bad.append(DevCloud(a))
                    with pytest.raises(api.DcregError, match="non-finite"):
                        put(bad[-1].ptr, len(a), 4)
            _snap_equal(_snapshot(ctx, poses, q, prm, poses[1]), before)
        cfg = api.default_config(**CFG)
        ref = api.Context(0)
        ref.set_target(tgt, 1.0); ref.set_source(src)
        _icp_equal(_icp(ctx, poses[2], cfg), _icp(ref, poses[2], cfg))
        ref.close()
    finally:
        ctx.close(); dt.free(); ds.free()
        for b in bad:
            b.free()


def test_frames_on_a_device_map_and_strided_host_clouds(parking):
    """register_frames against a map set from a device pointer is bitwise the host map's; frames and k-NN queries with 4 or 8 columns
    (garbage beyond x y z) are passed with their stride and give bitwise the [N, 3] array's records and neighbour lists"""
    tgt, _, T = parking
    rng = np.random.default_rng(7)
    Ts = [T @ h.pose6d_matrix(*rng.uniform(-5, 5, 2), 0.0, 0.0, 0.0, h.deg2rad(rng.uniform(-15, 15))) for _ in range(6)]
    frames = h.map_frames(tgt, Ts, [8000, 300, 5000, 64, 2000, 65], seed=2)
    T0 = [Tk @ h.pose6d_matrix(*rng.uniform(-0.1, 0.1, 3), *h.deg2rad(rng.uniform(-0.4, 0.4, 3))) for Tk in Ts]
    cfg = api.default_config(**CFG)
    host, dev = api.Context(0), api.Context(0)
    dt = DevCloud(strided(tgt, 7), 4)
    try:
        host.set_target(tgt, 1.0)
        dev.set_target_device(dt.ptr, len(tgt), 7, 1.0)
        want = host.register_frames(frames, T0, "Ours", cfg, slots=4)
        xyz = np.concatenate(frames)
        off = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
        q = (xyz[::11].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        qi, qd = host.knn(q, 5, 0.0)
        got = [dev.register_frames(frames, T0, "Ours", cfg, slots=4)]
        for cols in (4, 8):
            wide = [np.concatenate([f, rng.uniform(-1e6, 1e6, (len(f), cols - 3)).astype(np.float32)], 1) for f in frames]
            wide[0][::5, 3] = np.nan
            got.append(host.register_frames(wide, T0, "Ours", cfg, slots=4))
            got.append(host.register_frames((np.concatenate(wide), off), T0, "Ours", cfg, slots=3))
            qw = strided(q, cols, fill=np.nan)
            for c in (host, dev):
                i, d = c.knn(qw, 5, 0.0)
                assert np.array_equal(i, qi) and np.array_equal(d.view(np.uint32), qd.view(np.uint32))
            i, d, _ = host.knn_timed(qw, 5, 0.0, "grid", repeats=1)
            assert np.array_equal(i, qi) and np.array_equal(d.view(np.uint32), qd.view(np.uint32))
        for recs in got:
            for a, b in zip(recs, want):
                assert (a.iterations, a.converged, a.status, a.corr_num) == (b.iterations, b.converged, b.status, b.corr_num)
                assert np.array_equal(np.array(a.final_transform[:]), np.array(b.final_transform[:]))
                assert a.final_rmse == b.final_rmse and a.final_fitness == b.final_fitness
                assert np.array_equal(np.array(a.H_upper[:]), np.array(b.H_upper[:]))
    finally:
        host.close(); dev.close(); dt.free()


def test_calls_while_a_linearisation_is_in_flight_are_refused():
    """while a gated launch waits for its pose, or an ungated one is in flight, every entry point that would queue behind it, wait for
    the stream or replace what it reads returns DCREG_E_STATE at once (a waiting gate would otherwise hold each of them for its
    two-minute give-up); the launch then gives bitwise the blocking result, and after a gate is called off the same calls succeed"""
    tgt = h.scene_cylinder(100_000, seed=5, noise=0.01)
    src = tgt[::4].copy()
    prm = api.default_lin_params(1.0, 1)
    T0, T1 = h.pose6d_matrix(0.02, 0.0, 0.01, 0.0, 1e-3, 0.0), h.pose6d_matrix(0.05, -0.02, 0.01, 1e-3, 0.0, -2e-3)
    ref = api.Context(0)
    ref.set_target(tgt, 1.0); ref.set_source(src)
    ref.linearize(T0[:3, :3], T0[:3, 3], prm)
    want = ref.linearize(T1[:3, :3], T1[:3, 3], prm)
    ref.close()
    ctx = api.Context(0)
    dt = DevCloud(strided(tgt, 3))
    q = src[::9].copy()
    L = api.load()
    stamps = np.zeros((4096, 8), np.uint64)
    try:
        ctx.set_option("count_searches", 1)
        ctx.set_option("team_stamps", 1)
        ctx.set_target(tgt, 1.0); ctx.set_source(src)
        ctx.linearize(T0[:3, :3], T0[:3, 3], prm)
        have_stamps = L.dcreg_team_pass_stamps(ctx._h, None, 0) > 0

        def raw_stamps():
            rc = L.dcreg_team_pass_stamps(ctx._h, stamps.ctypes.data_as(C.POINTER(C.c_uint64)), len(stamps))
            if rc < 0:
                raise api.DcregError("dcreg_team_pass_stamps failed (%d): %s" % (rc, L.dcreg_last_error(ctx._h).decode()))
        calls = [("set_target", lambda: ctx.set_target(tgt, 1.0)),
                 ("set_target_device", lambda: ctx.set_target_device(dt.ptr, len(tgt), 3, 1.0)),
                 ("set_source", lambda: ctx.set_source(src)),
                 ("set_source_device", lambda: ctx.set_source_device(dt.ptr, len(src), 3)),
                 ("set_stream", lambda: ctx.set_stream(0)),
                 ("knn", lambda: ctx.knn(q, 5, 0.0)),
                 ("knn_timed", lambda: ctx.knn_timed(q, 5, 0.0, "grid", repeats=1)),
                 ("kdtree_build", lambda: ctx.kdtree_build(16)),
                 ("p2p_error", lambda: ctx.p2p_error(T0, 0.3)),
                 ("launch_stats", lambda: ctx.launch_stats()),
                 ("reserve_warm_states", lambda: ctx.reserve_warm_states(2)),
                 ("reset_warm_state", lambda: ctx.reset_warm_state(-1))]
        if have_stamps:
            calls.append(("team_pass_stamps", raw_stamps))

        def refused():
            for name, call in calls:
                t = time.perf_counter()
                with pytest.raises(api.DcregError, match=r"\(-4\)"):
                    call()
                assert time.perf_counter() - t < 1.0, name
            # readers of host state stay allowed
            ctx.index_info(); ctx.roi_info(); ctx.launch_series(reset=False); ctx.kernel_time(); ctx.hint_misalignment(0.1)

        ctx.linearize_gated_begin(prm, slot=1)
        refused()
        ctx.gate_open(T1[:3, :3], T1[:3, 3])
        _lin_equal(ctx.linearize_end(slot=1), want)

        ctx.linearize_gated_begin(prm, slot=0)
        refused()
        ctx.gate_abort()
        for name, call in calls:
            call()
        ctx.set_target(tgt, 1.0); ctx.set_source(src)
        ctx.linearize(T0[:3, :3], T0[:3, 3], prm)
        _lin_equal(ctx.linearize(T1[:3, :3], T1[:3, 3], prm), want)

        ctx.linearize_begin(T1[:3, :3], T1[:3, 3], prm, slot=0)
        refused()
        _lin_equal(ctx.linearize_end(slot=0), want)
    finally:
        ctx.close(); dt.free()
