"""Voxel-grid downsampling on the device (dcreg_voxel_downsample*, dcreg_set_source_voxel*, dcreg_set_target_voxel*).  The numpy reference
below implements the header's rules literally: finite points only, v = floor((double)p / leaf), voxels in (v_z, v_y, v_x) order with the
points of a voxel in input order (np.lexsort), voxels under min_points dropped, the centroid as the left-to-right double sum of the voxel's
points divided by their count (or the first point, bit for bit).  Every output is compared bitwise, and a context given a voxelised cloud
answers bitwise as one given the reference cloud through the plain calls."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from test_gpu_configs import cfg_pair
from test_gpu_device_seam import DevCloud, hip, strided
from test_gpu_frames import _frame_poses

pytestmark = pytest.mark.gpu

D2H = 2
ZERO = {"points": 0, "table": 0, "row_words": 0, "gap": 0, "owner": 0}


def voxel_ref(xyz, leaf, mode="centroid", min_points=1):
    """the header's rules, literally -> [m, 3] float32"""
    p = np.asarray(xyz, np.float32)[:, :3]
    leaf = np.broadcast_to(np.asarray(leaf, np.float64), (3,))
    idx = np.flatnonzero(np.all(np.isfinite(p), 1))
    v = np.floor(p[idx].astype(np.float64) / leaf).astype(np.int64)
    order = np.lexsort((idx, v[:, 0], v[:, 1], v[:, 2]))
    vs, ids = v[order], idx[order]
    if len(ids) == 0:
        return np.zeros((0, 3), np.float32)
    new = np.r_[True, np.any(vs[1:] != vs[:-1], 1)]
    starts = np.flatnonzero(new)
    counts = np.diff(np.r_[starts, len(ids)])
    if mode == "first":
        out = p[ids[starts]].copy()
    else:
        s = p[ids[starts]].astype(np.float64)
        for k in range(1, int(counts.max())):        # left to right within every voxel: point k of each voxel that has one
            m = counts > k
            s[m] += p[ids[starts[m] + k]].astype(np.float64)
        out = (s / counts[:, None].astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(out[counts >= max(min_points, 1)])


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def parking():
    tgt, src = h.scene_parkinglot()
    return tgt, src, h.pose6d_matrix(**h.PK01_GT), h.pose6d_matrix(**h.PK01_INIT)


@pytest.fixture(scope="module")
def sweep(parking):
    tgt, _, gt, _ = parking
    s = h.lidar_sweep(tgt, gt, seed=3)
    assert s.shape == (131072, 3) and np.isnan(s[:, 0]).any()
    return s


def boundary_cloud():
    """points on exact voxel boundaries (multiples of the leaf 0.25, exact in binary), negative coordinates, +-0.0 and duplicates"""
    g = np.arange(-8, 9, dtype=np.float32) * np.float32(0.25)
    x, y, z = np.meshgrid(g, g[::3], g[::4], indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    zeros = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, -0.0], [-1e-30, 0.0, 1e-30]], np.float32)
    rng = np.random.default_rng(5)
    jit = (rng.uniform(-1, 1, (500, 3)) * 2).astype(np.float32)
    cloud = np.concatenate([pts, zeros, jit, pts[::7], jit[::3], np.nextafter(pts[::5], np.float32(-np.inf))], 0)
    return cloud[rng.permutation(len(cloud))]


def cases(parking, sweep):
    tgt, src, _, _ = parking
    return {"cylinder": h.cylinder_cloud(), "sweep": sweep, "boundary": boundary_cloud(), "frame": src, "map": tgt}


@pytest.mark.parametrize("name,leaf", [("cylinder", 0.3), ("sweep", 0.2), ("sweep", [0.1, 0.3, 0.05]), ("boundary", 0.25),
                                       ("boundary", [0.25, 0.5, 0.125]), ("frame", 0.5), ("map", [0.4, 0.4, 0.1])])
@pytest.mark.parametrize("mode", ["centroid", "first"])
def test_bitwise_equal_to_the_reference(ctx, parking, sweep, name, leaf, mode):
    cloud = cases(parking, sweep)[name]
    for mp in (1, 3, 10):
        out, info = ctx.voxel_downsample([cloud], leaf, mode, min_points=mp)
        ref = voxel_ref(cloud, leaf, mode, mp)
        assert same(out[0], ref), (name, leaf, mode, mp, out[0].shape, ref.shape)
        fin = int(np.all(np.isfinite(cloud), 1).sum())
        assert info["n_in"] == len(cloud) and info["n_finite"] == fin and info["n_out"] == len(ref)
        assert info["n_voxels"] == len(voxel_ref(cloud, leaf, "first", 1))


def test_a_batch_is_the_concatenation_of_its_clouds(ctx, parking, sweep):
    """empty and all-NaN clouds among others; one call and cloud-by-cloud calls agree bit for bit, and a repeated call too.  The second
    batch holds clouds of wide spans, so that cloud + voxel key bits exceed 64 and the two-sort order serves"""
    tgt, src, _, _ = parking
    nan = np.full((300, 3), np.nan, np.float32)
    clouds = [h.cylinder_cloud(), np.zeros((0, 3), np.float32), sweep, nan, boundary_cloud(), src, np.zeros((0, 3), np.float32), sweep[::-1]]
    rng = np.random.default_rng(9)
    cubes = [rng.uniform(0.0, 100.0, (4000, 3)).astype(np.float32) for _ in range(40)]
    wide = [np.concatenate([c, c[:1500]]) for c in cubes] + [nan]      # 1e6 voxels per axis at 0.1 mm: 60 key bits + 6 cloud bits
    for batch, leaf in ((clouds, 0.2), (wide, 1e-4)):
        for mode in ("centroid", "first"):
            got, info = ctx.voxel_downsample(batch, leaf, mode, min_points=2)
            again, info2 = ctx.voxel_downsample(batch, leaf, mode, min_points=2)
            assert info == info2 and all(same(a, b) for a, b in zip(got, again))
            n_out = 0
            for cl, g in zip(batch, got):
                one, _ = ctx.voxel_downsample([cl], leaf, mode, min_points=2)
                assert same(g, one[0]) and same(g, voxel_ref(cl, leaf, mode, 2))
                n_out += len(g)
            assert info["n_out"] == n_out and info["n_in"] == sum(len(c) for c in batch)
            (xyz, off), _ = ctx.voxel_downsample(((np.concatenate(batch), np.r_[0, np.cumsum([len(c) for c in batch])])), leaf, mode, min_points=2)
            assert same(xyz, np.concatenate(got)) and list(np.diff(off)) == [len(g) for g in got]


def _hip_stream():
    L = hip()
    s = C.c_void_p()
    L.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    L.hipStreamDestroy.argtypes = [C.c_void_p]
    assert L.hipStreamCreate(C.byref(s)) == 0
    return s.value


def _read(ptr, n):
    out = np.empty((n, 3), np.float32)
    if n:
        assert hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), out.nbytes, D2H) == 0
    return out


def test_device_variants_give_the_host_bits(parking, sweep):
    """strided xyzi rows from an unaligned start, on the context's own stream and on a caller's stream"""
    tgt, src, gt, T0 = parking
    cfg, _ = cfg_pair(1.0, 30, 1)
    clouds = [sweep, boundary_cloud(), np.full((7, 3), np.nan, np.float32), h.cylinder_cloud()]
    off = np.r_[0, np.cumsum([len(c) for c in clouds])]
    allp = np.concatenate(clouds)
    xyzi = strided(allp, 4, fill=7.0)
    stream = _hip_stream()
    for use_stream in (False, True):
        a, b = api.Context(0), api.Context(0)
        dev = DevCloud(xyzi, offset=12)
        out = DevCloud(np.zeros((len(allp), 3), np.float32))
        try:
            if use_stream:
                a.set_stream(stream)
            for mode in ("centroid", "first"):
                (hx, hoff), hinfo = b.voxel_downsample((xyzi, off), 0.2, mode, 2)
                doff, dinfo = a.voxel_downsample_device(dev.ptr, off, 4, out.ptr, len(allp), 0.2, mode, 2)
                assert dinfo == hinfo and np.array_equal(doff, hoff) and same(_read(out.ptr, int(doff[-1])), hx)
            sw = DevCloud(strided(sweep, 4, fill=7.0), offset=4)
            try:
                assert a.set_source_voxel_device(sw.ptr, len(sweep), 4, 0.2) == b.set_source_voxel(strided(sweep, 4, fill=7.0), 0.2)
                a.set_target_voxel_device(dev.ptr, len(clouds[0]), 4, 1.0, [0.3, 0.3, 0.1])
                b.set_target_voxel(xyzi[:len(clouds[0])], 1.0, [0.3, 0.3, 0.1])
            finally:
                sw.free()
            assert same(a.target_points(), b.target_points())
            assert _run(a, np.eye(4), cfg) == _run(b, np.eye(4), cfg)
        finally:
            dev.free(); out.free(); a.close(); b.close()
    hip().hipStreamDestroy(C.c_void_p(stream))


def _run(ctx, T0, cfg):
    """what a registration returns: converged, iterations, status, R, t, the covariance, and every iteration's H_upper"""
    res, logs = ctx.icp_run(T0, "Ours", cfg)
    return (res.converged, res.iterations, res.status, tuple(res.R[:]), tuple(res.t[:]), tuple(res.icp_cov[:]),
            [tuple(L.H_upper[:]) for L in logs])


def test_set_source_voxel_is_set_source_of_the_reference(parking, sweep):
    tgt, src, gt, T0 = parking
    cfg, _ = cfg_pair(1.0, 30, 1)
    for leaf, mode in ((0.2, "centroid"), ([0.15, 0.15, 0.3], "first")):
        a, b = api.Context(0), api.Context(0)
        try:
            for c in (a, b):
                c.set_target(tgt, 1.0)
            info = a.set_source_voxel(sweep, leaf, mode)
            ref = voxel_ref(sweep, leaf, mode)
            assert info["n_out"] == len(ref)
            b.set_source(ref)
            ra = _run(a, T0, cfg)
            assert ra == _run(b, T0, cfg)
            assert a.p2p_error(T0, 0.3) == b.p2p_error(T0, 0.3)
            ia, da = a.knn(ref[:500], k=5, max_radius=1.0)
            ib, db = b.knn(ref[:500], k=5, max_radius=1.0)
            assert np.array_equal(ia, ib) and same(da, db)
        finally:
            a.close(); b.close()


def test_set_target_voxel_is_set_target_of_the_reference(parking):
    tgt, src, gt, T0 = parking
    cfg, _ = cfg_pair(1.0, 30, 1)
    leaf = [0.3, 0.3, 0.05]
    ref = voxel_ref(tgt, leaf)
    a, b = api.Context(0), api.Context(0)
    try:
        info = a.set_target_voxel(tgt, 1.0, leaf)
        b.set_target(ref, 1.0)
        assert info["n_out"] == len(ref) and same(a.target_points(), ref) and a.index_check() == ZERO
        for c in (a, b):
            c.set_source(src)
        assert _run(a, T0, cfg) == _run(b, T0, cfg)
        for c in (a, b):
            c.insert_source(gt, 0.05)
            c.crop(gt[:3, 3] - 25.0, gt[:3, 3] + 25.0)
        assert same(a.target_points(), b.target_points()) and a.index_check() == ZERO
        assert _run(a, T0, cfg) == _run(b, T0, cfg)
    finally:
        a.close(); b.close()


def test_the_batched_output_feeds_register_frames(parking):
    tgt, src, gt, _ = parking
    cfg, _ = cfg_pair(1.0, 30, 1)
    T, T0 = _frame_poses(gt, 6, seed=4, step=4.0)
    sweeps = [h.lidar_sweep(tgt, Tk, seed=k) for k, Tk in enumerate(T)]
    a = api.Context(0)
    try:
        a.set_target(tgt, 1.0)
        (xyz, off), _ = a.voxel_downsample((np.concatenate(sweeps), np.r_[0, np.cumsum([len(s) for s in sweeps])]), 0.2)
        refs = [voxel_ref(s, 0.2) for s in sweeps]
        recs = a.register_frames((xyz, off), np.stack(T0), "Ours", cfg, slots=4)
        want = a.register_frames(refs, np.stack(T0), "Ours", cfg, slots=4)
        key = lambda r: (r.iterations, r.converged, r.status, tuple(r.final_transform[:]), r.final_rmse, r.corr_num, tuple(r.H_upper[:]))
        assert [key(r) for r in recs] == [key(r) for r in want]
    finally:
        a.close()


def test_refusals_leave_the_context_untouched(parking, sweep):
    tgt, src, gt, T0 = parking
    cfg, _ = cfg_pair(1.0, 30, 1)
    L = api.load()
    a = api.Context(0)
    try:
        a.set_target(tgt, 1.0)
        a.set_source(src)
        before = _run(a, T0, cfg)
        map_before = a.target_points()
        nan = np.full_like(sweep, np.nan)
        far = np.array([[0, 0, 0], [21000.0, 0, 0]], np.float32)                # 2.1 M voxels on x at a 1 cm leaf: at least 2^21
        bad = api.voxel_params(0.2)
        bad.leaf[1] = 0.0                                                       # (past the Python checks: the library refuses too)
        x = np.ascontiguousarray(sweep)
        info = api.VoxelInfo()
        assert L.dcreg_set_source_voxel(a._h, x.ctypes.data, len(x), 3, C.byref(bad), C.byref(info)) == api.E_INVALID
        assert L.dcreg_set_target_voxel(a._h, x.ctypes.data, len(x), 3, C.byref(bad), 1.0, C.byref(info)) == api.E_INVALID
        for cloud, leaf in ((nan, 0.2), (far, 0.01)):
            with pytest.raises(api.DcregError):
                a.set_source_voxel(cloud, leaf)
            with pytest.raises(api.DcregError):
                a.set_target_voxel(cloud, 1.0, leaf)
        assert same(a.target_points(), map_before) and a.index_check() == ZERO
        assert _run(a, T0, cfg) == before
        # a short capacity: the needed offsets and info, nothing written
        clouds = [sweep, h.cylinder_cloud()]
        xyz = np.ascontiguousarray(np.concatenate(clouds))
        off = np.array([0, len(sweep), len(xyz)], np.int64)
        (want, want_off), want_info = a.voxel_downsample((xyz, off), 0.2)
        out = np.full((len(want) - 1, 3), 7.0, np.float32)
        out_off = np.zeros(3, np.int64)
        p = api.voxel_params(0.2)
        i64p = C.POINTER(C.c_int64)
        rc = L.dcreg_voxel_downsample(a._h, 2, xyz.ctypes.data, off.ctypes.data_as(i64p), 3, C.byref(p), out.ctypes.data, len(out),
                                      out_off.ctypes.data_as(i64p), C.byref(info))
        assert rc == api.E_INVALID and np.array_equal(out_off, want_off) and api._voxel_info_dict(info) == want_info
        assert np.all(out == 7.0)
        assert _run(a, T0, cfg) == before
    finally:
        a.close()
