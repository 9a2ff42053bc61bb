"""Motion compensation on the device (dcreg_deskew*, dcreg_set_source_deskew*).  The numpy reference below applies include/dcreg.h's rule
literally - the stamp decoded from the record's raw words, tau = (s - t_begin) / (t_end - t_begin), a = tau - ref, p' = (float)(R p + t) with
(R, t) = Exp(a xi) and xi = Log(motion), NaN for a non-finite point, a bitwise copy where a xi is zero - and the device must agree to one
float ulp (device and numpy sin / cos may differ in the last double bit).  Everything the deskew feeds (voxel pass, source, registration,
map insert, batched frames) is compared bitwise with the plain calls given the deskewed cloud."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from test_api_deskew_args import exp_ref, log_ref
from test_gpu_configs import cfg_pair
from test_gpu_device_seam import DevCloud, _icp, _icp_equal, _lin_equal, _poses, hip
from test_gpu_voxel import _hip_stream, _read, same

pytestmark = pytest.mark.gpu

TYPES = ("f32", "f64", "u32", "u64")
SCALE = {"f32": 1.0, "f64": 1.0, "u32": 1e-6, "u64": 1e-9}
EPOCH = {"f32": 0.0, "f64": 1.7e9, "u32": 1000.0, "u64": 1.7e9}        # seconds at stamp 0.0 of a sweep, per type
MOTIONS = {"translation": [0, 0, 0, 1.0, 0.2, 0.0], "rotation": [0.01, -0.02, 0.05, 0, 0, 0],
           "under series": [2e-4, -1e-4, 3e-4, 0.3, 0.1, 0.0], "fast vehicle": [0.002, -0.001, 0.052, 1.0, 0.05, 0.01]}


def write_stamps(rec, column, type, seconds):
    """the stamps (seconds) into float slot `column` of float32 records, as `type` with SCALE[type] seconds per unit"""
    w = rec.view(np.uint32)
    if type == "f32":
        rec[:, column] = seconds.astype(np.float32)
    elif type == "u32":
        w[:, column] = np.round(seconds / SCALE[type]).astype(np.uint32)
    else:
        u = (seconds.astype(np.float64).view(np.uint64) if type == "f64" else np.round(seconds / SCALE[type]).astype(np.uint64))
        w[:, column] = (u & 0xFFFFFFFF).astype(np.uint32)
        w[:, column + 1] = (u >> 32).astype(np.uint32)


def stamps_of(rec, column, type, scale):
    w = np.ascontiguousarray(rec).view(np.uint32)
    lo = w[:, column]
    if type == "f32":
        v = lo.view(np.float32).astype(np.float64)
    elif type == "u32":
        v = lo.astype(np.float64)
    else:
        u = lo.astype(np.uint64) | (w[:, column + 1].astype(np.uint64) << np.uint64(32))
        v = u.view(np.float64) if type == "f64" else u.astype(np.float64)
    return scale * v


def deskew_ref(rec, column, type, scale, T, span, ref):
    """the header's rule, literally, for one cloud -> [n, 3] float32"""
    p = rec[:, :3].astype(np.float64)
    s = stamps_of(rec, column, type, scale)
    fin = np.all(np.isfinite(p), 1) & np.isfinite(s)
    if span is None:
        tb, te = (s[fin].min(), s[fin].max()) if fin.any() else (0.0, 0.0)
    else:
        tb, te = span
    xi = log_ref(T)
    out = np.full((len(rec), 3), np.nan, np.float32)
    for i in np.flatnonzero(fin):
        a = (s[i] - tb) / (te - tb) - ref if te - tb > 0 else 0.0
        if np.all(a * xi == 0.0):
            out[i] = rec[i, :3]
        else:
            E = exp_ref(a * xi)
            out[i] = (E[:3, :3] @ p[i] + E[:3, 3]).astype(np.float32)
    return out


def ulps(a, b):
    """distance in float32 ulps of two arrays with NaN in the same places (NaN pairs count 0)"""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    return np.where(nan, 0, np.abs(ordered(a) - ordered(b)))


def records(n, stride, column, type, seconds, seed, nan_rows=True):
    rng = np.random.default_rng(seed)
    rec = np.full((n, stride), 7.0, np.float32)
    rec[:, :3] = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    if nan_rows:
        rec[rng.choice(n, n // 20, replace=False), rng.integers(0, 3)] = np.nan
    write_stamps(rec, column, type, seconds)
    if nan_rows and type in ("f32", "f64"):          # non-finite stamps
        bad = rng.choice(n, 6, replace=False)
        r = rec[bad]
        write_stamps(r, column, type, np.array([np.nan, np.inf, -np.inf] * 2))
        rec[bad] = r
    return rec


def sweep_seconds(n, type, rng, outside):
    """stamps over a 0.1 s sweep starting at EPOCH[type], quantised to the type's unit; a few beyond the span on both sides"""
    s = np.sort(rng.uniform(0.0, 0.1, n))
    if outside:
        s[:7] = rng.uniform(-0.02, 0.0, 7)
        s[-7:] = rng.uniform(0.1, 0.12, 7)
    s = EPOCH[type] + s
    if type != "f32" and type != "f64":
        s = np.round(s / SCALE[type]) * SCALE[type]
    return s


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


LAYOUTS = [(4, 3), (6, 3), (6, 4), (6, 5), (8, 3), (8, 4), (8, 5), (8, 6), (9, 3), (9, 4), (9, 5), (9, 6)]


@pytest.mark.parametrize("type", TYPES)
@pytest.mark.parametrize("from_data", [False, True], ids=["given span", "data span"])
def test_deskew_agrees_with_the_rule(ctx, type, from_data):
    """every stamp type, columns 3 - 6 in strides 4, 6, 8, 9; the four motions at ref 0, 0.5, 1 as the clouds of one call; stamps beyond
    the span (given spans); NaN coordinates and stamps -> within one float ulp of the reference, NaN in the same places"""
    wide = type in ("f64", "u64")
    rng = np.random.default_rng(11)
    worst = 0
    for stride, column in LAYOUTS:
        if wide and column + 1 >= stride:
            continue
        clouds, motions, refs = [], [], []
        for k, (name, xi) in enumerate(MOTIONS.items()):
            for ref in (0.0, 0.5, 1.0):
                secs = sweep_seconds(300, type, rng, outside=not from_data)
                clouds.append(records(300, stride, column, type, secs, seed=len(clouds) + 100 * stride + column))
                span = None if from_data else (EPOCH[type], EPOCH[type] + 0.1)
                motions.append((exp_ref(np.array(xi)), span, ref))
        f = api.time_field(column, type, SCALE[type])
        ms = [api.sweep_motion(T[:3, :3], T[:3, 3], span, ref) for T, span, ref in motions]
        out, info, vinfo = ctx.deskew(clouds, f, ms)
        assert vinfo is None and info["n_in"] == sum(len(c) for c in clouds)
        n_fin = n_out = 0
        for c, o, (T, span, ref) in zip(clouds, out, motions):
            r = deskew_ref(c, column, type, SCALE[type], T, span, ref)
            worst = max(worst, int(ulps(o, r).max()))
            s = stamps_of(c, column, type, SCALE[type])
            fin = np.all(np.isfinite(c[:, :3]), 1) & np.isfinite(s)
            n_fin += int(fin.sum())
            if span is not None:
                n_out += int(np.sum(fin & ((s < span[0]) | (s > span[1]))))
        assert info["n_finite"] == n_fin and info["n_outside"] == n_out
        if from_data:
            assert n_out == 0
    assert worst <= 1, worst


def test_zero_motions_copy_the_points_bit_for_bit(ctx):
    """an identity motion, a zero-length span and stamps at the reference instant give the input bits back, -0.0 included"""
    rng = np.random.default_rng(2)
    n = 400
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = rng.uniform(-30, 30, (n, 3)).astype(np.float32)
    rec[:50, :3] = -0.0
    rec[50:60, 1] = -0.0
    rec[:, 3] = rng.uniform(0.0, 0.1, n).astype(np.float32)
    M = exp_ref(np.array(MOTIONS["fast vehicle"]))
    f = api.time_field(3)
    te = float(np.float32(0.1))                 # (float32 0.05 is exactly half of it)
    ident = api.sweep_motion(np.eye(3), np.zeros(3), (0.0, te), 0.3)
    zero_span = api.sweep_motion(M[:3, :3], M[:3, 3], (0.05, 0.05), 0.5)
    cases = [(rec, ident), (rec, zero_span)]
    for ref, s in ((0.0, 0.0), (0.5, 0.05), (1.0, 0.1)):          # every stamp at the reference instant
        r = rec.copy()
        r[:, 3] = np.float32(s)
        cases.append((r, api.sweep_motion(M[:3, :3], M[:3, 3], (0.0, te), ref)))
    r = rec.copy()
    r[:, 3] = np.float32(0.04)
    cases.append((r, api.sweep_motion(M[:3, :3], M[:3, 3], None, 0.5)))     # a data span of one instant
    for r, m in cases:
        out, info, _ = ctx.deskew([r], f, [m])
        assert same(out[0], r[:, :3])
        assert np.array_equal(np.signbit(out[0]), np.signbit(r[:, :3]))


def _mixed_batch(rng):
    """clouds of different motions, spans, kinds of span and stamp ranges, with empty clouds among them"""
    clouds, ms = [], []
    for k in range(9):
        n = 0 if k in (2, 6) else int(rng.integers(1, 3000))
        secs = rng.uniform(-0.01, 0.11, n) + k
        rec = records(n, 6, 4, "f64", secs, seed=k) if n else np.zeros((0, 6), np.float32)
        xi = list(MOTIONS.values())[k % 4]
        T = exp_ref(np.array(xi) * (1 + 0.1 * k))
        span = None if k % 3 == 0 else (k + 0.0, k + 0.1 * (k % 2))
        clouds.append(rec)
        ms.append(api.sweep_motion(T[:3, :3], T[:3, 3], span, (0.0, 0.5, 1.0)[k % 3]))
    return clouds, ms


def test_each_cloud_of_a_batch_is_its_own_call(ctx):
    """a cloud's output depends on its own records and motion only: bitwise its single-cloud call, empty clouds included"""
    clouds, ms = _mixed_batch(np.random.default_rng(7))
    f = api.time_field(4, "f64")
    out, info, _ = ctx.deskew(clouds, f, ms)
    n_fin = 0
    for c, m, o in zip(clouds, ms, out):
        one, i1, _ = ctx.deskew([c], f, [m])
        assert same(o, one[0]) and len(o) == len(c)
        n_fin += i1["n_finite"]
    assert info["n_finite"] == n_fin
    (xyz, off), _, _ = ctx.deskew((np.concatenate(clouds), np.r_[0, np.cumsum([len(c) for c in clouds])]), f, ms)
    assert same(xyz, np.concatenate(out)) and np.array_equal(off, np.r_[0, np.cumsum([len(c) for c in clouds])])


@pytest.mark.parametrize("mode,min_points", [("centroid", 1), ("first", 1), ("centroid", 3)])
def test_a_voxel_block_gives_the_voxel_pass_of_the_deskewed_clouds(ctx, mode, min_points):
    clouds, ms = _mixed_batch(np.random.default_rng(8))
    f = api.time_field(4, "f64")
    plain, info, _ = ctx.deskew(clouds, f, ms)
    vox, info_v, vinfo = ctx.deskew(clouds, f, ms, leaf=[2.0, 2.0, 1.0], mode=mode, min_points=min_points)
    ref, rinfo = ctx.voxel_downsample(plain, [2.0, 2.0, 1.0], mode, min_points)
    assert vinfo == rinfo and info_v == info
    assert all(same(a, b) for a, b in zip(vox, ref))


@pytest.fixture(scope="module")
def parking():
    tgt, _ = h.scene_parkinglot()
    gt = h.pose6d_matrix(**h.PK01_GT)
    M = exp_ref(np.array(MOTIONS["fast vehicle"]))
    rec, T_ref = h.lidar_sweep_moving(tgt, gt, M, 0.1, rings=32, cols=1024, seed=5)
    return tgt, gt, M, rec, T_ref


def _source_checks(ctx, T_ref, cfg, prm):
    lins = [ctx.linearize(T[:3, :3], T[:3, 3], prm) for T in _poses(T_ref)]
    return lins, _icp(ctx, T_ref @ h.pose6d_matrix(0.1, -0.05, 0.0, 0.0, 0.0, 0.01), cfg)


@pytest.mark.parametrize("leaf", [None, 0.3], ids=["no voxel", "voxel"])
def test_set_source_deskew_is_set_source_of_the_deskewed_sweep(parking, leaf):
    """host and device forms (strided records from an unaligned start, the caller's stream): linearisations, a whole registration and the
    map after insert_source are bitwise what the plain calls give for the deskew output"""
    tgt, gt, M, rec, T_ref = parking
    if leaf is None:
        rec = rec[np.all(np.isfinite(rec[:, :3]), 1)]          # (a NaN point refuses the no-voxel call, as dcreg_set_source)
    f = api.time_field(3)
    m = api.sweep_motion(M[:3, :3], M[:3, 3], (0.0, 0.1), 0.5)
    cfg, _ = cfg_pair(1.0, 20, 1)
    prm = api.default_lin_params(1.0, 1)
    ref_ctx = api.Context(0)
    ref_ctx.set_target(tgt, 1.0)
    out, dinfo, _ = ref_ctx.deskew([rec], f, [m])
    if leaf is None:
        ref_ctx.set_source(out[0])
        rinfo = None
    else:
        rinfo = ref_ctx.set_source_voxel(out[0], leaf)
    want = _source_checks(ref_ctx, T_ref, cfg, prm)
    ref_ctx.insert_source(T_ref, 0.05)
    want_map = ref_ctx.target_points()
    ref_ctx.close()
    rec7 = np.full((len(rec), 7), 5.0, np.float32)
    rec7[:, :4] = rec
    stream = _hip_stream()
    for form in ("host", "device", "device on the caller's stream"):
        c = api.Context(0)
        dev = None
        try:
            c.set_target(tgt, 1.0)
            if form == "host":
                got = c.set_source_deskew(rec, f, m, leaf)
            else:
                if form.endswith("stream"):
                    c.set_stream(stream)
                dev = DevCloud(rec7, offset=8)
                got = c.set_source_deskew_device(dev.ptr, len(rec), 7, f, m, leaf)
            assert got == (dinfo, rinfo)
            lins, run = _source_checks(c, T_ref, cfg, prm)
            for a, b in zip(lins, want[0]):
                _lin_equal(a, b)
            _icp_equal(run, want[1])
            c.insert_source(T_ref, 0.05)
            assert same(c.target_points(), want_map)
        finally:
            if dev:
                dev.free()
            c.close()
    hip().hipStreamDestroy(C.c_void_p(stream))


def test_deskew_device_gives_the_host_bits(parking):
    tgt, gt, M, rec, T_ref = parking
    clouds, ms = _mixed_batch(np.random.default_rng(9))
    f = api.time_field(4, "f64")
    off = np.r_[0, np.cumsum([len(c) for c in clouds])]
    allr = np.concatenate(clouds)
    c = api.Context(0)
    dev = DevCloud(allr, offset=4)
    out = DevCloud(np.zeros((len(allr), 3), np.float32))
    try:
        for leaf in (None, 0.5):
            (hx, hoff), hinfo, hv = c.deskew((allr, off), f, ms, leaf)
            doff, dinfo, dv = c.deskew_device(dev.ptr, off, 6, f, ms, out.ptr, len(allr), leaf)
            assert np.array_equal(doff, hoff) and dinfo == hinfo and dv == hv
            assert same(_read(out.ptr, int(doff[-1])), hx)
    finally:
        dev.free(); out.free(); c.close()


def test_refused_calls_leave_the_source_as_it_was(parking):
    """the C entry points reached directly (past the Python checks): a column at the stride, a NaN point without a voxel block, a
    reflection, a reversed span, an unknown type, a zero leaf -> DCREG_E_INVALID, and the next linearisation is bitwise the one before"""
    tgt, gt, M, rec, T_ref = parking
    fin = rec[np.all(np.isfinite(rec[:, :3]), 1)]
    c = api.Context(0)
    try:
        c.set_target(tgt, 1.0)
        f, m = api.time_field(3), api.sweep_motion(M[:3, :3], M[:3, 3], (0.0, 0.1), 0.5)
        c.set_source_deskew(fin, f, m)
        prm = api.default_lin_params(1.0, 1)
        before = c.linearize(T_ref[:3, :3], T_ref[:3, 3], prm)
        L = c._L
        bad_col = api.TimeField(4, 0, 1.0)
        refl = api.SweepMotion()
        C.pointer(refl)[0] = m
        refl.R[8] = -1.0
        rev = api.SweepMotion()
        C.pointer(rev)[0] = m
        rev.t_begin, rev.t_end = 0.1, 0.0
        nan_rec = np.ascontiguousarray(fin.copy())
        nan_rec[17, 1] = np.nan
        bad_leaf = api.voxel_params(0.3)
        bad_leaf.leaf[1] = 0.0
        for r, ff, mm, vox in ((fin, bad_col, m, None), (nan_rec, f, m, None), (fin, f, refl, None), (fin, f, rev, None),
                               (fin, api.TimeField(3, 7, 1.0), m, None), (fin, f, m, bad_leaf)):
            rc = L.dcreg_set_source_deskew(c._h, r.ctypes.data, len(r), r.shape[1], C.byref(ff), C.byref(mm),
                                           C.byref(vox) if vox is not None else None, None, None)
            assert rc == api.E_INVALID
            _lin_equal(c.linearize(T_ref[:3, :3], T_ref[:3, 3], prm), before)
    finally:
        c.close()


def test_sixty_four_sweeps_deskewed_in_one_call_register_as_one_by_one(parking):
    """64 moving sweeps deskewed and voxelised in one call; register_frames of the result gives records bitwise equal to each sweep's own
    set_source_deskew + icp_run"""
    tgt, gt, _, _, _ = parking
    rng = np.random.default_rng(21)
    recs, ms, T0 = [], [], []
    for k in range(64):
        Tk = gt @ h.pose6d_matrix(rng.uniform(-5, 5), rng.uniform(-5, 5), 0.0, 0.0, 0.0, h.deg2rad(rng.uniform(-20, 20)))
        xi = np.array([0, 0, rng.uniform(-0.06, 0.06), rng.uniform(0, 1.2), 0, 0])
        M = exp_ref(xi)
        rec, T_ref = h.lidar_sweep_moving(tgt, Tk, M, 0.1, rings=16, cols=512, seed=k)
        recs.append(rec)
        ms.append(api.sweep_motion(M[:3, :3], M[:3, 3], None if k % 2 else (0.0, 0.1), 0.5))
        T0.append(T_ref @ h.pose6d_matrix(*rng.uniform(-0.1, 0.1, 3), *h.deg2rad(rng.uniform(-0.5, 0.5, 3))))
    f = api.time_field(3)
    cfg, _ = cfg_pair(1.0, 20, 1, 1e-5, 1e-3, gt.reshape(16))
    c = api.Context(0)
    try:
        c.set_target(tgt, 1.0)
        frames, info, vinfo = c.deskew(recs, f, ms, leaf=0.4)
        assert info["n_in"] == 64 * 16 * 512 and vinfo["n_out"] == sum(len(x) for x in frames)
        recs_f = c.register_frames(frames, T0, "Ours", cfg)
        for k in range(64):
            c.set_source_deskew(recs[k], f, ms[k], leaf=0.4)
            res, logs = c.icp_run(T0[k], "Ours", cfg)
            T = np.eye(4)
            T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
            T[:3, 3] = res.t[:]
            tr = recs_f[k]
            assert (tr.iterations, tr.converged, tr.status) == (res.iterations, res.converged, res.status), k
            assert np.array_equal(np.array(tr.final_transform[:]), T.reshape(16)), k
            assert np.array_equal(np.array(tr.H_upper[:]), np.array(logs[-1].H_upper[:])), k
    finally:
        c.close()


def test_deskewed_sweeps_register_as_well_as_a_static_sweep():
    """End to end on a world that constrains all six directions: scene_prior_map at its 350 m extent (20 M points, a dozen facades and two
    dozen poles in range), cropped to the sensor's range; a 128 x 1024 sweep at 10 m/s and 0.5 rad/s over 0.1 s, thinned with a 0.2 m
    voxel, registered from the previous pose times the predicted motion.  Errors at the reference instant, measured on an MI355X:
        raw (stamps ignored)                  26.5 cm / 0.85 deg
        deskewed with the true motion          2.21 cm / 0.119 deg
        deskewed with constant_velocity_motion 2.21 cm / 0.119 deg
        static sweep at the reference pose     2.23 cm / 0.120 deg (the floor: beam quantisation of the sweep model)
    Asserted: both deskewed runs within 0.5 cm / 0.02 deg of the floor; the raw run at least 5 times worse in translation or rotation
    than the worst of the other three (measured: 12 times / 7 times)."""
    tgt, _ = h.scene_prior_map(n_map=20_000_000, n_frame=10)
    gt = h.pose6d_matrix(**h.PK01_GT)
    d = tgt[:, :2] - gt[:2, 3].astype(np.float32)
    world = np.ascontiguousarray(tgt[np.einsum("ij,ij->i", d, d) < np.float32(95.0 ** 2)])
    del tgt
    period = 0.1
    xi = np.array([0.0, 0.0, 0.5 * period, 10.0 * period, 0.0, 0.0])
    M = exp_ref(xi)
    T_ref = gt
    T_begin = T_ref @ exp_ref(-0.5 * xi)
    T_prev2, T_prev = T_ref @ exp_ref(-2 * xi), T_ref @ exp_ref(-xi)            # the two previous sweeps' registered poses (true)
    M_cv = api.constant_velocity_motion(T_prev2, T_prev)
    T0 = T_prev @ M_cv
    rec, T_true = h.lidar_sweep_moving(world, T_begin, M, period, 0.5, max_range=90.0, seed=1)
    assert np.allclose(T_true, T_ref, atol=1e-9)
    static = h.lidar_sweep(world, T_ref, max_range=90.0, seed=1)
    f = api.time_field(3)
    cfg, _ = cfg_pair(1.0, 30, 1, 1e-6, 1e-4, T_ref.reshape(16))
    c = api.Context(0)
    errs = {}
    try:
        c.set_target(world, 1.0)
        runs = {"raw": lambda: c.set_source_voxel(rec, 0.2),
                "true motion": lambda: c.set_source_deskew(rec, f, api.sweep_motion(M[:3, :3], M[:3, 3], (0.0, period), 0.5), 0.2),
                "constant velocity": lambda: c.set_source_deskew(rec, f, api.sweep_motion(M_cv[:3, :3], M_cv[:3, 3], (0.0, period), 0.5), 0.2),
                "static": lambda: c.set_source_voxel(static, 0.2)}
        for name, load in runs.items():
            load()
            res, _ = c.icp_run(T0, "Ours", cfg)
            T = np.eye(4)
            T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
            T[:3, 3] = res.t[:]
            errs[name] = api.pose_error(T_ref, T)
    finally:
        c.close()
    print("deskew end to end (trans m, rot deg):", errs)
    fl = errs["static"]
    for name in ("true motion", "constant velocity"):
        assert errs[name][0] <= fl[0] + 0.005 and errs[name][1] <= fl[1] + 0.02, (name, errs)
    raw = errs["raw"]
    worst = max(errs["true motion"][0], errs["constant velocity"][0], fl[0]), max(errs["true motion"][1], errs["constant velocity"][1], fl[1])
    assert raw[0] >= 5 * worst[0] or raw[1] >= 5 * worst[1], errs
