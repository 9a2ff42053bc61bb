"""Candidate poses scored against the map on the device (dcreg_verify_poses*) against tests/verify_ref.py, which applies include/dcreg.h's
rule literally: every record - pose, count, cost, score as integers, fitness and rmse as bit patterns -, the rank, the detail arrays and
the info must be the reference's, whatever the number of points and poses, the point stride, the split of the poses over launches, the
form the cloud arrives in and whatever the context did before."""
import ctypes as C
import functools

import numpy as np
import pytest

import normal_icp_ref as nref
import normal_icp_scenes as sc
import verify_ref as vr
from dcreg_amd import api
from test_fpfh_reference import uniform
from test_gpu_device_seam import D2H, H2D, DevCloud, hip, strided
from test_gpu_voxel import _hip_stream
from test_normal_icp_reference import cfg_pk01
from test_normals_reference import lattice

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
DS = (0.1, 0.3, 0.5)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.loaded = None
    yield c
    c.close()


def use(c, tgt, src, tag):
    """the clouds of a test on the shared context (set once per run of tests that share them)"""
    if c.loaded != tag:
        c.set_target(tgt, 0.5)
        c.set_source(src)
        c.loaded = tag


def use_lot(c):
    L = sc.lot()
    use(c, L["tgt"], L["src"], "lot")
    return L


@functools.lru_cache(maxsize=None)
def lot_reference(d, stride=1, rank_by=0):
    L = sc.lot()
    return vr.verify(L["tgt"], L["src"], vr.lot_poses(), d, stride, rank_by)


@functools.lru_cache(maxsize=None)
def perturbed(P, seed=5):
    """P seeded perturbations of the lot's truth: the truth, then offsets growing from millimetres to metres"""
    rng = np.random.default_rng(seed)
    G = sc.lot()["GT"]
    Ts = [np.array(G)]
    for k in range(1, P):
        a = 3.0 * k / max(P - 1, 1)
        dx, dy, dz = rng.normal(0.0, 0.02 + a, 3) * [1.0, 1.0, 0.1]
        Ts.append(sc.offset(G, dx, dy, dz, rng.normal(0.0, 0.01 + 0.1 * a)))
    return sc.frozen(np.stack(Ts))


def check(got, want, n_points, what=""):
    vr.assert_records(got["records"], want["records"], what)
    assert got["order"] == want["order"], what
    assert got["info"] == dict(n_poses=len(want["order"]), n_points=n_points, n_scored=want["n_scored"], best_pose=want["order"][0]), (what, got["info"])


def small_poses(seed):
    """identity and six small motions of a cloud that fills a 4 x 4 x 1.2 m box"""
    rng = np.random.default_rng(seed)
    Ts = [np.eye(4)]
    for k in range(6):
        T = np.eye(4)
        Ts.append(sc.offset(T, *(rng.normal(0.0, 0.03 * (k + 1), 3)), yaw=rng.normal(0.0, 0.01 * (k + 1))))
    return np.stack(Ts)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, "lot"])
def test_source_sizes_distances_and_both_rank_rules(ctx, n):
    if n == "lot":
        L = use_lot(ctx)
        tgt, src, Ts = L["tgt"], L["src"], vr.lot_poses()
    else:
        tgt, src, Ts = uniform(4099), uniform(n, seed=1), small_poses(n)
        use(ctx, tgt, src, ("uniform", n))
    some = False
    for d in DS:
        for rank_by in (0, 1):
            want = lot_reference(d, 1, rank_by) if n == "lot" else vr.verify(tgt, src, Ts, d, 1, rank_by)
            got = ctx.verify_poses(Ts, api.verify_params(inlier_distance=d, rank_by=rank_by))
            check(got, want, len(src), (n, d, rank_by))
            some = some or any(0 < s["count"] for s in want["scores"])
    assert some or n == 1


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 300])
def test_pose_counts_and_the_split_over_launches(ctx, P):
    L = use_lot(ctx)
    Ts = perturbed(P)
    stride = 4 if P > 100 else 1                           # (the reference of 300 poses on every point takes ten seconds)
    want = vr.verify(L["tgt"], L["src"], Ts, 0.3, stride)
    assert want["scores"][0]["count"] == want["n_scored"] and (P < 63 or len({s["count"] for s in want["scores"]}) > 20)
    try:
        for per in (0, 1, 7):
            ctx.set_option("verify_poses_per_launch", per)
            check(ctx.verify_poses(Ts, api.verify_params(inlier_distance=0.3, point_stride=stride)), want, 523, (P, per))
            if P == 65:                                    # the detail pose in the first, a middle and the last launch
                for k in (0, 40, 64):
                    got = ctx.verify_poses(Ts, api.verify_params(inlier_distance=0.3, detail_pose=k), want_detail=True)
                    assert np.array_equal(got["mask"], want["scores"][k]["mask"]) and np.array_equal(got["nn"], want["scores"][k]["nn"]), (per, k)
    finally:
        ctx.set_option("verify_poses_per_launch", 0)


def test_the_lattice_edge_the_gate_is_strict(ctx):
    lat = lattice((8, 8, 8), 0.25)
    use(ctx, lat, lat, "lattice")
    T = np.eye(4)
    T[0, 3] = 0.125
    at = ctx.verify_poses([T], api.verify_params(inlier_distance=0.125))
    assert (at["records"][0]["count"], at["records"][0]["cost"], at["records"][0]["score"]) == (0, 0, 512 << 20)
    p = api.verify_params(inlier_distance=np.nextafter(0.125, 1.0), detail_pose=0)
    up = ctx.verify_poses([T], p, want_detail=True)
    assert (up["records"][0]["count"], up["records"][0]["cost"], up["records"][0]["fitness"]) == (512, 512 * ((1 << 20) - 1), 1.0)
    assert up["mask"].all() and np.array_equal(up["nn"], np.arange(512))
    for d in (0.125, np.nextafter(0.125, 1.0), np.nextafter(0.125, 0.0), 0.2):
        Ts = np.stack([T, np.eye(4)])
        check(ctx.verify_poses(Ts, api.verify_params(inlier_distance=d)), vr.verify(lat, lat, Ts, d), 512, d)


def test_duplicate_poses_and_far_poses_rank_by_their_index(ctx):
    L = use_lot(ctx)
    G, far = L["GT"], sc.offset(L["GT"], dx=300.0)
    Ts = np.stack([far, L["MID"], G, far, G, L["MID"], sc.offset(G, dz=-5.0e4), G])
    for rank_by in (0, 1):
        want = vr.verify(L["tgt"], L["src"], Ts, 0.3, 1, rank_by)
        got = ctx.verify_poses(Ts, api.verify_params(inlier_distance=0.3, rank_by=rank_by))
        check(got, want, 523, rank_by)
        assert got["order"][:3] == [2, 4, 7] and got["order"][-3:] == [0, 3, 6]
        assert [r["count"] for r in got["records"][-3:]] == [0, 0, 0] and got["records"][-1]["score"] == 523 << 20


@pytest.mark.parametrize("stride", [1, 2, 3, 64, 523, 524])
def test_the_point_stride_selects_by_original_index(ctx, stride):
    L = use_lot(ctx)
    Ts = vr.lot_poses()
    p = api.verify_params(inlier_distance=0.3, point_stride=stride, detail_pose=1)
    want = lot_reference(0.3, stride)
    got = ctx.verify_poses(Ts, p, want_detail=True)
    check(got, want, 523, stride)
    assert want["n_scored"] == len(range(0, 523, stride))
    assert np.array_equal(got["mask"], want["scores"][1]["mask"]) and np.array_equal(got["nn"], want["scores"][1]["nn"])
    cl = ctx.verify_poses(Ts, p, cloud=L["src"], want_detail=True)
    check(cl, want, 523, ("cloud", stride))
    assert np.array_equal(cl["mask"], got["mask"]) and np.array_equal(cl["nn"], got["nn"])


def lin_bytes(c, T):
    o = c.linearize(T[:3, :3], T[:3, 3], api.default_lin_params(0.5, 1))
    return (np.asarray(o["H_upper"]).tobytes(), np.asarray(o["g"]).tobytes(), o["sum_r2"], o["sum_b2"], o["n_eff"], o["n_pt"])


def test_the_cloud_forms_host_strides_device_pointers_and_a_late_write(ctx):
    L = use_lot(ctx)
    Ts = vr.lot_poses()
    p = api.verify_params(inlier_distance=0.3, detail_pose=2)
    want = lot_reference(0.3)
    before = lin_bytes(ctx, L["MID"])
    resident = ctx.verify_poses(Ts, p, want_detail=True)
    check(resident, want, 523, "resident")
    other = np.ascontiguousarray(L["src"][::-1] + np.float32(0.01))          # a cloud that is NOT the source, NaN rows among its points
    other[[0, 17, 300]] = [[np.nan, 0, 0], [0, np.inf, 0], [np.nan] * 3]
    want_other = vr.verify(L["tgt"], other, Ts, 0.3)
    assert want_other["n_scored"] == 520
    for stride in (3, 4, 7):
        got = ctx.verify_poses(Ts, p, cloud=strided(L["src"], stride), want_detail=True)
        check(got, want, 523, ("host", stride))                              # the cloud is the source: the resident form's records
        assert np.array_equal(got["mask"], resident["mask"]) and np.array_equal(got["nn"], resident["nn"])
        got = ctx.verify_poses(Ts, p, cloud=strided(other, stride), want_detail=True)
        check(got, want_other, 523, ("host other", stride))
        assert np.array_equal(got["mask"], want_other["scores"][2]["mask"]) and np.array_equal(got["nn"], want_other["scores"][2]["nn"])
        assert not got["mask"][[0, 17, 300]].any()
        dev = DevCloud(strided(other, stride), offset=4 * (stride % 4))
        dm, dn = DevCloud(np.full((523, 1), 9.0, np.float32)), DevCloud(np.full((523, 1), 9.0, np.float32))
        try:
            got = ctx.verify_poses_device(dev.ptr, 523, stride, Ts, p, dev_mask=dm.ptr, dev_nn=dn.ptr)
            check(got, want_other, 523, ("device", stride))
            mask, nn = np.empty(523, np.uint8), np.empty(523, np.int32)
            assert hip().hipMemcpy(C.c_void_p(mask.ctypes.data), C.c_void_p(dm.ptr), 523, D2H) == 0
            assert hip().hipMemcpy(C.c_void_p(nn.ctypes.data), C.c_void_p(dn.ptr), 4 * 523, D2H) == 0
            assert np.array_equal(mask, want_other["scores"][2]["mask"]) and np.array_equal(nn, want_other["scores"][2]["nn"])
            check(ctx.verify_poses_device(dev.ptr, 523, stride, Ts, api.verify_params(inlier_distance=0.3)), want_other, 523, ("device plain", stride))
        finally:
            dev.free(); dm.free(); dn.free()
    # a device cloud written on the caller's stream just before the call: the call is ordered behind the write
    Lh = hip()
    Lh.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    Lh.hipStreamSynchronize.argtypes = [C.c_void_p]
    stream = _hip_stream()
    rows = strided(other, 4, fill=7.0)
    dev = DevCloud(np.full_like(rows, np.nan))
    try:
        ctx.set_stream(stream)
        assert Lh.hipMemcpyAsync(C.c_void_p(dev.ptr), C.c_void_p(rows.ctypes.data), rows.nbytes, H2D, C.c_void_p(stream)) == 0
        check(ctx.verify_poses_device(dev.ptr, 523, 4, Ts, api.verify_params(inlier_distance=0.3)), want_other, 523, "side stream")
    finally:
        assert Lh.hipStreamSynchronize(C.c_void_p(stream)) == 0
        ctx.set_stream(0)
        dev.free()
        Lh.hipStreamDestroy(C.c_void_p(stream))
    # nothing of it touched the resident source
    check(ctx.verify_poses(Ts, p), want, 523, "resident again")
    assert lin_bytes(ctx, L["MID"]) == before
    empty = ctx.verify_poses(Ts, api.verify_params(inlier_distance=0.3), cloud=np.full((5, 3), np.nan, np.float32))
    assert empty["info"] == dict(n_poses=6, n_points=5, n_scored=0, best_pose=0) and empty["order"] == list(range(6))
    assert all((r["count"], r["score"], r["fitness"], r["rmse"]) == (0, 0, 0.0, 0.0) for r in empty["records"])
    none = ctx.verify_poses(Ts, api.verify_params(inlier_distance=0.3), cloud=np.zeros((0, 3), np.float32))
    assert none["info"]["n_points"] == 0 and none["order"] == list(range(6))


def test_the_detail_arrays_against_the_search_call(ctx):
    L = use_lot(ctx)
    Ts = vr.lot_poses()
    for d in (0.1, 0.3):
        want = lot_reference(d)
        for k in (0, len(Ts) - 1, 3):
            got = ctx.verify_poses(Ts, api.verify_params(inlier_distance=d, detail_pose=k), want_detail=True)
            assert np.array_equal(got["mask"], want["scores"][k]["mask"]) and np.array_equal(got["nn"], want["scores"][k]["nn"]), (d, k)
            assert int(got["mask"].sum()) == got["records"][got["order"].index(k)]["count"]
            q = nref.transform(Ts[k][:3, :3], Ts[k][:3, 3], L["src"])
            idx, d2 = ctx.knn(q, 1, d)
            gate = (idx[:, 0] >= 0) & (d2[:, 0].astype(np.float64) < np.float64(d) * np.float64(d))
            assert np.array_equal(got["mask"] == 1, gate), (d, k)
            assert np.array_equal(got["nn"][gate], idx[gate, 0]), (d, k)
    # without a detail pose the arrays are not written; a null array is skipped
    Lc = api.load()
    T16 = np.ascontiguousarray(Ts.reshape(-1, 16))
    recs, info = (api.VerifyRecord * 6)(), api.VerifyInfo()
    mask, nn = np.full(523, 5, np.uint8), np.full(523, 5, np.int32)
    p = api.verify_params(inlier_distance=0.3)
    assert Lc.dcreg_verify_poses(ctx._h, T16.ctypes.data, 6, 16, C.byref(p), recs, mask.ctypes.data, nn.ctypes.data, C.byref(info)) == 0
    assert (mask == 5).all() and (nn == 5).all()
    p.detail_pose = 1
    assert Lc.dcreg_verify_poses(ctx._h, T16.ctypes.data, 6, 16, C.byref(p), recs, None, nn.ctypes.data, None) == 0
    assert np.array_equal(nn, lot_reference(0.3)["scores"][1]["nn"])
    assert Lc.dcreg_verify_poses(ctx._h, T16.ctypes.data, 6, 16, C.byref(p), recs, mask.ctypes.data, None, None) == 0
    assert np.array_equal(mask, lot_reference(0.3)["scores"][1]["mask"])


def test_the_poses_of_an_array_of_align_records_are_read_in_place(ctx):
    L = use_lot(ctx)
    Ts = vr.lot_poses()
    recs_in = (api.AlignRecord * len(Ts))()
    for r, T in zip(recs_in, Ts):
        r.T[:] = list(T.reshape(16))
        r.hypothesis, r.count, r.cost, r.rmse = -1, 7, 2 ** 63, np.nan          # what lies between two poses is not read
    assert C.sizeof(api.AlignRecord) == 8 * api.VERIFY_RECORD_STRIDE
    out, info = (api.VerifyRecord * len(Ts))(), api.VerifyInfo()
    p = api.verify_params(inlier_distance=0.3)
    assert api.load().dcreg_verify_poses(ctx._h, C.addressof(recs_in), len(Ts), api.VERIFY_RECORD_STRIDE, C.byref(p), out, None, None, C.byref(info)) == 0
    vr.assert_records(api._verify_records(out, len(Ts)), lot_reference(0.3)["records"], "stride 22")
    dicts = [{"T": np.array(r.T).reshape(4, 4), "count": r.count} for r in recs_in]
    check(ctx.verify_poses(dicts, p), lot_reference(0.3), 523, "record dicts")


def test_the_records_do_not_depend_on_what_the_context_did_before(ctx):
    L = sc.lot()
    Ts = perturbed(20)
    p = api.verify_params(inlier_distance=0.3)
    want = vr.verify(L["tgt"], L["src"], Ts, 0.3)
    cfg = cfg_pk01()
    for option, value in ((None, 0), ("roi_index", 2), ("max_table_entries", 1 << 20)):
        c = api.Context(0)
        try:
            if option:
                c.set_option(option, value)
            c.set_target(L["tgt"], 0.5)
            c.set_source(L["src"])
            check(c.verify_poses(Ts, p), want, 523, (option, "fresh"))
            c.keep_target_normals()
            c.icp_run(L["INIT"], "Ours", cfg)
            c.icp_run_normals(L["INIT"], "Ours", cfg)
            check(c.verify_poses(Ts, p), want, 523, (option, "after runs"))
            # a verify call between two linearisations changes neither engine's sums
            prm = api.default_lin_params(0.5, 1)
            a = (lin_bytes(c, L["MID"]), c.linearize_normals(L["MID"], prm))
            check(c.verify_poses(Ts, p), want, 523, (option, "between"))
            b = (lin_bytes(c, L["MID"]), c.linearize_normals(L["MID"], prm))
            assert a[0] == b[0]
            for k in ("H_upper", "g"):
                assert np.asarray(a[1][k]).tobytes() == np.asarray(b[1][k]).tobytes(), (option, k)
            assert (a[1]["sum_r2"], a[1]["sum_b2"], a[1]["n_eff"], a[1]["n_pt"]) == (b[1]["sum_r2"], b[1]["sum_b2"], b[1]["n_eff"], b[1]["n_pt"])
        finally:
            c.close()


def test_the_count_is_the_point_to_point_metric_s(ctx):
    """an independent path: dcreg_p2p_error searches unbounded and gates (double)sqrtf(d2) < d"""
    L = use_lot(ctx)
    Ts = vr.lot_poses()
    for d in (0.3, 0.5):
        want = lot_reference(d)
        # the two gates agree unless a distance lies at the threshold: a precondition on the input
        for s in want["scores"]:
            root = np.sqrt(s["d2"][np.isfinite(s["d2"])].astype(np.float64))
            assert not (np.abs(root - d) < 1e-5).any()
        got = ctx.verify_poses(Ts, api.verify_params(inlier_distance=d))
        by_pose = {r["pose"]: r for r in got["records"]}
        for k, T in enumerate(Ts):
            assert ctx.p2p_error(T, d)[3] == by_pose[k]["count"] == want["scores"][k]["count"], (d, k)


def test_refusals_leave_every_output_untouched():
    L = sc.lot()
    Lc = api.load()
    c = api.Context(0)
    Ts = np.ascontiguousarray(vr.lot_poses().reshape(-1, 16))
    src = np.ascontiguousarray(L["src"])
    recs, info = (api.VerifyRecord * 6)(), api.VerifyInfo()
    mask, nn = np.full(523, 5, np.uint8), np.full(523, 5, np.int32)

    def call(form="resident", T=Ts, n_poses=6, pose_stride=16, params=True, records=True, xyz=src, n=523, stride=3, **kw):
        p = api.verify_params(detail_pose=0)
        for k, v in kw.items():
            setattr(p, k, v)
        for r in recs:
            r.count = 77
        info.n_poses = 88
        mask[:], nn[:] = 5, 5
        tail = (T.ctypes.data if T is not None else None, n_poses, pose_stride, C.byref(p) if params else None, recs if records else None,
                mask.ctypes.data, nn.ctypes.data, C.byref(info))
        if form == "resident":
            rc = Lc.dcreg_verify_poses(c._h, *tail)
        else:
            rc = getattr(Lc, "dcreg_verify_poses_" + form)(c._h, xyz.ctypes.data if xyz is not None else None, n, stride, *tail)
        untouched = all(r.count == 77 for r in recs) and info.n_poses == 88 and (mask == 5).all() and (nn == 5).all()
        return rc, untouched, Lc.dcreg_last_error(c._h).decode()

    def bad(k, how):
        T = Ts.copy().reshape(-1, 4, 4)
        if how == "nan":
            T[k, 0, 3] = np.nan
        elif how == "scaled":
            T[k, :3, :3] *= 1.001
        else:
            T[k, 1, 1] = -T[k, 1, 1]
        return np.ascontiguousarray(T.reshape(-1, 16))

    try:
        # ---- no map, no source: the state refusals come behind the argument refusals
        assert call()[:2] == (E_STATE, True) and call(inlier_distance=0.0)[:2] == (E_INVALID, True)
        c.set_target(L["tgt"], 0.5)
        assert call()[:2] == (E_STATE, True) and "source" in call()[2]
        assert call("cloud")[0] == 0                                            # the cloud form needs no source
        c.set_source(L["src"])
        assert call()[0] == 0 and info.n_poses == 6
        invalid = [dict(params=False), dict(records=False), dict(T=None), dict(n_poses=-1), dict(n_poses=65536), dict(pose_stride=15), dict(pose_stride=0),
                   dict(inlier_distance=0.0), dict(inlier_distance=-1.0), dict(inlier_distance=np.nan), dict(inlier_distance=np.inf),
                   dict(point_stride=0), dict(point_stride=-4), dict(rank_by=2), dict(rank_by=-1), dict(detail_pose=-2), dict(detail_pose=6),
                   dict(n_poses=0, detail_pose=0)]
        for form in ("resident", "cloud", "cloud_device"):
            for kw in invalid:
                assert call(form, **kw)[:2] == (E_INVALID, True), (form, kw)
            for k in (0, 5):
                for how in ("nan", "scaled", "mirror"):
                    rc, untouched, msg = call(form, T=bad(k, how))
                    assert (rc, untouched) == (E_INVALID, True) and "pose %d" % k in msg, (form, k, how, msg)
        for form in ("cloud", "cloud_device"):
            for kw in (dict(stride=2), dict(n=-1), dict(n=2 ** 31), dict(xyz=None)):
                assert call(form, **kw)[:2] == (E_INVALID, True), (form, kw)
        # n_poses == 0: nothing to do, a zero info
        rc, _, _ = call(n_poses=0, detail_pose=-1)
        assert rc == 0 and (info.n_poses, info.n_points, info.n_scored, info.best_pose) == (0, 0, 0, 0) and (mask == 5).all()
        # ---- a linearisation in flight
        three = vr.lot_poses()[:3]                            # dcreg_linearize_batch_begin itself, three poses in one launch
        R9 = np.ascontiguousarray(three[:, :3, :3]).reshape(3, 9)
        t3 = np.ascontiguousarray(three[:, :3, 3])
        prm, outs = api.default_lin_params(0.5, 1), (api.LinOut * 3)()
        dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
        assert Lc.dcreg_linearize_batch_begin(c._h, 0, 3, dp(R9), dp(t3), C.byref(prm)) == 0
        for form in ("resident", "cloud", "cloud_device"):
            assert call(form)[:2] == (E_STATE, True), form
        assert Lc.dcreg_linearize_batch_end(c._h, 0, outs) == 0 and outs[0].n_eff > 0
        assert call()[0] == 0
    finally:
        c.close()
