"""The kept voxel map and the fourth engine's linearisation on the device (dcreg_target_voxels_keep / _get, dcreg_linearize_voxels)
against the numpy reference of tests/voxels_ref.py, which applies include/dcreg.h's rule literally: the kept records and the per-point
dump must be BITWISE the reference's, the counts exact, every sum within the derived bound of the exact sum over the dump's rows
(tests/sums_check.py), two calls bitwise equal.  History, interleaved calls of the other engines and the window index change no bit."""
import ctypes as C

import numpy as np
import pytest

import normal_icp_scenes as sc
import sums_check as sums
import visibility_ref
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api
from test_gpu_device_seam import DevCloud, strided
from test_gpu_normals import OPTS_WINDOW
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
MAP_PARAMS = api.voxel_map_params(vs.LEAF, vs.EPS, vs.MIN_POINTS)
INFO_KEYS = ("n_points", "n_voxels", "n_small", "n_degenerate", "n_kept")


def lin_params():
    return api.default_lin_params(RADIUS, 1)


def context(tgt, src, src_normals=None, mode=0, keep=True, opts=()):
    c = api.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_target(tgt, RADIUS)
    if src is not None:
        c.set_source(src)
    if src_normals is not None:
        c.set_source_normals(np.ascontiguousarray(src_normals, np.float32))
    c.set_option("voxels_source_cov", mode)
    if keep:
        c.keep_target_voxels(MAP_PARAMS)
    return c


@pytest.fixture(scope="module")
def lot_ctx():
    """the lot with its frame as the source, the bounded source normals (some points have none) and the voxel map kept"""
    L = vs.lot()
    c = context(L["tgt"], L["src"], L["mb"])
    yield c
    c.close()


def check(c, want, T, what):
    got = c.linearize_voxels(T, lin_params(), debug=True)
    vs.assert_dump_bitwise(got, want, what)
    assert (got["n_eff"], got["n_pt"]) == (want["n_eff"], want["n_pt"]), what
    sums.assert_sums_entrywise(got, got["row"], want["n_eff"], want["n_pt"], what)          # every slot against the dump's own rows
    plain = c.linearize_voxels(T, lin_params())
    sc.assert_sums_bitwise(plain, got, what)                                                  # the plain call: the same sums
    sc.assert_sums_bitwise(c.linearize_voxels(T, lin_params()), plain, what)                  # two calls: the same bytes
    return got


def b_pose(S):
    return S["T"] if "T" in S else S["INIT"]


# ---- 1. the kept voxel map
@pytest.mark.parametrize("name", ["lot", "planted", "lattice"])
def test_the_kept_voxels_are_bitwise_the_reference(name):
    S = vs.MAPS[name]()
    want = S["vmap"]
    a, b = context(S["tgt"], None, keep=False), context(S["tgt"], S["src"], keep=False)
    try:
        assert a.target_voxels_kept() == 0
        with pytest.raises(api.DcregError) as e:
            a.kept_target_voxels()
        assert "(%d)" % api.E_STATE in str(e.value)
        info = a.keep_target_voxels(MAP_PARAMS)
        assert info == {k: want[k] for k in INFO_KEYS}, name
        assert a.target_voxels_kept() == want["n_kept"]
        first = a.kept_target_voxels()
        vs.assert_map_bitwise(first, want, name)
        assert a.keep_target_voxels(MAP_PARAMS) == info                      # keep twice: the same bytes
        vs.assert_map_bitwise(a.kept_target_voxels(), first, name)
        b.linearize(b_pose(S)[:3, :3].reshape(9), b_pose(S)[:3, 3])           # a second context with some history: the same bytes
        assert b.keep_target_voxels(MAP_PARAMS) == info
        vs.assert_map_bitwise(b.kept_target_voxels(), first, name)
        # other parameters: another map, again the reference's
        p2 = api.voxel_map_params(0.5, 1e-2, 3)
        want2 = vr.voxel_map(S["tgt"], 0.5, 1e-2, 3)
        assert a.keep_target_voxels(p2) == {k: want2[k] for k in INFO_KEYS}
        vs.assert_map_bitwise(a.kept_target_voxels(), want2, (name, "leaf 0.5"))
        a.drop_target_voxels()
        assert a.target_voxels_kept() == 0
    finally:
        a.close()
        b.close()


def test_the_map_refusals_need_a_device():
    L = vs.lot()
    c = api.Context(0)
    try:
        with pytest.raises(api.DcregError) as e:
            c.keep_target_voxels(MAP_PARAMS)                               # no target
        assert "(%d)" % api.E_STATE in str(e.value)
        c.set_target(L["tgt"], RADIUS)
        with pytest.raises(api.DcregError) as e:
            c.keep_target_voxels(api.voxel_map_params(1e-7))               # the map spans more than 2^21 voxels
        assert "(%d)" % api.E_INVALID in str(e.value) and c.target_voxels_kept() == 0
        with pytest.raises(api.DcregError) as e:
            c.keep_target_voxels(api.voxel_map_params(1e-300))             # a voxel coordinate beyond 2^62
        assert "(%d)" % api.E_INVALID in str(e.value)
        info = c.keep_target_voxels(MAP_PARAMS)
        n = info["n_kept"]
        buf = [np.zeros((n, 3), np.int64), np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32)]
        ptr = [x.ctypes.data for x in buf]
        assert c._L.dcreg_target_voxels_get(c._h, *ptr, n - 1) == api.E_INVALID and not buf[1].any()
        assert c._L.dcreg_target_voxels_get(c._h, None, ptr[1], ptr[2], ptr[3], n) == api.E_INVALID
        assert c._L.dcreg_target_voxels_get(c._h, *ptr, n) == 0 and buf[1].min() >= vs.MIN_POINTS
        with pytest.raises(api.DcregError):
            c.keep_target_voxels(api.voxel_map_params(1e-7))               # a refused keep leaves the member as it was
        assert c.target_voxels_kept() == n
        # a linearisation in flight: DCREG_E_STATE from every call, and nothing moves
        c.set_source(L["src"])
        before = c.kept_target_voxels()
        out = api.LinOut()
        R, t = np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), np.ascontiguousarray(L["INIT"][:3, 3])
        c.linearize_gated_begin(lin_params())
        try:
            assert c._L.dcreg_target_voxels_keep(c._h, C.byref(MAP_PARAMS), None) == api.E_STATE
            assert c._L.dcreg_target_voxels_get(c._h, *ptr, n) == api.E_STATE
            assert c._L.dcreg_target_voxels_drop(c._h) == api.E_STATE
            assert c._L.dcreg_linearize_voxels(c._h, api._dp(R), api._dp(t), C.byref(lin_params()), C.byref(out)) == api.E_STATE
            assert c._L.dcreg_linearize_voxels_debug(c._h, api._dp(R), api._dp(t), C.byref(lin_params()), C.byref(out), C.byref(api.VlinDebug())) == api.E_STATE
        finally:
            c.gate_abort()
        assert c.target_voxels_kept() == n and out.n_eff == 0
        vs.assert_map_bitwise(c.kept_target_voxels(), before)
        # null arguments and a null dump
        assert c._L.dcreg_target_voxels_keep(c._h, None, None) == api.E_INVALID
        assert c._L.dcreg_linearize_voxels(c._h, None, api._dp(t), C.byref(lin_params()), C.byref(out)) == api.E_INVALID
        assert c._L.dcreg_linearize_voxels_debug(c._h, api._dp(R), api._dp(t), C.byref(lin_params()), C.byref(out), None) == api.E_INVALID
        bad = R.copy()
        bad[4] = np.nan
        assert c._L.dcreg_linearize_voxels(c._h, api._dp(bad), api._dp(t), C.byref(lin_params()), C.byref(out)) == api.E_INVALID
        assert c._L.dcreg_linearize_voxels(c._h, api._dp(R), api._dp(t), C.byref(lin_params()), C.byref(out)) == 0 and out.n_eff > 0
        # a keep that keeps nothing succeeds and leaves no member
        assert c.keep_target_voxels(api.voxel_map_params(1.0, 1e-3, 100000))["n_kept"] == 0 and c.target_voxels_kept() == 0
    finally:
        c.close()


# ---- 2. the dump and the sums against the reference
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pose", ["INIT", "MID", "GT"])
def test_the_lot_is_bitwise_the_reference(lot_ctx, pose, mode):
    L = vs.lot()
    lot_ctx.set_option("voxels_source_cov", mode)
    try:
        for eps in (1e-3, 1e-2):
            lot_ctx.set_option("gicp_epsilon", eps)
            want = vr.linearize(L["vmap"], L["src"], L[pose], mode, L["mb"], eps)
            check(lot_ctx, want, L[pose], (pose, mode, eps))
        assert (want["flag"] == 1).any() and (want["flag"] == 0).any() and (want["flag"] == 3).any() == (mode == 1)
    finally:
        lot_ctx.set_option("gicp_epsilon", vs.GICP_EPS)
        lot_ctx.set_option("voxels_source_cov", 0)


@pytest.mark.parametrize("name", ["planted", "lattice"])
@pytest.mark.parametrize("mode", [0, 1])
def test_planted_voxels_flags_and_the_table_under_load(name, mode):
    S = vs.MAPS[name]()
    c = context(S["tgt"], S["src"], S["src_normals"], mode)
    try:
        want = vr.linearize(S["vmap"], S["src"], S["T"], mode, S["src_normals"], vs.GICP_EPS)
        got = check(c, want, S["T"], (name, mode))
        if name == "planted":
            assert got["flag"].tolist() == S["flags%d" % mode]
            assert got["voxel_idx"][10] == -1 and got["voxel_idx"][11] == -1 and got["voxel_idx"][7] != got["voxel_idx"][8]
    finally:
        c.close()


def test_mode_1_without_source_normals_is_refused_and_mode_0_does_not_need_them():
    L = vs.lot()
    c = context(L["tgt"], L["src"])
    try:
        want = vr.linearize(L["vmap"], L["src"], L["INIT"])
        check(c, want, L["INIT"], "no source normals")
        c.set_option("voxels_source_cov", 1)
        out = api.LinOut()
        out.n_eff = 77
        R, t = np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), np.ascontiguousarray(L["INIT"][:3, 3])
        assert c._L.dcreg_linearize_voxels(c._h, api._dp(R), api._dp(t), C.byref(lin_params()), C.byref(out)) == api.E_STATE
        assert out.n_eff == 77 and "no kept source normals" in c._L.dcreg_last_error(c._h).decode()
        with pytest.raises(api.DcregError):
            c.set_option("voxels_source_cov", 2)
    finally:
        c.close()


# ---- 3. source sizes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_source_sizes_across_wave_and_block_boundaries(n):
    L = vs.lot()
    src = sc.sized_source(n)
    m = np.array(sc.unit_normals(n, 300 + n))
    m[::7] = np.nan                                                       # every 7th normal is missing
    c = context(L["tgt"], src, m)
    try:
        for mode in (0, 1):
            c.set_option("voxels_source_cov", mode)
            for pose in ("INIT", "GT"):
                want = vr.linearize(L["vmap"], src, L[pose], mode, m, vs.GICP_EPS)
                check(c, want, L[pose], (n, mode, pose))
            assert (want["flag"] == 3).any() == (mode == 1)
    finally:
        c.close()


# ---- 5. robust kernels
@pytest.mark.parametrize("mode", [0, 1])
def test_the_robust_kernels_scale_the_rows_by_the_references_factor(lot_ctx, mode):
    L = vs.lot()
    lot_ctx.set_option("voxels_source_cov", mode)
    try:
        base = lot_ctx.linearize_voxels(L["INIT"], lin_params(), debug=True)
        lot_ctx.set_robust(0, gicp_scale=0.7)
        none = lot_ctx.linearize_voxels(L["INIT"], lin_params(), debug=True)
        vs.assert_dump_bitwise(none, base, "kernel 0")
        sc.assert_sums_bitwise(none, base, "kernel 0")
        eff = base["flag"] == 1
        for kind in (1, 2, 3):
            lot_ctx.set_robust(kind, gicp_scale=0.7)
            want = vr.linearize(L["vmap"], L["src"], L["INIT"], mode, L["mb"], vs.GICP_EPS, kind, 0.7)
            got = check(lot_ctx, want, L["INIT"], (mode, kind))
            assert np.array_equal(got["row"][eff][:, :, :7], want["k"][eff][:, None, None] * base["row"][eff][:, :, :7])
            assert np.array_equal(got["row"][..., 7], base["row"][..., 7]) and (want["k"][eff] < 1.0).any()
    finally:
        lot_ctx.set_robust(0, gicp_scale=1.0)
        lot_ctx.set_option("voxels_source_cov", 0)


# ---- 6. history independence, with the other engines' calls in between, and the window index
def test_a_walk_is_bitwise_fresh_contexts_with_the_other_engines_in_between(lot_ctx):
    L = vs.lot()
    mixed = context(L["tgt"], L["src"], L["mb"])
    others = context(L["tgt"], L["src"], L["mb"], keep=False)
    window = context(L["tgt"], L["src"], L["mb"], opts=OPTS_WINDOW)
    R9 = lambda T: np.ascontiguousarray(T[:3, :3]).reshape(9)
    try:
        for c in (mixed, others):
            c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
        for step, T in enumerate(sc.walk()):
            U = sc.walk()[(step + 2) % 5]
            fresh = context(L["tgt"], L["src"])
            try:
                want = fresh.linearize_voxels(T, lin_params(), debug=True)
            finally:
                fresh.close()
            want_n, want_g = others.linearize_normals(T, lin_params()), others.linearize_gicp(T, lin_params())
            want_1 = others.linearize(R9(T), T[:3, 3], lin_params())
            a = lot_ctx.linearize_voxels(T, lin_params())                  # carries everything this module did before
            n1 = mixed.linearize_normals(T, lin_params())
            v1 = mixed.linearize_voxels(T, lin_params())
            g1 = mixed.linearize_gicp(U, lin_params())
            v2 = mixed.linearize_voxels(T, lin_params(), debug=True)
            l1 = mixed.linearize(R9(T), T[:3, 3], lin_params())
            v3 = mixed.linearize_voxels(T, lin_params())
            g2, n2 = mixed.linearize_gicp(T, lin_params()), mixed.linearize_normals(T, lin_params())
            for x in (a, v1, v2, v3):
                sc.assert_sums_bitwise(x, want, step)
            vs.assert_dump_bitwise(v2, want, step)
            for x in (n1, n2):
                sc.assert_sums_bitwise(x, want_n, step)
            sc.assert_sums_bitwise(g2, want_g, step)
            sc.assert_sums_bitwise(g1, others.linearize_gicp(U, lin_params()), step)
            sc.assert_sums_bitwise(l1, want_1, step)
            # the window index: active or not, rebuilt or not, it changes nothing
            w = window.linearize_voxels(T, lin_params(), debug=True)
            vs.assert_dump_bitwise(w, want, (step, "window"))
            sc.assert_sums_bitwise(w, want, (step, "window"))
            ref = vr.linearize(L["vmap"], L["src"], T)
            vs.assert_dump_bitwise(v2, ref, step)
    finally:
        mixed.close()
        others.close()
        window.close()


def test_a_keep_behind_a_live_window_summarises_the_whole_map():
    """the window is the ACTIVE index once a single-pose launch of the first engine has run (roi_index = 2): a keep that arrives then must
    read the whole map's points, not the window's (tests/state_walk.py reaches the same order from many histories)"""
    L = vs.lot()
    c = context(L["tgt"], L["src"], keep=False, opts=OPTS_WINDOW)
    try:
        c.linearize(np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), L["INIT"][:3, 3], api.default_lin_params(RADIUS))
        assert c.roi_info()["active"]
        assert c.keep_target_voxels(MAP_PARAMS) == {k: L["vmap"][k] for k in INFO_KEYS}
        vs.assert_map_bitwise(c.kept_target_voxels(), L["vmap"], "behind the window")
        check(c, vr.linearize(L["vmap"], L["src"], L["INIT"]), L["INIT"], "behind the window")
    finally:
        c.close()


# ---- 7. invalidation
def test_every_change_of_the_map_drops_the_voxels_and_the_source_side_calls_leave_them():
    L = vs.lot()
    tgt, src = np.array(L["tgt"]), np.array(L["src"])
    c = context(tgt, src, keep=False)
    R, t = np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), np.ascontiguousarray(L["INIT"][:3, 3])
    dev = DevCloud(strided(tgt, 4, fill=0.0))

    def refused():
        assert c.target_voxels_kept() == 0
        out = api.LinOut()
        out.n_eff, out.sum_r2 = 77, 5.5
        assert c._L.dcreg_linearize_voxels(c._h, api._dp(R), api._dp(t), C.byref(lin_params()), C.byref(out)) == api.E_STATE
        assert (out.n_eff, out.sum_r2) == (77, 5.5) and "no kept voxels" in c._L.dcreg_last_error(c._h).decode()          # the output is untouched
        with pytest.raises(api.DcregError):
            c.kept_target_voxels()

    c.keyframes_reset()
    kf = c.keyframes_add([tgt[:2000], tgt[2000:]])
    members = [(kf, np.eye(4)), (kf + 1, np.eye(4))]
    lo, hi = tgt.min(axis=0) + 1.0, tgt.max(axis=0) - 1.0
    changes = (lambda: c.set_target(tgt, RADIUS), lambda: c.set_target_device(dev.ptr, dev.n, dev.stride, RADIUS),
               lambda: c.set_target_voxel(tgt, RADIUS, 0.05), lambda: c.set_target_outliers(tgt, RADIUS, api.outlier_params(k=4, std_mul=5.0)),
               lambda: c.insert(src, L["GT"], 0.05), lambda: c.insert_source(L["GT"], 0.02), lambda: c.crop(lo, hi),
               lambda: c.remove_outliers(api.outlier_params(k=4, std_mul=1.0)), lambda: c.set_target_keyframes(members, RADIUS))
    try:
        refused()                                                          # nothing kept yet
        for i, change in enumerate(changes):
            c.keep_target_voxels(MAP_PARAMS)
            assert c.target_voxels_kept() > 0 and c.linearize_voxels(L["INIT"], lin_params())["n_pt"] > 0, i
            change()
            refused()
        # moving objects voted out of the map (tests/visibility_ref.py's scene: a box drives past twelve sweeps)
        M = visibility_ref.mover_scene()
        c.keyframes_reset()
        c.keyframes_add(M["store"])
        c.set_target(M["map"], RADIUS)
        assert c.keep_target_voxels(MAP_PARAMS)["n_kept"] > 0
        assert c.remove_dynamic(list(enumerate(M["poses"])), api.visibility_params())["n_flagged"] > 0
        refused()
        # a new source, the batched calls and the source's normals leave the member alone
        c.set_target(tgt, RADIUS)
        c.keep_target_voxels(MAP_PARAMS)
        first = c.kept_target_voxels()
        base = c.linearize_voxels(L["INIT"], lin_params(), debug=True)
        c.set_source(src[::-1].copy())
        again = c.linearize_voxels(L["INIT"], lin_params(), debug=True)
        vs.assert_dump_bitwise({k: again[k][::-1] for k in vs.DUMP_KEYS}, base)
        c.set_source(src)
        cfg = cfg_pk01(max_iterations=3)
        c.register_frames([src[:200], src[100:400]], [L["INIT"], L["MID"]], "Ours", cfg)
        c.icp_run_trials([L["INIT"], L["MID"]], "Ours", cfg)
        c.keep_source_normals(api.normal_params(k=5))
        c.set_source_voxel(src, 0.01)
        c.set_source(src)
        assert c.target_voxels_kept() == len(first["count"])
        vs.assert_map_bitwise(c.kept_target_voxels(), first)
        after = c.linearize_voxels(L["INIT"], lin_params(), debug=True)
        vs.assert_dump_bitwise(after, base)
        sc.assert_sums_bitwise(after, base)
        # a refused target leaves map and member as they were
        with pytest.raises(api.DcregError):
            c.set_target(np.full((4, 3), np.nan, np.float32), RADIUS)
        assert c.target_voxels_kept() == len(first["count"])
        sc.assert_sums_bitwise(c.linearize_voxels(L["INIT"], lin_params()), base)
    finally:
        dev.free()
        c.close()
