"""The third engine on the device (dcreg_source_normals_keep / _set / _get, dcreg_linearize_gicp, dcreg_icp_run_gicp) against the numpy
reference of tests/gicp_ref.py, which applies include/dcreg.h's rule literally: the per-point dump must be BITWISE the reference's, the
sums agree with the exactly rounded sums of the reference rows to the tolerances of tests/test_gpu_parity.py, the counts exactly; every sum also lies within the derived bound of the
exact sum over the reference's rows (tests/sums_check.py).
History, interleaved calls of the second engine and the window index change no bit; the other engines' results do not move."""
import ctypes as C

import numpy as np
import pytest

import gicp_ref as gref
import gicp_scenes as gs
import normal_icp_scenes as sc
import sums_check as sums
from dcreg_amd import api
from test_gpu_device_seam import D2H, DevCloud, hip, strided
from test_gpu_normals import OPTS_WINDOW
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = gs.RADIUS
PARAMS_B = api.normal_params(k=5, search_radius=RADIUS)
PARAMS_5 = api.normal_params(k=5)


def read_device(dev, rows, cols):
    """rows x cols floats of a DevCloud's memory"""
    back = np.zeros((rows, cols), np.float32)
    assert hip().hipMemcpy(C.c_void_p(back.ctypes.data), C.c_void_p(dev.ptr), back.nbytes, D2H) == 0
    return back


def lin_params(radius=RADIUS):
    return api.default_lin_params(radius, 1)


def values(o):
    """a ctypes record as nested tuples of its fields' bit patterns (padding bytes are nobody's)"""
    if isinstance(o, C.Structure):
        return tuple(values(getattr(o, f[0])) for f in o._fields_)
    if isinstance(o, C.Array):
        return tuple(values(x) for x in o)
    return np.float64(o).tobytes() if isinstance(o, float) else o


def context(tgt, src, normals=None, src_normals=None, opts=()):
    c = api.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_target(tgt, RADIUS)
    if src is not None:
        c.set_source(src)
    if normals is not None:
        c.set_target_normals(np.ascontiguousarray(normals, np.float32))
    if src_normals is not None:
        c.set_source_normals(np.ascontiguousarray(src_normals, np.float32))
    return c


@pytest.fixture(scope="module")
def lot_ctx():
    """the lot with its frame as the source and the bounded normals kept on both sides"""
    L = gs.lot()
    c = context(L["tgt"], L["src"])
    c.keep_target_normals(PARAMS_B)
    c.keep_source_normals(PARAMS_B)
    yield c
    c.close()


def check(c, want, T, what, radius=RADIUS):
    got = c.linearize_gicp(T, lin_params(radius), debug=True)
    gs.assert_dump_bitwise(got, want, what)
    sc.assert_sums_close(got, want, what)
    sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], what)          # every slot against its own terms
    sc.assert_sums_bitwise(c.linearize_gicp(T, lin_params(radius)), got, what)          # the plain call: the same sums
    return got


# ---- 1. the dump and the sums against the reference
@pytest.mark.parametrize("pose", ["INIT", "MID", "GT"])
def test_the_lot_is_bitwise_the_reference(lot_ctx, pose):
    L = gs.lot()
    for eps in (1e-3, 1e-2):
        lot_ctx.set_option("gicp_epsilon", eps)
        want = gref.linearize(L["tgt"], L["nb"], L["src"], L["mb"], L[pose], RADIUS, eps)
        check(lot_ctx, want, L[pose], (pose, eps))
    lot_ctx.set_option("gicp_epsilon", gs.EPS)
    assert (want["flag"] == 1).any() and (want["flag"] == 2).any() and (want["flag"] == 3).any()
    want = gref.linearize(L["tgt"], L["nb"], L["src"], L["mb"], L[pose], 0.1, gs.EPS)
    check(lot_ctx, want, L[pose], (pose, "radius 0.1"), 0.1)
    assert (want["flag"] == 0).any() == (pose != "GT")          # (at the truth every point has its map point within 0.1)


@pytest.mark.parametrize("name", ["lattice", "duplicates", "outside", "planted"])
def test_ties_duplicates_queries_outside_the_grid_and_the_planted_flags(name):
    S = {"lattice": gs.lattice_case, "duplicates": gs.duplicate_case, "outside": gs.outside_case, "planted": gs.plant_case}[name]()
    c = context(S["tgt"], S["src"], S["normals"], S["src_normals"])
    try:
        want = gref.linearize(S["tgt"], S["normals"], S["src"], S["src_normals"], S["T"], S["radius"], gs.EPS)
        for _ in range(2):                              # cold, then from the warm words
            got = check(c, want, S["T"], name)
        if name == "planted":
            assert list(got["flag"]) == gs.PLANT_FLAGS and got["nn_idx"][0] == -1        # d2 == R*R stays out
    finally:
        c.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_source_sizes_across_wave_and_block_boundaries(n):
    L = gs.lot()
    src, m = sc.sized_source(n), gs.sized_source_normals(n)
    c = context(L["tgt"], src, L["nb"], m)
    try:
        for pose in ("INIT", "GT"):
            want = gref.linearize(L["tgt"], L["nb"], src, m, L[pose], RADIUS, gs.EPS)
            check(c, want, L[pose], (n, pose))
        if n >= 255:
            assert all((want["flag"] == f).any() for f in (1, 2, 3))
    finally:
        c.close()


def test_the_epsilon_option_refuses_values_outside_its_range(lot_ctx):
    L = gs.lot()
    before = lot_ctx.linearize_gicp(L["INIT"], lin_params())
    for bad in (0.0, 9e-7, 1.0000001, -1.0, np.nan, np.inf):
        with pytest.raises(api.DcregError) as e:
            lot_ctx.set_option("gicp_epsilon", bad)
        assert "(%d)" % api.E_INVALID in str(e.value)
    sc.assert_sums_bitwise(lot_ctx.linearize_gicp(L["INIT"], lin_params()), before)
    for ok in (1e-6, 1.0, gs.EPS):
        lot_ctx.set_option("gicp_epsilon", ok)


# ---- 2. history independence, alone and with the second engine's calls in between
def test_a_walk_is_bitwise_fresh_contexts_with_and_without_the_second_engine_in_between(lot_ctx):
    L = gs.lot()
    mixed = context(L["tgt"], L["src"], L["nb"], L["mb"])
    only_n = context(L["tgt"], L["src"], L["nb"])
    try:
        for step, T in enumerate(sc.walk()):
            fresh = context(L["tgt"], L["src"], L["nb"], L["mb"])
            try:
                want = fresh.linearize_gicp(T, lin_params())
            finally:
                fresh.close()
            want_n = only_n.linearize_normals(T, lin_params())             # the second engine on a context that never ran the third
            a = lot_ctx.linearize_gicp(T, lin_params())                    # carries the words of everything this module did before
            b = lot_ctx.linearize_gicp(T, lin_params())                    # a repeated call
            n1 = mixed.linearize_normals(T, lin_params())                  # the words come from the other engine ...
            g1 = mixed.linearize_gicp(T, lin_params())
            n2 = mixed.linearize_normals(sc.walk()[(step + 2) % 5], lin_params())      # ... and from another pose
            g2 = mixed.linearize_gicp(T, lin_params())
            n3 = mixed.linearize_normals(T, lin_params())
            for x in (a, b, g1, g2):
                sc.assert_sums_bitwise(x, want, step)
            for x in (n1, n3):
                sc.assert_sums_bitwise(x, want_n, step)
            sc.assert_sums_bitwise(n2, only_n.linearize_normals(sc.walk()[(step + 2) % 5], lin_params()), step)
            ref = gref.linearize(L["tgt"], L["nb"], L["src"], L["mb"], T, RADIUS, gs.EPS)
            sc.assert_sums_close(a, ref, step)
            sums.assert_sums_entrywise(a, ref["row"], ref["n_eff"], ref["n_pt"], step)
    finally:
        mixed.close()
        only_n.close()


# ---- 3. the kept source normals
def test_keep_is_bitwise_the_cloud_form_and_set_then_get_round_trips(lot_ctx):
    L = gs.lot()
    for p, key, cur in ((PARAMS_B, "mb", "mcurb"), (PARAMS_5, "m5", "mcur5")):
        c = context(L["tgt"], L["src"])
        try:
            assert c.source_normals_kept() == 0
            info = c.keep_source_normals(p)
            nrm, curv, _, info2 = c.normals(L["src"], p)
            got_n, got_c = c.kept_source_normals()
            assert c.source_normals_kept() == 1 and info == info2
            assert sc.same_bits(got_n, nrm) and sc.same_bits(got_c, curv)
            assert sc.same_bits(got_n, L[key]) and sc.same_bits(got_c, L[cur])
            out = DevCloud(np.full((len(nrm) + 1, 4), 7.0, np.float32))          # one record more than asked for: it must stay
            try:
                assert c.kept_source_normals(dev_ptr=out.ptr, capacity=len(nrm)) is None
                back = read_device(out, len(nrm) + 1, 4)
            finally:
                out.free()
            assert sc.same_bits(back[:-1, :3], nrm) and sc.same_bits(back[:-1, 3], curv) and np.all(back[-1] == 7.0)
            assert np.isfinite(curv).any()
        finally:
            c.close()
    base = lot_ctx.linearize_gicp(L["INIT"], lin_params(), debug=True)
    nrm = np.array(L["mb"])
    c = context(L["tgt"], L["src"], L["nb"])
    dev = DevCloud(strided(nrm, 5))
    out = DevCloud(np.zeros((len(nrm), 4), np.float32))
    try:
        for how in ("host", "strided", "device"):
            if how == "host":
                c.set_source_normals(nrm)
            elif how == "strided":
                c.set_source_normals(strided(nrm, 7, fill=3.0))
            else:
                c.set_source_normals(dev_ptr=dev.ptr, n=dev.n, stride=dev.stride)
            assert c.source_normals_kept() == 1
            got_n, got_c = c.kept_source_normals()
            assert sc.same_bits(got_n, nrm) and np.isnan(got_c).all(), how            # as given, in the order given; no curvature
            got = c.linearize_gicp(L["INIT"], lin_params(), debug=True)
            gs.assert_dump_bitwise(got, base, how)
            sc.assert_sums_bitwise(got, base, how)
            c.drop_source_normals()
            assert c.source_normals_kept() == 0
        c.set_source_normals(nrm)
        assert c.kept_source_normals(dev_ptr=out.ptr, capacity=len(nrm)) is None
        back = read_device(out, len(nrm), 4)
        assert sc.same_bits(back[:, :3], nrm) and np.isnan(back[:, 3]).all()          # as given, in the order given; no curvature
        with pytest.raises(api.DcregError):
            c.set_source_normals(nrm[:-1])              # one normal per source point
        with pytest.raises(api.DcregError):
            c.kept_source_normals(dev_ptr=out.ptr, capacity=len(nrm) - 1)
        assert c.source_normals_kept() == 1
    finally:
        dev.free()
        out.free()
        c.close()


def test_every_new_source_drops_the_source_normals_and_the_batched_calls_leave_them():
    L = gs.lot()
    src = np.array(L["src"])
    c = context(L["tgt"], src, L["nb"])
    dev = DevCloud(strided(src, 4, fill=0.0))
    rec = strided(src, 4, fill=0.0)
    rec[:, 3] = np.linspace(0.0, 0.1, len(rec), dtype=np.float32)
    f, m = api.time_field(3), api.sweep_motion(np.eye(3), [0.01, 0.0, 0.0], (0.0, 0.1), 0.5)
    st = np.array([0.0, 0.05, 0.1])
    P = np.stack([np.eye(4)] * 3)
    P[1, 0, 3], P[2, 0, 3] = 0.005, 0.01
    block = api.sweep_path(0, 3, 0.05)
    forms = (lambda: c.set_source(src), lambda: c.set_source_device(dev.ptr, dev.n, dev.stride), lambda: c.set_source_voxel(src, 0.05),
             lambda: c.set_source_outliers(src, api.outlier_params(k=4, std_mul=5.0)), lambda: c.set_source_deskew(rec, f, m),
             lambda: c.set_source_deskew_path(rec, f, st, P, block))
    try:
        for i, change in enumerate(forms):
            c.keep_source_normals(PARAMS_5)
            assert c.source_normals_kept() == 1 and c.linearize_gicp(L["INIT"], lin_params())["n_pt"] > 0
            change()
            assert c.source_normals_kept() == 0, i
            with pytest.raises(api.DcregError) as e:
                c.linearize_gicp(L["INIT"], lin_params())
            assert "(%d)" % api.E_STATE in str(e.value) and "no kept source normals" in str(e.value)
            with pytest.raises(api.DcregError):
                c.kept_source_normals()
        # the batched calls leave the context's own source as it was, and its normals with it
        c.set_source(src)
        c.set_source_normals(L["mb"])
        before = c.linearize_gicp(L["INIT"], lin_params(), debug=True)
        cfg = cfg_pk01(max_iterations=3)
        c.register_frames_normals([src[:200], src[100:400]], [L["INIT"], L["MID"]], "Ours", cfg)
        c.icp_run_trials_normals([L["INIT"], L["MID"]], "Ours", cfg)
        assert c.source_normals_kept() == 1 and sc.same_bits(c.kept_source_normals()[0], L["mb"])
        after = c.linearize_gicp(L["INIT"], lin_params(), debug=True)
        gs.assert_dump_bitwise(after, before)
        sc.assert_sums_bitwise(after, before)
        # a refused source leaves source and normals as they were
        with pytest.raises(api.DcregError):
            c.set_source(np.full((4, 3), np.nan, np.float32))
        assert c.source_normals_kept() == 1
        sc.assert_sums_bitwise(c.linearize_gicp(L["INIT"], lin_params()), before)
    finally:
        dev.free()
        c.close()


# ---- 4. the window index
def test_the_window_index_changes_no_bit(lot_ctx):
    L = gs.lot()
    w = context(L["tgt"], L["src"], opts=OPTS_WINDOW)
    try:
        w.keep_target_normals(PARAMS_B)
        w.keep_source_normals(PARAMS_B)
        built = []
        for T in (L["INIT"], sc.walk()[3], L["INIT"]):                 # the jump leaves the window's box: a rebuild, and one more on the way back
            want = lot_ctx.linearize_gicp(T, lin_params(), debug=True)
            got = w.linearize_gicp(T, lin_params(), debug=True)
            assert w.roi_info()["active"]
            built.append(w.roi_info()["windows_built"])
            gs.assert_dump_bitwise(got, want)
            sc.assert_sums_bitwise(got, want)
            sc.assert_sums_bitwise(w.linearize_gicp(T, lin_params()), want)
            sc.assert_sums_bitwise(w.linearize_gicp(T, lin_params()), want)         # ... and from the window's own warm words
        assert built[1] > built[0]
        assert w.target_normals_kept() == 1 and w.source_normals_kept() == 1
    finally:
        w.close()


# ---- 5. the engine
@pytest.mark.parametrize("method", ["NONE", "Ours"])
def test_the_engine_follows_the_reference_engine_and_a_python_loop_of_its_parts(method):
    L = gs.lot()
    cfg = cfg_pk01()
    c = context(L["tgt"], L["src"])
    try:
        c.keep_target_normals(PARAMS_5)
        c.keep_source_normals(PARAMS_5)
        T_ref, conv_ref, recs = gref.icp(L["tgt"], L["n5"], L["src"], L["m5"], L["INIT"], cfg, method, eps=gs.EPS)
        res, logs = c.icp_run_gicp(L["INIT"], method, cfg)
        assert (res.status, res.converged, res.iterations) == (0, int(conv_ref), len(recs)) and len(logs) == len(recs)
        for it, (g, r) in enumerate(zip(logs, recs)):
            assert (g.effective_points, g.corr_pt_count) == (r["n_eff"], r["n_pt"]), it
            assert list(g.analysis.degenerate_mask[:]) == r["mask"], it
            err = np.max(np.abs(np.array(g.transform_matrix[:]).reshape(4, 4) - r["T"]))
            print("%s iteration %d: pose difference %.3g" % (method, it, err))
            assert err < 1e-7, (it, err)
            assert g.fitness == r["n_pt"] / 523.0
        t_err, r_err = api.pose_error(L["GT"], np.array(logs[-1].transform_matrix[:]).reshape(4, 4))
        print("%s: %d iterations -> %.4f m %.3f deg" % (method, len(logs), t_err, r_err))
        assert res.converged == 1 and len(logs) <= 10 and t_err < 0.012 and r_err < 0.15
        # the same loop in Python: linearize_gicp + the solver seam + boxplus, bitwise the engine's log
        det, hand = api.METHODS[method]
        T = L["INIT"].copy()
        for it, g in enumerate(logs):
            lin = c.linearize_gicp(T, lin_params(cfg.search_radius))
            assert np.array_equal(lin["H_upper"], g.H_upper[:]) and (lin["n_eff"], lin["n_pt"]) == (g.effective_points, g.corr_pt_count), it
            an = api.analyze_degeneracy(lin["H"], det, hand, cfg)
            dx = api.solve_degenerate_system(lin["H"], lin["g"], hand, cfg, an)
            R, t = api.boxplus(T[:3, :3], T[:3, 3], dx)
            T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
            assert np.array_equal(dx, g.update_dx[:]) and np.array_equal(-lin["g"], g.gradient[:]), it
            assert np.array_equal(T.reshape(16), g.transform_matrix[:]), it
            assert g.rmse == np.sqrt(lin["sum_r2"] / lin["n_eff"]) and g.objective_value == 0.5 * lin["sum_b2"], it
            assert values(an) == values(g.analysis), it
        assert np.array_equal(T[:3, :3].reshape(9), res.R[:]) and np.array_equal(T[:3, 3], res.t[:])
    finally:
        c.close()


def test_a_frame_far_outside_the_map_aborts_with_status_1(lot_ctx):
    L = gs.lot()
    res, logs = lot_ctx.icp_run_gicp(sc.offset(L["INIT"], 500.0, 0.0, 0.0), "Ours", cfg_pk01())
    assert (res.status, res.converged, res.iterations, len(logs)) == (1, 0, 1, 0)
    assert np.array_equal(np.array(res.t[:]), sc.offset(L["INIT"], 500.0, 0.0, 0.0)[:3, 3])


# ---- 6. the other engines do not move
def test_the_other_engines_do_not_move():
    """dcreg_linearize, dcreg_linearize_normals, dcreg_icp_run and dcreg_icp_run_normals give the same bytes without source normals, with
    them, and after calls of the third engine"""
    L = gs.lot()
    c = context(L["tgt"], L["src"])
    c.keep_target_normals(PARAMS_B)
    prm = api.default_lin_params(RADIUS, 1)
    cfg = cfg_pk01(max_iterations=8, use_weight_derivative=1)

    def snapshot():
        out = api.LinOut()
        R, t = np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), np.ascontiguousarray(L["INIT"][:3, 3])
        c.linearize_raw(R, t, prm, out)
        nl = c.linearize_normals(L["INIT"], prm, debug=True)
        recs = []
        for run in (c.icp_run, c.icp_run_normals):
            res, logs = run(L["INIT"], "Ours", cfg)
            for g in logs:
                g.iter_time_ms = 0.0
                recs.append(values(g))
            res.time_ms = 0.0
            recs.append(values(res))
        return values(out), tuple(np.asarray(nl[k]).tobytes() for k in sc.DUMP_KEYS + sc.SUM_KEYS), recs

    try:
        before = snapshot()
        assert len(before[2]) > 4
        c.keep_source_normals(PARAMS_B)
        assert snapshot() == before
        c.linearize_gicp(L["MID"], lin_params())
        assert snapshot() == before
        c.icp_run_gicp(L["INIT"], "Ours", cfg)
        assert snapshot() == before
        c.drop_source_normals()
        assert snapshot() == before
    finally:
        c.close()


# ---- 7. state errors
def test_state_errors_leave_the_results_untouched():
    L = gs.lot()
    c = context(L["tgt"], L["src"])
    try:
        def refused(text):
            out = api.LinOut()
            out.n_eff, out.n_pt, out.sum_r2 = 77, 78, 79.0
            R, t = np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), np.ascontiguousarray(L["INIT"][:3, 3])
            rc = c._L.dcreg_linearize_gicp(c._h, api._dp(R), api._dp(t), C.byref(lin_params()), C.byref(out))
            assert rc == api.E_STATE and text in c._L.dcreg_last_error(c._h).decode() and (out.n_eff, out.n_pt, out.sum_r2) == (77, 78, 79.0)
            with pytest.raises(api.DcregError) as e:
                c.icp_run_gicp(L["INIT"], "Ours", cfg_pk01())
            assert "(%d)" % api.E_STATE in str(e.value)
        refused("no kept normals")
        c.keep_source_normals(PARAMS_5)
        refused("no kept normals")                      # the source's alone do not serve
        c.drop_source_normals()
        c.keep_target_normals(PARAMS_5)
        refused("no kept source normals")
        c.keep_source_normals(PARAMS_5)
        assert c.linearize_gicp(L["INIT"], lin_params())["n_eff"] == 523
        c.set_target(L["tgt"], RADIUS)                  # a new map drops its normals, not the source's
        assert c.source_normals_kept() == 1
        refused("no kept normals")
    finally:
        c.close()
    e = api.Context(0)
    try:
        e.set_target(L["tgt"], RADIUS)
        with pytest.raises(api.DcregError) as err:
            e.keep_source_normals(PARAMS_5)             # no source
        assert "(%d)" % api.E_STATE in str(err.value)
        with pytest.raises(api.DcregError) as err:
            e.set_source_normals(np.array(L["m5"]))
        assert "(%d)" % api.E_STATE in str(err.value)
    finally:
        e.close()
