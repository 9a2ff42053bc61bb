"""The second engine on the device (dcreg_target_normals_keep / _set, dcreg_linearize_normals, dcreg_icp_run_normals) against the numpy
reference of tests/normal_icp_ref.py, which applies include/dcreg.h's rule literally: the per-point dump must be BITWISE the reference's,
the sums agree with the exactly rounded sums of the reference rows to the tolerances of tests/test_gpu_parity.py, the counts exactly; every sum also lies within the derived bound of the
exact sum over the reference's rows (tests/sums_check.py).
History, context and window index change no bit; the first engine's results do not move."""
import ctypes as C

import numpy as np
import pytest

import normal_icp_ref as ref
import normal_icp_scenes as sc
import sums_check as sums
from dcreg_amd import api
from test_gpu_device_seam import DevCloud, strided
from test_gpu_normals import OPTS_WINDOW
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
PARAMS_B = api.normal_params(k=5, search_radius=RADIUS)


def lin_params(radius=RADIUS, wd=1, slope=None):
    p = api.default_lin_params(radius, wd)
    if slope is not None:
        p.weight_slope = slope
    return p


def values(o):
    """a ctypes record as nested tuples of its fields' bit patterns (padding bytes are nobody's)"""
    if isinstance(o, C.Structure):
        return tuple(values(getattr(o, f[0])) for f in o._fields_)
    if isinstance(o, C.Array):
        return tuple(values(x) for x in o)
    return np.float64(o).tobytes() if isinstance(o, float) else o


def context(tgt, src, normals=None, opts=()):
    c = api.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_target(tgt, RADIUS)
    if src is not None:
        c.set_source(src)
    if normals is not None:
        c.set_target_normals(np.ascontiguousarray(normals, np.float32))
    return c


@pytest.fixture(scope="module")
def lot_ctx():
    """the lot with its frame as the source and the bounded normals kept"""
    L = sc.lot()
    c = context(L["tgt"], L["src"])
    c.keep_target_normals(PARAMS_B)
    yield c
    c.close()


# ---- 1. the dump against the reference
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4099])
def test_the_dump_is_bitwise_the_reference_across_wave_and_block_boundaries(n):
    L = sc.lot()
    src = sc.sized_source(n)
    c = context(L["tgt"], src)
    try:
        for name, p in (("n5", api.normal_params(k=5)), ("nb", PARAMS_B)):
            info = c.keep_target_normals(p)
            assert info["n_sparse"] == (0 if name == "n5" else 1065) and c.target_normals_kept() == 1
            for pose in ("INIT", "MID"):
                nn = ref.nearest(L["tgt"], ref.transform(L[pose][:3, :3], L[pose][:3, 3], src))
                for radius in (0.5, 0.1):
                    for wd in (0, 1):
                        want = ref.linearize(L["tgt"], L[name], src, L[pose], radius, use_weight_derivative=wd, nn=nn)
                        got = c.linearize_normals(L[pose], lin_params(radius, wd), debug=True)
                        what = (n, name, pose, radius, wd)
                        sc.assert_dump_bitwise(got, want, what)
                        sc.assert_sums_close(got, want, what)
                        sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], what)     # every slot against its own terms
                        sc.assert_sums_bitwise(c.linearize_normals(L[pose], lin_params(radius, wd)), got, what)     # the plain call: the same sums
        if n >= 255:
            assert (want["flag"] == 0).any() and (want["flag"] == 1).any() and (want["flag"] == 2).any()
    finally:
        c.close()


# ---- 2. ties, duplicates, gates
@pytest.mark.parametrize("name", ["lattice", "duplicates", "outside"])
def test_ties_duplicates_and_queries_outside_the_grid(name):
    S = {"lattice": sc.lattice_case, "duplicates": sc.duplicate_case, "outside": sc.outside_case}[name]()
    c = context(S["tgt"], S["src"], S["normals"])
    try:
        want = ref.linearize(S["tgt"], S["normals"], S["src"], S["T"], S["radius"], use_weight_derivative=1)
        for _ in range(2):                              # cold, then from the warm words
            got = c.linearize_normals(S["T"], lin_params(), debug=True)
            sc.assert_dump_bitwise(got, want, name)
            sc.assert_sums_close(got, want, name)
            sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], name)
            plain = c.linearize_normals(S["T"], lin_params())
            sc.assert_sums_bitwise(plain, got, name)
    finally:
        c.close()


@pytest.mark.parametrize("slope", sc.GATE_SLOPES)
def test_the_planted_gates(slope):
    G = sc.gate_case()
    c = context(G["tgt"], G["src"], G["normals"])
    try:
        want = ref.linearize(G["tgt"], G["normals"], G["src"], G["T"], G["radius"], weight_slope=slope, use_weight_derivative=1)
        got = c.linearize_normals(G["T"], lin_params(slope=slope), debug=True)
        assert list(got["flag"]) == sc.GATE_FLAGS and got["nn_idx"][0] == -1        # d2 == R*R stays out
        sc.assert_dump_bitwise(got, want, slope)
        sc.assert_sums_close(got, want, slope)
        sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], slope)
    finally:
        c.close()


def test_a_map_without_any_normal_has_no_effective_point():
    L = sc.lot()
    c = context(L["tgt"], L["src"], np.full((len(L["tgt"]), 3), np.nan, np.float32))
    try:
        got = c.linearize_normals(L["INIT"], lin_params(), debug=True)
        assert got["n_eff"] == 0 and got["n_pt"] == 523 and (got["flag"] == 2).all()
        assert not got["H_upper"].any() and not got["g"].any() and got["sum_r2"] == 0.0 and got["sum_b2"] == 0.0
        res, logs = c.icp_run_normals(L["INIT"], "NONE", cfg_pk01())
        assert (res.status, res.converged, res.iterations, len(logs)) == (1, 0, 1, 0)
    finally:
        c.close()


# ---- 3. keep equals set
def test_keep_equals_set_of_the_map_normals_host_strided_and_device(lot_ctx):
    L = sc.lot()
    base = lot_ctx.linearize_normals(L["INIT"], lin_params(), debug=True)
    nrm, cur, _, info = lot_ctx.target_normals(PARAMS_B)
    assert sc.same_bits(nrm, L["nb"]) and info["n_sparse"] == 1065
    c = context(L["tgt"], L["src"])
    dev = DevCloud(strided(nrm, 5))
    try:
        assert c.target_normals_kept() == 0
        for how in ("host", "strided", "device"):
            if how == "host":
                c.set_target_normals(nrm)
            elif how == "strided":
                c.set_target_normals(strided(nrm, 7, fill=3.0))
            else:
                c.set_target_normals(dev_ptr=dev.ptr, n=dev.n, stride=dev.stride)
            assert c.target_normals_kept() == 1
            got = c.linearize_normals(L["INIT"], lin_params(), debug=True)
            sc.assert_dump_bitwise(got, base, how)
            sc.assert_sums_bitwise(got, base, how)
            c.drop_target_normals()
            assert c.target_normals_kept() == 0
        c.set_target_normals(-nrm)
        flipped = c.linearize_normals(L["INIT"], lin_params(), debug=True)
        sc.assert_sums_bitwise(flipped, base, "flipped")
        eff = base["flag"] == 1
        assert np.array_equal(flipped["flag"], base["flag"]) and sc.same_bits(flipped["r"][eff], -base["r"][eff])
        with pytest.raises(api.DcregError):
            c.set_target_normals(nrm[:-1])              # one normal per map point
        assert c.target_normals_kept() == 1
    finally:
        dev.free()
        c.close()


# ---- 4. history independence
def test_a_walk_is_bitwise_a_fresh_context_at_every_pose(lot_ctx):
    L = sc.lot()
    other = context(L["tgt"], L["src"])
    other.keep_target_normals(PARAMS_B)
    try:
        for step, T in enumerate(sc.walk()):
            fresh = context(L["tgt"], L["src"], L["nb"])
            try:
                want = fresh.linearize_normals(T, lin_params(), debug=True)
                sc.assert_sums_bitwise(fresh.linearize_normals(T, lin_params()), want, step)
            finally:
                fresh.close()
            a = lot_ctx.linearize_normals(T, lin_params())             # carries the words of everything this module did before
            b = lot_ctx.linearize_normals(T, lin_params())             # a repeated call
            o = other.linearize_normals(T, lin_params())               # a second context
            d = lot_ctx.linearize_normals(T, lin_params(), debug=True)
            for x in (a, b, o, d):
                sc.assert_sums_bitwise(x, want, step)
            sc.assert_dump_bitwise(d, want, step)
            want_ref = ref.linearize(L["tgt"], L["nb"], L["src"], T, RADIUS, use_weight_derivative=1)
            sc.assert_dump_bitwise(d, want_ref, step)
            sums.assert_sums_entrywise(d, want_ref["row"], want_ref["n_eff"], want_ref["n_pt"], step)
    finally:
        other.close()


# ---- 5. the window index
def test_the_window_index_changes_no_bit(lot_ctx):
    L = sc.lot()
    w = context(L["tgt"], L["src"], opts=OPTS_WINDOW)
    try:
        w.keep_target_normals(PARAMS_B)
        built = []
        for T in (L["INIT"], sc.walk()[3], L["INIT"]):                 # the jump leaves the window's box: a rebuild, and one more on the way back
            want = lot_ctx.linearize_normals(T, lin_params(), debug=True)
            got = w.linearize_normals(T, lin_params(), debug=True)
            assert w.roi_info()["active"]
            built.append(w.roi_info()["windows_built"])
            sc.assert_dump_bitwise(got, want)
            sc.assert_sums_bitwise(got, want)
            sc.assert_sums_bitwise(w.linearize_normals(T, lin_params()), want)
            sc.assert_sums_bitwise(w.linearize_normals(T, lin_params()), want)         # ... and from the window's own warm words
        assert built[1] > built[0]
        assert w.target_normals_kept() == 1
    finally:
        w.close()


# ---- 6. invalidation and non-interference
def test_every_change_of_the_map_drops_the_kept_normals():
    L = sc.lot()
    c = context(L["tgt"], L["src"])
    try:
        def refused():
            assert c.target_normals_kept() == 0
            with pytest.raises(api.DcregError) as e:
                c.linearize_normals(L["INIT"], lin_params())
            assert "(%d)" % api.E_STATE in str(e.value) and "no kept normals" in str(e.value)
        refused()                                                      # nothing kept yet
        for change in (lambda: c.insert_source(L["GT"], 0.05), lambda: c.crop(L["tgt"].min(axis=0) + 1.0, L["tgt"].max(axis=0) - 1.0),
                       lambda: c.set_target(L["tgt"], RADIUS)):
            c.keep_target_normals(PARAMS_B)
            assert c.target_normals_kept() == 1 and c.linearize_normals(L["INIT"], lin_params())["n_pt"] > 0
            change()
            refused()
        # a new source keeps the normals (they belong to the map) and starts cold
        c.keep_target_normals(PARAMS_B)
        base = c.linearize_normals(L["INIT"], lin_params(), debug=True)
        c.set_source(L["src"][::-1].copy())
        assert c.target_normals_kept() == 1
        again = c.linearize_normals(L["INIT"], lin_params(), debug=True)
        sc.assert_dump_bitwise({k: again[k][::-1] for k in sc.DUMP_KEYS}, base)
    finally:
        c.close()


def test_the_first_engine_does_not_move():
    """dcreg_linearize and dcreg_icp_run give the same bytes before keep, after keep and after a linearize_normals call"""
    L = sc.lot()
    c = context(L["tgt"], L["src"])
    prm = api.default_lin_params(RADIUS, 1)
    cfg = cfg_pk01(max_iterations=8, use_weight_derivative=1)

    def snapshot():
        out = api.LinOut()
        R, t = np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), np.ascontiguousarray(L["INIT"][:3, 3])
        c.linearize_raw(R, t, prm, out)
        res, logs = c.icp_run(L["INIT"], "Ours", cfg)
        recs = []
        for g in logs:
            g.iter_time_ms = 0.0
            recs.append(values(g))
        res.time_ms = 0.0
        return values(out), values(res), recs

    try:
        before = snapshot()
        assert len(before[2]) > 1
        c.keep_target_normals(PARAMS_B)
        assert snapshot() == before
        c.linearize_normals(L["MID"], lin_params())
        assert snapshot() == before
        c.icp_run_normals(L["INIT"], "Ours", cfg)
        assert snapshot() == before
    finally:
        c.close()


# ---- 7. the engine
@pytest.mark.parametrize("method", ["NONE", "Ours"])
def test_the_engine_follows_the_reference_engine_and_a_python_loop_of_its_parts(method):
    L = sc.lot()
    cfg = cfg_pk01()
    c = context(L["tgt"], L["src"])
    try:
        c.keep_target_normals(api.normal_params(k=5))
        T_ref, conv_ref, recs = ref.icp(L["tgt"], L["n5"], L["src"], L["INIT"], cfg, method)
        res, logs = c.icp_run_normals(L["INIT"], method, cfg)
        assert (res.status, res.converged, res.iterations) == (0, int(conv_ref), len(recs)) and len(logs) == len(recs)
        for it, (g, r) in enumerate(zip(logs, recs)):
            assert (g.effective_points, g.corr_pt_count) == (r["n_eff"], r["n_pt"]), it
            assert list(g.analysis.degenerate_mask[:]) == r["mask"], it
            err = np.max(np.abs(np.array(g.transform_matrix[:]).reshape(4, 4) - r["T"]))
            print("%s iteration %d: pose difference %.3g" % (method, it, err))
            assert err < 1e-7, (it, err)
            assert g.fitness == r["n_pt"] / 523.0
        t_err, r_err = api.pose_error(L["GT"], np.array(logs[-1].transform_matrix[:]).reshape(4, 4))
        assert t_err < 0.229 / 5 and r_err < 2.53 / 5
        # the same loop in Python: linearize_normals + the solver seam + boxplus, bitwise the engine's log
        det, hand = api.METHODS[method]
        T = L["INIT"].copy()
        for it, g in enumerate(logs):
            lin = c.linearize_normals(T, lin_params(cfg.search_radius, cfg.use_weight_derivative))
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
    L = sc.lot()
    res, logs = lot_ctx.icp_run_normals(sc.offset(L["INIT"], 500.0, 0.0, 0.0), "Ours", cfg_pk01())
    assert (res.status, res.converged, res.iterations, len(logs)) == (1, 0, 1, 0)
    assert np.array_equal(np.array(res.t[:]), sc.offset(L["INIT"], 500.0, 0.0, 0.0)[:3, 3])
