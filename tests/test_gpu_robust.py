"""The robust kernels of the second and third engine on the device (the options "robust_kernel", "robust_scale", "gicp_robust_scale" of
include/dcreg.h) against the numpy reference of tests/robust_ref.py: the per-point dump BITWISE, every one of the 31 sums within the
derived bound of the exact sum over the reference's scaled rows (tests/sums_check.py), the counts exactly.  The planted Huber edge, sizes
across wave and block boundaries, a source past one chunk, "off is off" (kernel 0 returns the bytes of a context that never heard of the
options, refused values change nothing), history independence, and the engines on the contaminated frame of tests/robust_scenes.py."""
import functools

import numpy as np
import pytest

import gicp_scenes as gs
import normal_icp_ref as ref
import normal_icp_scenes as sc
import robust_ref as rr
import robust_scenes as rs
import sums_check as sums
import test_gpu_frames_gicp as fg
import test_gpu_frames_normals as fn
import test_gpu_one_nn_chunks as chunks
from dcreg_amd import api
from test_gpu_normals import OPTS_WINDOW
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
ENGINES = ["normals", "gicp"]
SCALE_KEY = {"normals": "robust_scale", "gicp": "gicp_robust_scale"}
SCALES = {"normals": rs.SCALES_N, "gicp": rs.SCALES_G}


def lin_params():
    return api.default_lin_params(RADIUS, 1)


def lot_context(engine, opts=()):
    """the lot's map with its bounded normals, the frame as the source (with its bounded normals for the third engine)"""
    L = gs.lot()
    return fn.context(L["src"]) if engine == "normals" and not opts else fg.context(L["src"], L["mb"] if engine == "gicp" else None, opts=opts)


def linearize(c, engine, T, debug=False):
    return (c.linearize_normals if engine == "normals" else c.linearize_gicp)(T, lin_params(), debug=debug)


def reference(engine, src, m, T, kind, c, nn=None):
    L = gs.lot()
    if engine == "normals":
        return rr.linearize_normals(L["tgt"], L["nb"], src, T, RADIUS, kind, c, use_weight_derivative=1, nn=nn)
    return rr.linearize_gicp(L["tgt"], L["nb"], src, m, T, RADIUS, kind, c, gs.EPS, nn=nn)


def assert_dump(engine, got, want, what):
    (sc if engine == "normals" else gs).assert_dump_bitwise(got, want, what)


def assert_same(engine, a, b, what=""):
    assert_dump(engine, a, b, what)
    sc.assert_sums_bitwise(a, b, what)


@functools.lru_cache(maxsize=None)
def walk_nearest():
    L = gs.lot()
    return [ref.nearest(L["tgt"], ref.transform(T[:3, :3], T[:3, 3], L["src"])) for T in sc.walk()]


@pytest.fixture(scope="module")
def ctx():
    cs = {e: lot_context(e) for e in ENGINES}
    yield cs
    for c in cs.values():
        c.close()


# ---- 1. dump and sums
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("kind", rs.KINDS)
@pytest.mark.parametrize("small", [True, False])
def test_the_dump_is_bitwise_the_reference_and_the_sums_are_its_rows(ctx, engine, kind, small):
    L = gs.lot()
    c = ctx[engine]
    scale = (min if small else max)(SCALES[engine])
    c.set_option("robust_kernel", kind)
    c.set_option(SCALE_KEY[engine], scale)
    try:
        for step, T in enumerate(sc.walk()):
            want = reference(engine, L["src"], L["mb"], T, kind, scale, walk_nearest()[step])
            got = linearize(c, engine, T, debug=True)
            what = (engine, kind, scale, step)
            assert_dump(engine, got, want, what)
            sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], what)
            sc.assert_sums_bitwise(linearize(c, engine, T), got, what)              # the plain call: the same sums
        plain = reference(engine, L["src"], L["mb"], T, 0, scale, walk_nearest()[step])
        assert want["n_eff"] == plain["n_eff"] > 100 and not np.array_equal(want["H_upper"], plain["H_upper"])      # the kernel did something
    finally:
        c.set_option("robust_kernel", 0)


# ---- 2. the planted Huber edge
def test_the_planted_huber_edge_of_the_second_engine():
    c = api.Context(0)
    try:
        c.set_target(rs.EDGE_MAP, RADIUS)
        c.set_source(rs.EDGE_SRC)
        c.set_target_normals(rs.EDGE_NORMALS)
        c.set_option("robust_kernel", api.ROBUST["huber"])
        c.set_option("robust_scale", rs.EDGE_SCALE)
        got = c.linearize_normals(np.eye(4), api.default_lin_params(RADIUS, 0), debug=True)
        want = rr.linearize_normals(rs.EDGE_MAP, rs.EDGE_NORMALS, rs.EDGE_SRC, np.eye(4), RADIUS, 1, rs.EDGE_SCALE)
        assert list(got["flag"]) == [1, 1, 1] and list(got["r"]) == [0.0, 0.125, 0.25]
        assert rs.EDGE_K[:2] == (1.0, 1.0) and rs.EDGE_K[2] == np.sqrt(np.float64(0.5))
        assert tuple(got["row"][:, 5]) == tuple(np.array(rs.EDGE_K) * got["s"])         # m2 = 1, w = s: slot 5 is k * s, rounded once
        assert tuple(got["row"][:, 5] / got["s"]) == rs.EDGE_K
        sc.assert_dump_bitwise(got, want)
    finally:
        c.close()


def test_the_planted_huber_edge_of_the_third_engine():
    E = rs.gicp_edge()
    c = api.Context(0)
    try:
        c.set_target(rs.EDGE_MAP, RADIUS)
        c.set_source(E["src"])
        c.set_target_normals(rs.EDGE_NORMALS)
        c.set_source_normals(E["src_normals"])
        plain = c.linearize_gicp(np.eye(4), lin_params(), debug=True)
        c.set_option("robust_kernel", api.ROBUST["huber"])
        c.set_option("gicp_robust_scale", E["c"])
        got = c.linearize_gicp(np.eye(4), lin_params(), debug=True)
        want = rr.linearize_gicp(rs.EDGE_MAP, rs.EDGE_NORMALS, E["src"], E["src_normals"], np.eye(4), RADIUS, 1, E["c"], gs.EPS)
        assert list(got["flag"]) == [1, 1, 1]
        assert E["k"][:2] == (1.0, 1.0) and 0.5 < E["k"][2] < 1.0
        assert tuple(got["row"][:, 2, 5]) == tuple(np.array(E["k"]) * plain["row"][:, 2, 5])
        assert tuple(got["row"][:, 2, 5] / plain["row"][:, 2, 5]) == E["k"]
        assert np.array_equal(got["r"], plain["r"])                                     # slot 7 and the dumped r stay the residual
        gs.assert_dump_bitwise(got, want)
    finally:
        c.close()


# ---- 3. sizes across wave and block boundaries
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_source_sizes_across_wave_and_block_boundaries(n):
    L = gs.lot()
    src, m = sc.sized_source(n), gs.sized_source_normals(n)
    for engine, scale in (("normals", 0.1), ("gicp", 1.0)):
        c = fn.context(src) if engine == "normals" else fg.context(src, m)
        try:
            c.set_option("robust_kernel", api.ROBUST["cauchy"])
            c.set_option(SCALE_KEY[engine], scale)
            want = reference(engine, src, m, L["INIT"], 2, scale)
            got = linearize(c, engine, L["INIT"], debug=True)
            assert_dump(engine, got, want, (engine, n))
            sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], (engine, n))
            sc.assert_sums_bitwise(linearize(c, engine, L["INIT"]), got, (engine, n))
        finally:
            c.close()


# ---- 4. past one chunk of the reduction (the case of tests/test_gpu_one_nn_chunks.py: a second chunk of one block holding one point)
@pytest.mark.parametrize("engine", ENGINES)
def test_a_source_past_one_chunk(engine):
    n = 16385
    T = sc.walk()[chunks.POSE_OF[n]]
    scale = {"normals": 0.1, "gicp": 1.0}[engine]
    want = reference(engine, sc.sized_source(n), gs.sized_source_normals(n), T, 2, scale)
    assert want["n_eff"] > n // 4
    c = chunks.context(engine, n)
    try:
        c.set_option("robust_kernel", api.ROBUST["cauchy"])
        c.set_option(SCALE_KEY[engine], scale)
        cold = linearize(c, engine, T)
        got = linearize(c, engine, T, debug=True)
    finally:
        c.close()
    assert_dump(engine, got, want, (engine, n))
    sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], (engine, n))
    sc.assert_sums_bitwise(cold, got, (engine, n))


# ---- 5. off is off
BAD_KERNELS = (4.0, 1.5, -1.0, np.nan, np.inf)
BAD_SCALES = (0.0, -1.0, 1.0e7, 9.0e-7, np.inf, np.nan)


@pytest.mark.parametrize("engine", ENGINES)
def test_off_is_off_and_a_refused_value_changes_nothing(engine):
    L = gs.lot()
    T = L["INIT"]
    fresh = lot_context(engine)
    c = lot_context(engine)
    try:
        base = linearize(fresh, engine, T, debug=True)
        c.set_option("robust_kernel", 0)
        c.set_option("robust_scale", 0.02)
        c.set_option("gicp_robust_scale", 0.02)
        assert_same(engine, linearize(c, engine, T, debug=True), base, "kernel 0, scales set")
        sc.assert_sums_bitwise(linearize(c, engine, T), base)
        c.set_option("robust_kernel", 2)
        on = linearize(c, engine, T, debug=True)
        assert on["n_eff"] == base["n_eff"] and on["n_pt"] == base["n_pt"] and not np.array_equal(on["H_upper"], base["H_upper"])
        assert_dump(engine, on, reference(engine, L["src"], L["mb"], T, 2, 0.02), "kernel 2")
        c.set_option("robust_kernel", 0)
        assert_same(engine, linearize(c, engine, T, debug=True), base, "kernel 2, then 0")
        # refused values: DCREG_E_INVALID, and the next launch has the bits from before
        c.set_option("robust_kernel", 2)
        for key, bad in [("robust_kernel", v) for v in BAD_KERNELS] + [(k, v) for k in ("robust_scale", "gicp_robust_scale") for v in BAD_SCALES]:
            with pytest.raises(api.DcregError) as e:
                c.set_option(key, bad)
            assert "(%d)" % api.E_INVALID in str(e.value), (key, bad)
            sc.assert_sums_bitwise(linearize(c, engine, T), on, (key, bad))
        assert_same(engine, linearize(c, engine, T, debug=True), on, "after the refusals")
        for key, ok in (("robust_scale", 1e-6), ("robust_scale", 1e6), ("gicp_robust_scale", 1e-6), ("gicp_robust_scale", 1e6), ("robust_kernel", 3.0)):
            c.set_option(key, ok)
    finally:
        fresh.close()
        c.close()


# ---- 6. history independence
def test_history_interleaved_engines_and_the_window_index_change_no_bit(ctx):
    L = gs.lot()
    GM = api.ROBUST["geman_mcclure"]
    mixed = lot_context("gicp")
    window = lot_context("gicp", opts=OPTS_WINDOW)
    for c in (ctx["normals"], ctx["gicp"], mixed, window):
        c.set_robust(GM, 0.05, 1.0)
    try:
        for step, T in enumerate(sc.walk()):
            want = {}
            for engine in ENGINES:
                fresh = lot_context(engine)
                try:
                    fresh.set_robust("geman_mcclure", scale=0.05, gicp_scale=1.0)
                    want[engine] = linearize(fresh, engine, T)
                finally:
                    fresh.close()
                ref_e = reference(engine, L["src"], L["mb"], T, GM, {"normals": 0.05, "gicp": 1.0}[engine], walk_nearest()[step])
                sums.assert_sums_entrywise(want[engine], ref_e["row"], ref_e["n_eff"], ref_e["n_pt"], (engine, step))
                sc.assert_sums_bitwise(linearize(ctx[engine], engine, T), want[engine], (engine, step))       # the walk in order
                sc.assert_sums_bitwise(linearize(ctx[engine], engine, T), want[engine], (engine, step))       # a repeated call
            other = sc.walk()[(step + 2) % 5]
            n1 = mixed.linearize_normals(T, lin_params())
            g1 = mixed.linearize_gicp(T, lin_params())
            mixed.linearize_normals(other, lin_params())                                 # the words now come from another pose
            g2 = mixed.linearize_gicp(T, lin_params())
            n2 = mixed.linearize_normals(T, lin_params())
            for x in (g1, g2):
                sc.assert_sums_bitwise(x, want["gicp"], step)
            for x in (n1, n2):
                sc.assert_sums_bitwise(x, want["normals"], step)
            sc.assert_sums_bitwise(window.linearize_normals(T, lin_params()), want["normals"], ("window", step))
            sc.assert_sums_bitwise(window.linearize_gicp(T, lin_params()), want["gicp"], ("window", step))
            assert window.roi_info()["active"]
    finally:
        for c in (ctx["normals"], ctx["gicp"]):
            c.set_option("robust_kernel", 0)
        mixed.close()
        window.close()


# ---- 7. the engines on the contaminated frame
@pytest.mark.parametrize("engine", ENGINES)
def test_the_engines_follow_the_reference_engines_on_the_contaminated_frame(engine):
    L, S = gs.lot(), rs.contaminated()
    cfg = cfg_pk01(max_iterations=40)
    c = api.Context(0)
    try:
        c.set_target(L["tgt"], RADIUS)
        c.set_source(S["src"])
        c.set_target_normals(np.ascontiguousarray(L["n5"], np.float32))
        if engine == "gicp":
            c.set_source_normals(np.ascontiguousarray(S["m5"], np.float32))
        run = c.icp_run_normals if engine == "normals" else c.icp_run_gicp
        final = {}
        for kind in (rs.GM, 0):
            c.set_robust(kind, scale=rs.C_N, gicp_scale=rs.C_G)
            T_ref, conv_ref, recs = rs.reference_run(engine, "dirty", kind)
            res, logs = run(L["INIT"], "NONE", cfg, log_capacity=40)
            assert (res.status, res.converged, res.iterations) == (0, int(conv_ref), len(recs)) and len(logs) == len(recs), kind
            for it, (g, r) in enumerate(zip(logs, recs)):
                assert (g.effective_points, g.corr_pt_count) == (r["n_eff"], r["n_pt"]), (kind, it)
                assert list(g.analysis.degenerate_mask[:]) == r["mask"], (kind, it)
                err = np.max(np.abs(np.array(g.transform_matrix[:]).reshape(4, 4) - r["T"]))
                assert err < 1e-7, (kind, it, err)
                assert g.fitness == r["n_pt"] / 523.0
            final[kind] = rs.rot_trans_error(np.array(logs[-1].transform_matrix[:]).reshape(4, 4), L["GT"])
            print("%s, kernel %d: %d iterations -> %.4f m %.3f deg" % (engine, kind, len(logs), final[kind][0], final[kind][1]))
            # the log's H_upper is the scaled Hessian: the linearisation at the pose before the last step, with the same options
            T_prev = np.array(logs[-2].transform_matrix[:]).reshape(4, 4)
            prm = api.default_lin_params(cfg.search_radius, cfg.use_weight_derivative)
            lin = (c.linearize_normals if engine == "normals" else c.linearize_gicp)(T_prev, prm)
            assert np.array_equal(lin["H_upper"], logs[-1].H_upper[:]) and logs[-1].rmse == np.sqrt(lin["sum_r2"] / lin["n_eff"])
        assert final[rs.GM][1] < 0.5 and final[0][1] > 1.0
    finally:
        c.close()
