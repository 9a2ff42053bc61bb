"""The kept voxel map and the fourth engine at their edges (dcreg_target_voxels_keep / _get, dcreg_linearize_voxels, dcreg_icp_run_voxels,
and the voxel pass they share with dcreg_voxel_downsample): leaves that binary cannot represent, a voxel box as wide as the key allows
and the refusal one voxel beyond it, lookup tables of two slots and around a doubling, one voxel of 20 000 points, and a map 1e5 m from
the origin.  The scenes are those of tests/voxels_edge_scenes.py (tests/test_voxels_edge_scenes.py shows on the CPU that they have
teeth).  Every comparison is the usual one: the kept records and the dump BITWISE the numpy reference's (tests/voxels_ref.py), the
counts exact, every one of the 31 sums within the derived bound of the exact sum over the REFERENCE's rows (tests/sums_check.py), the
plain call, the second call and the dump call bitwise equal."""
import numpy as np
import pytest

import sums_check as sums
import normal_icp_scenes as sc
import voxels_edge_scenes as es
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api
from test_gpu_normals import OPTS_WINDOW
from test_gpu_voxel import same, voxel_ref
from test_gpu_voxels import INFO_KEYS, MAP_PARAMS, RADIUS, context, lin_params
from test_gpu_voxels_engine import values
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu


def keep(c, S, params=MAP_PARAMS, what=""):
    """keep_target_voxels: the info and the records bitwise the scene's reference map"""
    info = c.keep_target_voxels(params)
    assert info == {k: S["vmap"][k] for k in INFO_KEYS}, (what, info)
    assert c.target_voxels_kept() == S["vmap"]["n_kept"]
    got = c.kept_target_voxels()
    vs.assert_map_bitwise(got, S["vmap"], what)
    return got


def check(c, want, T, what):
    """the dump bitwise, the counts, the sums entry by entry over the reference's rows; plain call = second call = dump call"""
    got = c.linearize_voxels(T, lin_params(), debug=True)
    vs.assert_dump_bitwise(got, want, what)
    worst = sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], what)
    print("%s: %d points, n_eff %d, the largest error is %.3g of its bound" % (what, len(want["flag"]), want["n_eff"], worst))
    plain = c.linearize_voxels(T, lin_params())
    sc.assert_sums_bitwise(plain, got, what)
    sc.assert_sums_bitwise(c.linearize_voxels(T, lin_params()), plain, what)
    return got


def scene_context(S, mode, params=MAP_PARAMS, opts=()):
    c = context(S["tgt"], S["src"], S["src_normals"] if mode else None, mode, keep=False, opts=opts)
    keep(c, S, params)
    return c


def untimed(o):
    """a result or log record as its fields' bit patterns, without the clock's"""
    return tuple(values(getattr(o, f[0])) for f in o._fields_ if not f[0].endswith("time_ms"))


def refused(call, text=""):
    with pytest.raises(api.DcregError) as e:
        call()
    assert "(%d)" % api.E_INVALID in str(e.value) and text in str(e.value), str(e.value)


# ---- 1. a leaf that binary cannot represent: voxel_of (the key pass, the map keep) and vmap_find (the engine) state the rule twice
@pytest.mark.parametrize("leaf", [0.1, 0.7])
def test_a_leaf_that_binary_cannot_represent_is_divided_by_in_double(leaf):
    S = es.leafy(leaf)
    params = api.voxel_map_params(*S["params"])
    for mode in (0, 1):
        c = scene_context(S, mode, params)
        try:
            want = vr.linearize(S["vmap"], S["src"], S["T"], mode, S["src_normals"] if mode else None, vs.GICP_EPS)
            assert want["n_pt"] == S["n_face"] and (want["voxel_idx"][S["n_face"]:] == -1).all()
            got = check(c, want, S["T"], "leaf %g, mode %d" % (leaf, mode))
            assert np.array_equal(got["voxel_idx"], want["voxel_idx"])
        finally:
            c.close()


@pytest.mark.parametrize("leaf", [0.1, 0.7])
def test_the_key_pass_divides_by_such_a_leaf_in_double(leaf):
    S = es.leafy(leaf)
    c = api.Context(0)
    try:
        for name in ("tgt", "src"):
            for mode in ("centroid", "first"):
                for mp in (1, 2):
                    out, info = c.voxel_downsample([S[name]], leaf, mode, min_points=mp)
                    ref = voxel_ref(S[name], leaf, mode, mp)
                    assert same(out[0], ref), (leaf, name, mode, mp, out[0].shape, ref.shape)
                    assert info["n_out"] == len(ref) and info["n_voxels"] == len(voxel_ref(S[name], leaf, "first", 1))
        assert len(voxel_ref(S["tgt"], leaf, "first", 1)) == S["vmap"]["n_voxels"]
    finally:
        c.close()


# ---- 2. key widths at the limit: 21 bits per axis, 63 bits of voxel key, a 64-bit sort key
TOP = (1 << 20) - 2


@pytest.mark.parametrize("mode", [0, 1])
def test_a_map_2_pow_21_minus_1_voxels_wide_is_kept_and_looked_up(mode):
    W = es.wide(TOP)
    assert W["span"] == (es.WIDE_SPAN_MAX,) * 3
    c = scene_context(W, mode, api.voxel_map_params(es.WIDE_LEAF, vs.EPS, vs.MIN_POINTS))
    try:
        got = c.kept_target_voxels()
        assert got["coords"].min() == -1048576 and got["coords"].max() == TOP
        for name in ("T", "T_step"):
            want = vr.linearize(W["vmap"], W["src"], W[name], mode, W["src_normals"] if mode else None, vs.GICP_EPS)
            assert want["n_eff"] > 0 and (want["voxel_idx"] == -1).any()
            dump = check(c, want, W[name], "span 2^21 - 1, mode %d, %s" % (mode, name))
            assert np.array_equal(dump["voxel_idx"], want["voxel_idx"])
        assert set(want["voxel_idx"].tolist()) >= {-1, 1, 2, 3}
    finally:
        c.close()


def test_the_voxel_pass_sorts_a_64_bit_key():
    W = es.wide(TOP)
    c = api.Context(0)
    try:
        for cloud in (W["tgt"], W["src"][:-18]):                           # (the last 18 source points lie outside the box: 2^21 + 1 voxels)
            for mode in ("centroid", "first"):
                for mp in (1, 6):
                    out, info = c.voxel_downsample([cloud], es.WIDE_LEAF, mode, min_points=mp)
                    ref = voxel_ref(cloud, es.WIDE_LEAF, mode, mp)
                    assert same(out[0], ref) and len(ref) > 0, (mode, mp, out[0].shape, ref.shape)
        assert tuple(int(s) for s in np.subtract(*vs.box_of(W["src"][:-18], es.WIDE_LEAF)[::-1]) + 1) == W["span"]
    finally:
        c.close()


def test_a_span_of_2_pow_21_voxels_is_refused_and_moves_nothing():
    """include/dcreg.h: a cloud / a map that spans 2^21 or more voxels on an axis is refused - exactly 2^21 included"""
    W, B = es.wide(TOP), es.wide(TOP + 1)
    assert B["span"] == (1 << 21,) * 3
    text = "spans 2097152 voxels on axis 0 (at most 2^21 - 1 = 2097151)"
    params = api.voxel_map_params(es.WIDE_LEAF, vs.EPS, vs.MIN_POINTS)
    c = scene_context(W, 0, params)
    try:
        before_map = c.kept_target_voxels()
        before = c.linearize_voxels(W["T"], lin_params(), debug=True)
        refused(lambda: c.voxel_downsample([B["tgt"]], es.WIDE_LEAF), "cloud 0 " + text)
        refused(lambda: c.set_source_voxel(B["tgt"], es.WIDE_LEAF), "cloud 0 " + text)
        refused(lambda: c.set_target_voxel(B["tgt"], RADIUS, es.WIDE_LEAF), "cloud 0 " + text)
        # the map's own 27 points through a leaf a little smaller: one voxel more
        refused(lambda: c.keep_target_voxels(api.voxel_map_params(es.WIDE_LEAF_ONE_MORE, vs.EPS, vs.MIN_POINTS)), "the map " + text)
        refused(lambda: c.voxel_downsample([W["tgt"]], es.WIDE_LEAF_ONE_MORE), "cloud 0 " + text)
        assert c.target_voxels_kept() == 4 and c.index_info().n_source == len(W["src"])
        vs.assert_map_bitwise(c.kept_target_voxels(), before_map)
        vs.assert_map_bitwise(before_map, W["vmap"])
        after = c.linearize_voxels(W["T"], lin_params(), debug=True)
        vs.assert_dump_bitwise(after, before)
        sc.assert_sums_bitwise(after, before)
        out, info = c.voxel_downsample([W["tgt"]], es.WIDE_LEAF)            # the widest cloud that is taken still is
        assert same(out[0], voxel_ref(W["tgt"], es.WIDE_LEAF))
    finally:
        c.close()
    d = context(B["tgt"], None, keep=False)                               # the map of 2^21 voxels itself
    try:
        refused(lambda: d.keep_target_voxels(params), "the map " + text)
        assert d.target_voxels_kept() == 0
    finally:
        d.close()


# ---- 3. table sizes and a full voxel
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(es.TABLES))
def test_tables_of_two_slots_and_around_a_doubling_and_a_voxel_of_20000_points(name, mode):
    S = es.TABLES[name]()
    c = scene_context(S, mode)
    try:
        want = vr.linearize(S["vmap"], S["src"], S["T"], mode, S["src_normals"] if mode else None, vs.GICP_EPS)
        assert want["n_eff"] > 0 and (want["voxel_idx"] == -1).any()
        got = check(c, want, S["T"], "%s, mode %d" % (name, mode))
        assert np.array_equal(got["voxel_idx"], want["voxel_idx"])
        if name == "full":
            full = int(np.argmax(S["vmap"]["count"]))
            assert S["vmap"]["count"][full] == es.N_FULL and (got["voxel_idx"] == full).sum() > 250
    finally:
        c.close()


def test_the_added_and_the_missing_voxel_of_the_lattice_are_looked_up():
    P, M = es.lattice_plus(), es.lattice_minus()
    tail = slice(len(vs.lattice()["src"]), None)
    idx = {}
    for key, S in (("plus", P), ("minus", M)):
        c = scene_context(S, 0)
        try:
            idx[key] = c.linearize_voxels(S["T"], lin_params(), debug=True)["voxel_idx"][tail]
        finally:
            c.close()
    assert (idx["plus"][:8] >= 0).sum() >= 6 and (idx["plus"][8:] >= 0).sum() >= 6 and (idx["minus"] == -1).all()


# ---- 4. far from the origin
@pytest.fixture(scope="module")
def far_ctx():
    F = es.far_lot()
    c = context(F["tgt"], F["src"], F["mb"], keep=False)
    keep(c, F, what="far")
    yield c
    c.set_option("voxels_source_cov", 0)
    c.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pose", ["GT", "INIT", "MID"])
def test_the_far_lot_is_bitwise_the_reference(far_ctx, pose, mode):
    F = es.far_lot()
    far_ctx.set_option("voxels_source_cov", mode)
    want = vr.linearize(F["vmap"], F["src"], F[pose], mode, F["mb"], vs.GICP_EPS)
    assert want["n_eff"] > 250 and (want["flag"] == 0).any() and (want["flag"] == 3).any() == (mode == 1)
    check(far_ctx, want, F[pose], "far, %s, mode %d" % (pose, mode))


@pytest.mark.parametrize("mode", [0, 1])
def test_the_far_engine_is_bitwise_a_python_loop_of_its_parts_with_and_without_the_window(far_ctx, mode):
    F = es.far_lot()
    cfg = cfg_pk01(max_iterations=30, gt_matrix=np.ascontiguousarray(F["GT"]).reshape(16))
    c = far_ctx
    c.set_option("voxels_source_cov", mode)
    res, logs = c.icp_run_voxels(F["INIT"], "Ours", cfg)
    assert (res.status, res.converged) == (0, 1) and res.iterations == len(logs) >= 5
    assert logs[0].effective_points == vr.linearize(F["vmap"], F["src"], F["INIT"], mode, F["mb"], vs.GICP_EPS)["n_eff"]
    det, hand = api.METHODS["Ours"]
    T = F["INIT"].copy()
    prm = api.default_lin_params(cfg.search_radius, 1)
    for it, g in enumerate(logs):
        lin = c.linearize_voxels(T, prm)
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
    # the run through the window index: the same bits
    w = context(F["tgt"], F["src"], F["mb"], mode, keep=False, opts=OPTS_WINDOW)
    try:
        keep(w, F, what="far, window")
        res_w, logs_w = w.icp_run_voxels(F["INIT"], "Ours", cfg)
        assert untimed(res_w) == untimed(res) and len(logs_w) == len(logs)
        for it, (a, b) in enumerate(zip(logs_w, logs)):
            assert untimed(a) == untimed(b), it
    finally:
        w.close()
