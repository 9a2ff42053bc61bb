"""The fourth engine's loop on the device (dcreg_icp_run_voxels) on the 40 000-point variant of the parking lot: its log is bitwise a
Python loop of linearize_voxels + the solver seam + boxplus, within 1e-7 per iteration of the numpy reference engine (tests/voxels_ref.py),
and it ends within twice the reference engine's own final error; a frame far outside the map aborts with status 1."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as h
import normal_icp_scenes as sc
import normals_ref as nr
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
# The numpy reference engine's final error on this scene from PK01_INIT (0.23 m / 2.5 deg off), run on the CPU with 30 iterations allowed:
# (method, mode) -> (metres, degrees).  The device run must end within twice that; the margin covers nothing but the choice of scene.
REFERENCE_FINAL = {("NONE", 0): (0.00765, 0.1138), ("Ours", 0): (0.00765, 0.1138), ("Ours", 1): (0.01494, 0.2510)}


def values(o):
    """a ctypes record as nested tuples of its fields' bit patterns (padding bytes are nobody's)"""
    if isinstance(o, C.Structure):
        return tuple(values(getattr(o, f[0])) for f in o._fields_)
    if isinstance(o, C.Array):
        return tuple(values(x) for x in o)
    return np.float64(o).tobytes() if isinstance(o, float) else o


@functools.lru_cache(maxsize=None)
def dense_lot():
    """the lot's generator with ten times the map points (40 000) and a 1 500-point frame, its reference voxel map and source normals"""
    tgt, src = h.scene_parkinglot(n_map=40000, n_frame=1500, extent=12.0, frame_range=5.0)
    assert len(src) == 1500
    return dict(tgt=sc.frozen(tgt), src=sc.frozen(src), GT=vs.lot()["GT"], INIT=vs.lot()["INIT"],
                vmap=vr.voxel_map(tgt, vs.LEAF, vs.EPS, vs.MIN_POINTS), m5=sc.frozen(nr.normals_reference(src, k=5)["normals"]))


@pytest.fixture(scope="module")
def dense_ctx():
    D = dense_lot()
    c = api.Context(0)
    c.set_target(D["tgt"], RADIUS)
    c.set_source(D["src"])
    c.set_source_normals(np.ascontiguousarray(D["m5"], np.float32))
    info = c.keep_target_voxels(api.voxel_map_params(vs.LEAF, vs.EPS, vs.MIN_POINTS))
    assert info["n_kept"] == D["vmap"]["n_kept"] == 693
    yield c
    c.close()


@pytest.mark.parametrize("method,mode", [("NONE", 0), ("Ours", 0), ("Ours", 1)])
def test_the_engine_follows_the_reference_engine_and_a_python_loop_of_its_parts(dense_ctx, method, mode):
    D = dense_lot()
    c = dense_ctx
    cfg = cfg_pk01(max_iterations=30)
    c.set_option("voxels_source_cov", mode)
    try:
        T_ref, conv_ref, recs = vr.icp(D["vmap"], D["src"], D["INIT"], cfg, method, mode, D["m5"], vs.GICP_EPS)
        res, logs = c.icp_run_voxels(D["INIT"], method, cfg)
        assert (res.status, res.converged, res.iterations) == (0, int(conv_ref), len(recs)) and len(logs) == len(recs)
        for it, (g, r) in enumerate(zip(logs, recs)):
            assert (g.effective_points, g.corr_pt_count) == (r["n_eff"], r["n_pt"]), it
            assert list(g.analysis.degenerate_mask[:]) == r["mask"], it
            err = np.max(np.abs(np.array(g.transform_matrix[:]).reshape(4, 4) - r["T"]))
            print("%s mode %d iteration %d: pose difference %.3g" % (method, mode, it, err))
            assert err < 1e-7, (it, err)
            assert g.fitness == r["n_pt"] / 1500.0
        t_ref, r_ref = vr.pose_error(T_ref, D["GT"])
        t_err, r_err = vr.pose_error(np.array(logs[-1].transform_matrix[:]).reshape(4, 4), D["GT"])
        print("%s mode %d: %d iterations -> %.4f m %.3f deg (reference engine %.4f m %.3f deg)" % (method, mode, len(logs), t_err, r_err, t_ref, r_ref))
        cap_t, cap_r = REFERENCE_FINAL[(method, mode)]
        assert abs(t_ref - cap_t) < 1e-4 and abs(r_ref - cap_r) < 1e-3           # the figures above are this reference engine's
        assert res.converged == 1 and t_err < 2.0 * cap_t and r_err < 2.0 * cap_r
        # the same loop in Python: linearize_voxels + the solver seam + boxplus, bitwise the engine's log
        det, hand = api.METHODS[method]
        T = D["INIT"].copy()
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
    finally:
        c.set_option("voxels_source_cov", 0)


def test_a_frame_far_outside_the_map_aborts_with_status_1(dense_ctx):
    D = dense_lot()
    far = sc.offset(D["INIT"], 500.0, 0.0, 0.0)
    res, logs = dense_ctx.icp_run_voxels(far, "Ours", cfg_pk01())
    assert (res.status, res.converged, res.iterations, len(logs)) == (1, 0, 1, 0)
    assert np.array_equal(np.array(res.t[:]), far[:3, 3]) and np.array_equal(np.array(res.R[:]), far[:3, :3].reshape(9))


def test_the_engine_without_kept_voxels_is_refused():
    D = dense_lot()
    c = api.Context(0)
    try:
        c.set_target(D["tgt"], RADIUS)
        c.set_source(D["src"])
        with pytest.raises(api.DcregError) as e:
            c.icp_run_voxels(D["INIT"], "Ours", cfg_pk01())
        assert "(%d)" % api.E_STATE in str(e.value) and "no kept voxels" in str(e.value)
    finally:
        c.close()
