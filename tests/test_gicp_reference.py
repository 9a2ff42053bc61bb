"""The numpy reference of the plane-to-plane linearisation (tests/gicp_ref.py: include/dcreg.h's rule, literally) checked against what it
must satisfy by construction - the 6 x 6 system against the textbook formula with numpy.linalg.inv, invariances that hold bitwise, the
isotropic limit, the planted flags - and the reference ENGINE (that linearisation + the host solver seam, no device) on the parking lot.
The device and the host replay are compared bitwise with this reference (tests/test_gpu_gicp.py, tests/test_emul_glin.py)."""
import numpy as np
import pytest

import gicp_ref as gref
import gicp_scenes as gs
import helpers as h
import normal_icp_ref as ref
import normal_icp_scenes as sc
from dcreg_amd import api
from test_normal_icp_reference import cfg_pk01


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def direct_system(L, T, eps, jacobian_only=False):
    """H = sum J^T S^-1 J and g = -sum J^T S^-1 e over the points inside the radius, S = C_map + R C_src R^T inverted by numpy, J the
    derivative of R Exp(dtheta) (p + dt) + t in the right perturbation (dcreg_boxplus).  jacobian_only: S = I (the point-to-point Gram)"""
    R, t = T[:3, :3], T[:3, 3]
    q = ref.transform(R, t, L["src"])
    j, d2 = ref.nearest(L["tgt"], q)
    H, g = np.zeros((6, 6)), np.zeros(6)
    for i in np.flatnonzero(d2.astype(np.float64) < gs.RADIUS ** 2):
        n, u = L["n5"][j[i]].astype(np.float64), R @ L["m5"][i].astype(np.float64)
        S = 2.0 * np.eye(3) - (1.0 - eps) * (np.outer(n, n) + np.outer(u, u))
        Si = np.eye(3) if jacobian_only else np.linalg.inv(S)
        p = L["src"][i].astype(np.float64)
        J = np.hstack([-R @ skew(p), R])
        e = q[i].astype(np.float64) - L["tgt"][j[i]].astype(np.float64)
        H += J.T @ Si @ J
        g -= J.T @ Si @ e
    return H, g


@pytest.fixture(scope="module")
def engine_none():
    L = gs.lot()
    return gref.icp(L["tgt"], L["n5"], L["src"], L["m5"], L["INIT"], cfg_pk01(), "NONE", eps=gs.EPS)


@pytest.mark.parametrize("pose", ["INIT", "MID"])
def test_the_system_is_the_sum_of_jt_sigma_inverse_j(pose):
    L = gs.lot()
    out = gref.linearize(L["tgt"], L["n5"], L["src"], L["m5"], L[pose], gs.RADIUS, gs.EPS)
    assert out["n_eff"] == out["n_pt"] == 523
    H, g = direct_system(L, L[pose], gs.EPS)
    eh, eg = h.rel_err(api.unpack_hessian(out["H_upper"]), H), h.rel_err(out["g"], g)
    print("%s: H %.3g, g %.3g, cond(H) %.3g" % (pose, eh, eg, np.linalg.cond(H)))
    assert eh < 1e-9 and eg < 1e-9
    # both squared sums are the Mahalanobis distances
    assert out["sum_r2"] == out["sum_b2"] > 0.0


def test_flipping_a_normal_changes_no_bit_of_any_row():
    L = gs.lot()
    a = gref.linearize(L["tgt"], L["nb"], L["src"], L["mb"], L["INIT"], gs.RADIUS, gs.EPS)
    assert (a["flag"] == 1).any() and (a["flag"] == 2).any() and (a["flag"] == 3).any()
    rng = np.random.default_rng(7)
    some_n, some_m = rng.random(len(L["tgt"])) < 0.5, rng.random(len(L["src"])) < 0.5
    for nmap, nsrc in ((-L["nb"], L["mb"]), (L["nb"], -L["mb"]), (-L["nb"], -L["mb"]),
                       (np.where(some_n[:, None], -L["nb"], L["nb"]), np.where(some_m[:, None], -L["mb"], L["mb"]))):
        b = gref.linearize(L["tgt"], nmap, L["src"], nsrc, L["INIT"], gs.RADIUS, gs.EPS)
        for k in ("flag", "nn_idx", "nn_d2", "w", "r", "row"):
            assert sc.same_bits(a[k], b[k]), k
        sc.assert_sums_bitwise(a, b)


def test_epsilon_one_is_half_the_point_to_point_system():
    """c = 0: S = 2 I whatever the normals, W = I / sqrt(2)"""
    L = gs.lot()
    out = gref.linearize(L["tgt"], L["n5"], L["src"], L["m5"], L["MID"], gs.RADIUS, 1.0)
    H, g = direct_system(L, L["MID"], 1.0, jacobian_only=True)
    assert h.rel_err(api.unpack_hessian(out["H_upper"]), 0.5 * H) < 1e-12 and h.rel_err(out["g"], 0.5 * g) < 1e-12
    eff = out["flag"] == 1
    assert eff.all() and np.all(out["w"][eff] == np.eye(3) * (1.0 / np.sqrt(2.0)))


def test_the_planted_case_hits_every_flag():
    P = gs.plant_case()
    out = gref.linearize(P["tgt"], P["normals"], P["src"], P["src_normals"], P["T"], P["radius"], gs.EPS)
    assert list(out["flag"]) == gs.PLANT_FLAGS
    assert out["nearest_d2"][0] == np.float32(0.25) and out["nn_idx"][0] == -1 and np.isinf(out["nn_d2"][0])      # d2 == R*R stays out
    assert list(out["nn_idx"]) == [-1, 0, 1, 2, 3, 4, -1, 2]
    assert np.isnan(out["normal_map"][3, 0]) and np.isinf(out["normal_src"][2, 1]) and np.isnan(out["normal_src"][7, 0])
    for i in (0, 2, 3, 4, 6, 7):
        assert not out["w"][i].any() and not out["r"][i].any() and not out["row"][i].any(), i
    # point 1: both normals (0, 0, 1), e = (-x, 0, 0): S = diag(2, 2, 2 eps), the residual lies in the plane
    x = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert np.array_equal(out["r"][1], [(1.0 / np.sqrt(2.0)) * x + 0.0 + 0.0, 0.0, 0.0])
    assert out["n_eff"] == 2 and out["n_pt"] == 6


def test_the_reference_engine_converges_on_the_lot(engine_none):
    """from PK01_INIT (0.229 m, 2.53 deg) with k = 5 unbounded normals on both sides at eps = 1e-3, plain Gauss-Newton ("NONE"): within
    10 iterations to below 0.012 m and 0.15 deg (the numpy prototype of the rule: 5 iterations, 0.0071 m, 0.088 deg)"""
    L = gs.lot()
    T, converged, recs = engine_none
    t1, r1 = api.pose_error(L["GT"], T)
    print("-> %.4f m %.3f deg in %d iterations" % (t1, r1, len(recs)))
    assert converged and len(recs) <= 10
    assert t1 < 0.012 and r1 < 0.15
    assert all(r["n_pt"] == 523 and r["n_eff"] == 523 for r in recs)


def test_no_point_of_the_run_sits_on_the_gate(engine_none):
    """what lets the device test compare counts exactly across two summation orders"""
    for it, r in enumerate(engine_none[2]):
        assert gref.gate_margin(r["lin"], 0.5) > 1e-6, it
