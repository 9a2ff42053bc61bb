"""The numpy reference of the robust kernels (tests/robust_ref.py, include/dcreg.h "robust kernels") on its own: with no kernel it is the
plain references bit for bit, factor() at its exact points, k*k*r against the analytic rho'(r) of each kernel, and what the kernels are
for - the contaminated frame of tests/robust_scenes.py ends more than a degree off without a kernel and within half a degree with
Geman-McClure, while the clean frame does not move.  No device."""
import numpy as np
import pytest

import gicp_ref as gref
import gicp_scenes as gs
import normal_icp_ref as ref
import normal_icp_scenes as sc
import robust_ref as rr
import robust_scenes as rs

RADIUS = sc.RADIUS


def test_no_kernel_is_the_plain_references_bit_for_bit():
    L = gs.lot()
    for T in (L["INIT"], L["MID"]):
        for c in (0.02, 0.1):
            a = rr.linearize_normals(L["tgt"], L["nb"], L["src"], T, RADIUS, 0, c, use_weight_derivative=1)
            b = ref.linearize(L["tgt"], L["nb"], L["src"], T, RADIUS, use_weight_derivative=1)
            sc.assert_dump_bitwise(a, b)
            sc.assert_sums_bitwise(a, b)
            a = rr.linearize_gicp(L["tgt"], L["nb"], L["src"], L["mb"], T, RADIUS, 0, c, gs.EPS)
            b = gref.linearize(L["tgt"], L["nb"], L["src"], L["mb"], T, RADIUS, gs.EPS)
            gs.assert_dump_bitwise(a, b)
            sc.assert_sums_bitwise(a, b)


def test_the_values_of_factor():
    for kind in (0, 1, 2, 3):
        assert rr.factor(kind, 0.0) == 1.0
    assert rr.factor(1, 1.0) == 1.0
    assert rr.factor(1, 4.0) == np.sqrt(np.float64(0.5))
    assert rr.factor(2, 3.0) == 0.5
    assert rr.factor(3, 1.0) == 0.5
    u2 = np.concatenate([[0.0], np.logspace(-300, 24, 2000), [1e24]])
    for kind in (1, 2, 3):
        k = rr.factor(kind, u2)
        assert np.isfinite(k).all() and (k > 0.0).all() and (k <= 1.0).all()
        assert (np.diff(k) <= 0.0).all()                               # never a larger weight further out


def test_k_squared_times_r_is_the_derivative_of_the_kernel():
    """the IRLS identity: k = sqrt(rho'(r) / r).  Huber rho' = r (|r| <= c), c sign(r) beyond; Cauchy rho' = r / (1 + (r/c)^2);
    Geman-McClure rho' = r / (1 + (r/c)^2)^2 - to 4 ulp"""
    rng = np.random.default_rng(21)
    r = rng.normal(0.0, 0.3, 4000) * 10.0 ** rng.uniform(-3, 1, 4000)
    c = 10.0 ** rng.uniform(-2, 0.5, 4000)
    u2 = (r * r) / (c * c)
    want = {1: np.where(np.abs(r) <= c, r, c * np.sign(r)), 2: r / (1.0 + u2), 3: r / ((1.0 + u2) * (1.0 + u2))}
    for kind in (1, 2, 3):
        k = rr.factor(kind, u2)
        got = k * k * r
        assert (np.abs(got - want[kind]) <= 4.0 * np.spacing(np.abs(want[kind]))).all(), kind
    assert (np.abs(r) <= c).any() and (np.abs(r) > c).any()


@pytest.mark.parametrize("engine", ["normals", "gicp"])
def test_the_contaminated_frame_needs_the_kernel_and_the_clean_frame_does_not_mind_it(engine):
    L = gs.lot()
    S = rs.contaminated()
    assert len(S["moved"]) == rs.N_MOVED and len(S["src"]) == 523
    runs = {(engine, f, k): rs.reference_run(engine, f, k) for f in ("dirty", "clean") for k in (0, rs.GM)}
    t0, r0 = rs.rot_trans_error(runs[engine, "dirty", 0][0], L["GT"])
    t3, r3 = rs.rot_trans_error(runs[engine, "dirty", rs.GM][0], L["GT"])
    print("%s, contaminated: no kernel %.4f m %.3f deg (%d iterations), Geman-McClure %.4f m %.3f deg (%d iterations)"
          % (engine, t0, r0, len(runs[engine, "dirty", 0][2]), t3, r3, len(runs[engine, "dirty", rs.GM][2])))
    assert r0 > 1.0 and r3 < 0.5
    dt, dr = rs.rot_trans_error(runs[engine, "clean", rs.GM][0], runs[engine, "clean", 0][0])
    print("%s, clean: kernel on against off %.4f m %.3f deg" % (engine, dt, dr))
    assert dt < 0.005 and dr < 0.1
