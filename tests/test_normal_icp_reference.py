"""The numpy reference of the 1-NN point-to-plane linearisation (tests/normal_icp_ref.py: include/dcreg.h's rule, literally) checked against
what it must satisfy by construction - the nearest neighbour against a double-precision brute force, invariances that hold bitwise, the
planted gates - and the reference ENGINE (that linearisation + the host solver seam, no device) on the parking lot.  The device and the host
replay are compared bitwise with this reference (tests/test_gpu_normal_icp.py, tests/test_emul_nlin.py)."""
import numpy as np
import pytest

import normal_icp_ref as ref
import normal_icp_scenes as sc
from dcreg_amd import api


def cfg_pk01(**kw):
    """the thresholds of configs/icp_pk01.yaml"""
    L = sc.lot()
    base = dict(search_radius=0.5, max_iterations=10, CONVERGENCE_THRESH_TRANS=1e-3, CONVERGENCE_THRESH_ROT=1e-5, gt_matrix=L["GT"].reshape(-1))
    base.update(kw)
    return api.default_config(**base)


@pytest.fixture(scope="module")
def engine_none():
    L = sc.lot()
    return ref.icp(L["tgt"], L["n5"], L["src"], L["INIT"], cfg_pk01(), "NONE")


@pytest.mark.parametrize("pose", ["INIT", "MID"])
def test_the_nearest_neighbour_is_the_brute_force_minimum_to_float_rounding(pose):
    """A float d2 is three squares and two adds of float differences: relative error below 2^-22 per candidate, so the double-precision
    distance of the reference's pick lies within a factor 1 + 2^-21 of the true minimum."""
    L = sc.lot()
    q = ref.transform(L[pose][:3, :3], L[pose][:3, 3], L["src"])
    j, d2 = ref.nearest(L["tgt"], q)
    dd = ((q.astype(np.float64)[:, None, :] - L["tgt"].astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    assert np.all(dd[np.arange(len(q)), j] <= dd.min(axis=1) * (1.0 + 2.0 ** -21))
    # ... and the float d2 it reports is the one the rule computes for that pair
    assert sc.same_bits(d2, ((q[:, 0] - L["tgt"][j, 0]) ** 2 + (q[:, 1] - L["tgt"][j, 1]) ** 2) + (q[:, 2] - L["tgt"][j, 2]) ** 2)


def test_a_common_shift_exact_in_float_changes_no_flag_and_no_residual():
    """R = I: q = p + t exactly when the sums are exact in float, so map and source shifted by the same vector keep every difference"""
    rng = np.random.default_rng(21)
    grid = np.float32(2.0 ** -10)                                   # coordinates on a 2^-10 grid below 8: the shifted sums stay exact
    m = (np.round(rng.uniform(-4, 4, (600, 3)) / grid) * grid).astype(np.float32)
    s = (np.round(rng.uniform(-4, 4, (300, 3)) / grid) * grid).astype(np.float32)
    normals = sc.unit_normals(len(m), 22)
    shift = np.array([64.0, -32.0, 16.0], np.float32)
    a = ref.linearize(m, normals, s, np.eye(4), 0.5, use_weight_derivative=1)
    b = ref.linearize(m + shift, normals, s + shift, np.eye(4), 0.5, use_weight_derivative=1)
    assert 0 < a["n_eff"] < len(s) and (a["flag"] == 0).any()
    for k in ("flag", "nn_idx", "nn_d2", "r", "s"):
        assert sc.same_bits(a[k], b[k]), k


@pytest.mark.parametrize("wd", [0, 1])
def test_flipping_every_normal_keeps_the_sums_and_negates_the_residuals(wd):
    L = sc.lot()
    a = ref.linearize(L["tgt"], L["nb"], L["src"], L["INIT"], 0.5, use_weight_derivative=wd)
    b = ref.linearize(L["tgt"], -L["nb"], L["src"], L["INIT"], 0.5, use_weight_derivative=wd)
    assert a["n_eff"] == 369 and a["n_pt"] == 523 and (a["flag"] == 2).sum() == 154
    sc.assert_sums_bitwise(a, b)
    assert np.array_equal(a["flag"], b["flag"]) and sc.same_bits(b["s"], a["s"])
    reached, eff = (a["flag"] == 1) | (a["flag"] == 4), a["flag"] == 1          # (elsewhere the dump holds +0.0, which has no negative here)
    assert sc.same_bits(b["r"][reached], -a["r"][reached]) and not b["r"][~reached].any()
    assert sc.same_bits(b["row"][eff][:, :6], -a["row"][eff][:, :6]) and sc.same_bits(b["row"][eff][:, 6:], -a["row"][eff][:, 6:])


@pytest.mark.parametrize("slope", sc.GATE_SLOPES)
def test_the_planted_case_hits_every_flag(slope):
    G = sc.gate_case()
    out = ref.linearize(G["tgt"], G["normals"], G["src"], G["T"], G["radius"], weight_slope=slope, use_weight_derivative=1)
    assert list(out["flag"]) == sc.GATE_FLAGS
    assert out["nearest_d2"][0] == np.float32(0.25) and out["nn_idx"][0] == -1 and np.isinf(out["nn_d2"][0])      # d2 == R*R stays out
    assert out["nn_idx"][1] == 0 and out["nn_d2"][1] < np.float32(0.25) and out["r"][1] == 0.0 and out["s"][1] == 1.0
    assert list(out["nn_idx"]) == [-1, 0, 1, 2, 3, 3, 4, -1]
    assert np.isnan(out["normal"][3, 0]) and out["normal"][3, 2] == 1.0 and not out["row"][3].any()
    r4 = float(np.float32(0.475))
    assert out["r"][4] == r4 and out["s"][4] == max(1.0 - slope * r4, 0.0) and (out["s"][4] == 0.0) == (slope == 3.0) and not out["row"][4].any()
    assert out["r"][5] < 0.0 and out["s"][5] <= 0.1
    # point 6: r = 0.25, s = 1 - slope r, w = s + r ds = 1 - 2 slope r; m = n (identity pose); b = -(s r)
    s6, w6 = 1.0 - slope * 0.25, 1.0 - 2.0 * slope * 0.25
    assert out["s"][6] == s6 and np.array_equal(out["row"][6], [w6 * 0.0, w6 * (0.25 * 0.0 - 40.0 * 1.0), w6 * 0.0, 0.0, 0.0, w6, -(s6 * 0.25), 0.25])
    assert out["n_eff"] == 3 and out["n_pt"] == 6


def test_the_reference_engine_converges_on_the_lot(engine_none):
    """from PK01_INIT (0.229 m, 2.53 deg) under the thresholds of icp_pk01.yaml within 10 iterations, both errors at least 5x down (the numpy
    prototype of the rule reached 0.0074 m and 0.153 deg in 5 iterations: 31x and 17x)"""
    L = sc.lot()
    T, converged, recs = engine_none
    t0, r0 = api.pose_error(L["GT"], L["INIT"])
    t1, r1 = api.pose_error(L["GT"], T)
    print("start %.4f m %.3f deg -> %.4f m %.3f deg in %d iterations" % (t0, r0, t1, r1, len(recs)))
    assert abs(t0 - 0.229) < 1e-3 and abs(r0 - 2.53) < 1e-2
    assert converged and len(recs) <= 10
    assert t1 * 5.0 <= t0 and r1 * 5.0 <= r0
    assert all(r["n_pt"] == 523 and r["n_eff"] == 523 for r in recs)


def test_no_point_of_the_run_sits_on_a_gate(engine_none):
    """what lets the device test compare counts exactly across two summation orders: at every iteration every point is more than 1e-6 from
    the radius gate (in d2) and from the weight gate (in s)"""
    for it, r in enumerate(engine_none[2]):
        d_gate, w_gate = ref.gate_margins(r["lin"], 0.5)
        print("iteration %d: radius gate margin %.3g, weight gate margin %.3g" % (it, d_gate, w_gate))
        assert d_gate > 1e-6 and w_gate > 1e-6
