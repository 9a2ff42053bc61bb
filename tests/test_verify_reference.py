"""The verification rule (include/dcreg.h, "Verification of candidate poses against the map") in its numpy form, tests/verify_ref.py: the
strict gate and the largest term on a lattice whose distances are exact, both rank rules with their ties, the score identity, the stride's
selection, non-finite rows, the derived values as bit patterns, the rmse bound of step 6, and what the stage is for - the true pose of the
lot ranks first among its neighbours under both rules.  No device."""
import math

import numpy as np
import pytest

import normal_icp_ref as nref
import normal_icp_scenes as sc
import verify_ref as vr
from test_normals_reference import lattice

UNIT = 1 << 20


def shifted(dx):
    T = np.eye(4)
    T[0, 3] = dx
    return T


def test_the_gate_is_strict_and_the_largest_term_is_two_to_the_twenty_less_one():
    m = lattice((8, 8, 8), 0.25)
    T = shifted(0.125)                                   # every point lands midway between two lattice points: d2 = 0.015625 exactly
    at = vr.score_pose(m, m, T, 0.125)
    assert (at["d2"] == np.float32(0.015625)).all()
    assert (at["count"], at["cost"], at["score"], at["fitness"], at["rmse"]) == (0, 0, 512 * UNIT, 0.0, 0.0)
    assert not at["mask"].any() and (at["nn"] == -1).all()
    up = vr.score_pose(m, m, T, np.nextafter(0.125, 1.0))
    assert (up["count"], up["cost"], up["score"], up["fitness"]) == (512, 512 * (UNIT - 1), 512 * (UNIT - 1), 1.0)
    assert up["mask"].all()
    # two lattice points tie at every query but those of the last layer: the lower index wins - the one at the smaller x, the point itself
    assert (up["nn"] == np.arange(512)).all()


def test_both_rank_rules_and_their_ties():
    S = lambda count, cost, n=10: dict(count=count, cost=cost, score=cost + (n - count) * UNIT)
    scores = [S(5, 900), S(7, 5000), S(7, 4000), S(0, 0), S(7, 4000), S(0, 0), S(9, 9 * UNIT - 9)]
    assert vr.rank(scores, 0) == [6, 2, 4, 1, 0, 3, 5]              # duplicates and the all-zero poses keep their input order
    # rule 1: many poor inliers lose to fewer good ones - 9 points at the gate score 9 * 2^20 - 9 + 2^20, 7 good ones 3 * 2^20 + 4000
    assert vr.rank(scores, 1) == [2, 4, 1, 0, 6, 3, 5]
    assert vr.rank([S(0, 0)] * 4, 0) == vr.rank([S(0, 0)] * 4, 1) == [0, 1, 2, 3]
    tie = [S(3, 5), S(10, 7 * UNIT + 5)]                             # one score, two counts: the larger count first
    assert tie[0]["score"] == tie[1]["score"] and vr.rank(tie, 1) == [1, 0] and vr.rank(tie, 0) == [1, 0]


def test_the_score_identity_the_stride_and_non_finite_rows():
    L = sc.lot()
    src = np.array(L["src"])
    src[[0, 6, 7, 100]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3]
    for s in (1, 2, 3, 64, len(src), len(src) + 1):
        sel = vr.selected(src, s)
        want = [i for i in range(0, len(src), s) if i not in (0, 6, 7, 100)]
        assert list(sel) == want
        r = vr.score_pose(L["tgt"], src, L["GT"], 0.3, s)
        assert r["n_scored"] == len(want)
        assert r["score"] == r["cost"] + (r["n_scored"] - r["count"]) * UNIT
        assert r["count"] == int(r["mask"].sum()) and not r["mask"][np.setdiff1d(np.arange(len(src)), sel)].any()
        assert ((r["nn"] >= 0) == (r["mask"] == 1)).all()
        whole = vr.score_pose(L["tgt"], src[sel], L["GT"], 0.3)      # the selected rows as a cloud of their own
        assert (whole["count"], whole["cost"]) == (r["count"], r["cost"]) and (whole["nn"] == r["nn"][sel]).all()
    empty = vr.score_pose(L["tgt"], src[[0, 6]], L["GT"], 0.3)
    assert (empty["n_scored"], empty["count"], empty["score"], empty["fitness"], empty["rmse"]) == (0, 0, 0, 0.0, 0.0)


def test_a_transformed_point_that_overflows_is_no_inlier():
    m = lattice((4, 4, 4), 0.25)
    src = np.array([[0.0, 0.0, 0.0], [3.0e38, 0.0, 0.0], [0.25, 0.25, 0.25]], np.float32)
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[1, 3] = 3.0e38                                      # y = 3e38 + 3e38 overflows the float store of the second point only
    r = vr.score_pose(m, src, shifted(0.0), 0.2)
    assert list(r["mask"]) == [1, 0, 1]
    r = vr.score_pose(m, src[[1]], T, 1.0e30)
    assert (r["n_scored"], r["count"], r["score"]) == (1, 0, UNIT)


@pytest.mark.parametrize("d", [0.1, 0.3, 0.5])
def test_fitness_and_rmse_are_their_formulas_bit_for_bit_and_rmse_keeps_its_bound(d):
    L = sc.lot()
    for T in vr.lot_poses()[:5]:
        r = vr.score_pose(L["tgt"], L["src"], T, d)
        dd = np.float64(d) * np.float64(d)
        fit = np.float64(r["count"]) / np.float64(r["n_scored"])
        assert np.float64(r["fitness"]).tobytes() == fit.tobytes()
        if r["count"] == 0:
            assert r["rmse"] == 0.0
            continue
        rm = np.sqrt(((np.float64(r["cost"]) / np.float64(UNIT)) * dd) / np.float64(r["count"]))
        assert np.float64(r["rmse"]).tobytes() == rm.tobytes()
        inl = r["mask"] == 1
        mean = math.fsum(r["d2"][inl].astype(np.float64)) / r["count"]          # the exactly rounded sum of the float d2
        assert mean - dd * 2.0 ** -20 * (1.0 + 1e-9) <= r["rmse"] ** 2 <= mean * (1.0 + 1e-12)


def test_the_true_pose_of_the_lot_ranks_first_under_both_rules():
    L = sc.lot()
    assert len(L["src"]) == 523
    Ts = vr.lot_poses()
    at3 = vr.verify(L["tgt"], L["src"], Ts, 0.3)
    # (competitors by normal_icp_scenes.offset: moved along x, turned about the pose's own position)
    assert [s["count"] for s in at3["scores"]] == [523, 523, 523, 405, 402, 0]
    assert [s["cost"] for s in at3["scores"]] == [7168006, 22830526, 179460158, 154767710, 151344017, 0]      # the 523-tie goes to the truth on cost
    assert at3["order"][0] == 0 and vr.rank(at3["scores"], 1)[0] == 0
    assert at3["order"][-1] == 5                                                   # 30 m and 90 degrees off: nothing within reach
    assert vr.rank(at3["scores"], 1) == [0, 1, 2, 4, 3, 5]                         # MSAC: 402 good inliers beat 405 poorer ones
    # at d = 0.5 the ground plane saturates the count - three poses tie at 523 - and the cost and the MSAC score decide
    at5 = vr.verify(L["tgt"], L["src"], Ts, 0.5)
    assert [s["count"] for s in at5["scores"]] == [523, 523, 523, 513, 498, 0]
    assert [s["cost"] for s in at5["scores"]] == [2580313, 8218830, 64605496, 118632790, 107336621, 0]
    assert at5["order"][0] == 0 and vr.rank(at5["scores"], 1)[0] == 0
    assert [r["pose"] for r in at5["records"]] == at5["order"] and at5["n_scored"] == 523


def test_the_transform_and_the_search_are_the_engines_own():
    """the reference is built on normal_icp_ref.transform / nearest: one pose's inliers are the second engine's radius gate"""
    L = sc.lot()
    lin = nref.linearize(L["tgt"], L["n5"], L["src"], L["MID"], 0.3)
    r = vr.score_pose(L["tgt"], L["src"], L["MID"], 0.3)
    assert r["count"] == lin["n_pt"] and (r["nn"] == lin["nn_idx"]).all()
