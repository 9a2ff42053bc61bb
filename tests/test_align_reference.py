"""The numpy reference of the alignment rule (tests/align_ref.py) against what the rule promises: the generator's pinned values, proper
rotations, the recovery of a known motion from seeded synthetic pairs, degenerate inputs and the refinement's stop.

Measured with this reference on the two recovery scenes (align_scenes.RECOVERY: 2 cm noise, d = 0.10, s = 0.9, three refinement steps):
    M = 400, 30 % inliers, H = 4 000: the mask is the true-inlier set (120 pairs), the refined pose maps every one of them within d;
    M = 2 000, 10 % inliers, H = 50 000: likewise (200 pairs).
The test asserts exactly that."""
import numpy as np
import pytest

import align_ref as ar
import align_scenes as sc


def test_the_generator_is_splitmix64_with_the_pinned_values():
    x = ar.splitmix(0, np.arange(1, 4, dtype=np.uint64))
    assert [int(v) for v in x] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # the seed is an offset of the counter's start: x(k) of seed s is mix(s + k * golden)
    assert int(ar.splitmix(0x9E3779B97F4A7C15, np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF
    u = ar.draws(0, 2, 1 << 31)
    assert [int(v) for v in u[0]] == [0xE220A839 >> 1, 0x6E789E6A >> 1, 0x06C45D18 >> 1]


@pytest.mark.parametrize("m_u", [1, 2, 3, 5, 17])
def test_the_draws_hit_every_used_pair(m_u):
    u = ar.draws(42, 400, m_u)
    assert u.min() == 0 and u.max() == m_u - 1 and sorted(np.unique(u)) == list(range(m_u))
    assert np.array_equal(u, ar.draws(42, 400, m_u))
    assert m_u == 1 or not np.array_equal(u, ar.draws(43, 400, m_u))


def orthonormal(T):
    R = np.asarray(T)[:3, :3]
    return np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.array_equal(np.asarray(T)[3], [0, 0, 0, 1])


@pytest.mark.parametrize("refine", [0, 1, 8])
def test_every_record_holds_a_proper_rotation(refine):
    a, b, ca, cb = sc.synthetic(300, 0.3, 0.02, 21)[:4]
    for s in (0.0, 0.9):
        r = ar.align(a, b, ca, cb, n_hypotheses=300, seed=1, inlier_distance=0.3, edge_similarity=s, n_best=32, refine_iterations=refine)
        assert r["info"]["n_returned"] == min(32, r["info"]["n_scored"]) > 0
        for rec in r["records"]:
            assert orthonormal(rec["T"]), rec
            assert rec["refined"] <= refine and 0 <= rec["count"] and rec["n_inliers"] <= 300


@pytest.mark.parametrize("name", sorted(sc.RECOVERY))
def test_a_known_motion_is_recovered_with_its_inlier_set(name):
    (a, b, ca, cb, R, t, inlier), kw, r = sc.recovery(name)
    d = kw["inlier_distance"]
    assert r["info"]["n_returned"] == 1 and r["info"]["n_used"] == len(ca)
    rec = r["records"][0]
    T = rec["T"]
    moved = a[ca].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    err = np.linalg.norm(moved - b[cb].astype(np.float64), axis=1)
    print(name, "true inliers", int(inlier.sum()), "found", int(r["mask"].sum()), "max error of a true inlier", err[inlier].max(),
          "pose error", np.abs(T[:3, :3] - R).max(), np.abs(T[:3, 3] - t).max(), "info", r["info"])
    assert np.all(err[inlier] <= d)
    assert np.array_equal(r["mask"] != 0, inlier)
    assert rec["n_inliers"] == inlier.sum() and rec["refined"] == 3 and rec["rmse"] <= d
    assert orthonormal(T)


def test_the_ranking_is_count_then_cost_then_h():
    a, b, ca, cb = sc.synthetic(200, 0.3, 0.02, 22)[:4]
    r = ar.align(a, b, ca, cb, n_hypotheses=500, seed=3, inlier_distance=0.3, edge_similarity=0.0, n_best=32, refine_iterations=0)
    keys = [(-x["count"], x["cost"], x["hypothesis"]) for x in r["records"]]
    assert keys == sorted(keys) and len(set(keys)) == 32
    # without refinement the pose is the hypothesis's: its inliers are the ranking key's
    assert all(x["n_inliers"] == x["count"] and x["refined"] == 0 for x in r["records"])


def degenerate_inputs():
    line = np.outer(np.arange(20, dtype=np.float32), np.array([1.0, 2.0, -1.0], np.float32))
    same = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (20, 1))
    idx = np.arange(20, dtype=np.int32)
    return {"collinear": (line, line + np.float32(1.0), idx, idx), "one point": (same, same, idx, idx)}


@pytest.mark.parametrize("name", ["collinear", "one point"])
@pytest.mark.parametrize("s", [0.0, 0.9])
def test_degenerate_pairs_return_nothing_and_count_as_degenerate(name, s):
    a, b, ca, cb = degenerate_inputs()[name]
    r = ar.align(a, b, ca, cb, n_hypotheses=200, seed=0, inlier_distance=0.5, edge_similarity=s, n_best=4)
    i = r["info"]
    assert r["records"] == [] and not r["mask"].any()
    assert (i["n_pairs"], i["n_used"], i["n_drawn"], i["n_scored"], i["n_returned"]) == (20, 20, 200, 0, 0)
    # congruent triangles pass the pre-rejection, so every hypothesis ends as degenerate
    assert i["n_degenerate"] == 200 and i["n_rejected"] == 0


def test_fewer_than_three_used_pairs_return_nothing_before_anything_is_drawn():
    a = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 1, 0]], np.float32)
    r = ar.align(a, a, np.array([0, 1, 2, 7, -1], np.int32), np.array([0, 1, 2, 3, 3], np.int32), n_hypotheses=50)
    assert r["records"] == [] and not r["mask"].any() and len(r["mask"]) == 5
    assert r["info"] == {"n_pairs": 5, "n_used": 2, "n_drawn": 0, "n_degenerate": 0, "n_rejected": 0, "n_scored": 0, "n_returned": 0}


def test_the_refinement_stops_below_three_inliers():
    # three congruent pairs far from everything else and a d too small for any other pair: without pre-rejection some hypothesis of
    # non-congruent triangles has fewer than three inliers, and its record keeps the triad's pose
    rng = np.random.default_rng(5)
    a = rng.uniform(-5, 5, (12, 3)).astype(np.float32)
    b = rng.uniform(-5, 5, (12, 3)).astype(np.float32)
    idx = np.arange(12, dtype=np.int32)
    r = ar.align(a, b, idx, idx, n_hypotheses=64, seed=2, inlier_distance=1e-3, edge_similarity=0.0, n_best=32, refine_iterations=8)
    raw = ar.align(a, b, idx, idx, n_hypotheses=64, seed=2, inlier_distance=1e-3, edge_similarity=0.0, n_best=32, refine_iterations=0)
    assert r["info"]["n_returned"] == 32
    for rec, unrefined in zip(r["records"], raw["records"]):
        assert rec["count"] < 3 and rec["refined"] == 0 and rec["n_inliers"] == rec["count"]
        assert rec["hypothesis"] == unrefined["hypothesis"] and np.array_equal(rec["T"], unrefined["T"])
    # ... and with enough inliers it runs: identical clouds, every pair an inlier of every hypothesis
    r = ar.align(a, a, idx, idx, n_hypotheses=64, seed=2, inlier_distance=1e-3, edge_similarity=0.0, n_best=4, refine_iterations=8)
    assert all(rec["refined"] == 8 and rec["n_inliers"] == 12 and np.abs(rec["T"] - np.eye(4)).max() < 1e-6 for rec in r["records"])
