"""What the consensus reference (tests/consensus_ref.py, the rule of include/dcreg.h in numpy) is worth on its own: it recovers the true
pairs and the pose at inlier shares of 1 % and 0.5 %, where the three-pair sampler's reference returns a single inlier; its weights do
not depend on the numbering of the pairs; its second-order counts are a brute-force triple loop's."""
import time

import numpy as np
import pytest

import align_ref as ar
import consensus_ref as cr
import consensus_scenes as cs


@pytest.mark.parametrize("name", sorted(cs.RECOVERY))
def test_the_reference_recovers_every_true_pair_and_the_pose(name):
    (a, b, ca, cb, R, t, inlier), kw, ref = cs.solved("recovery", name)
    assert ref["info"]["n_returned"] == 1 and np.array_equal(ref["mask"] != 0, inlier)
    rec = ref["records"][0]
    dt, ang = cs.pose_error(rec["T"], R, t)
    print(name, "true pairs", int(inlier.sum()), "record", {k: rec[k] for k in ("seed_rank", "weight", "n_members", "count", "n_inliers", "rmse")},
          "pose error", dt, "m", ang, "deg", ref["info"])
    assert dt <= 0.05 and ang <= 0.5
    assert rec["n_inliers"] == int(inlier.sum())
    # the members of the best set are true pairs, and the weights single the true pairs out
    mem = ref["members"][0]
    assert inlier[mem[mem >= 0]].all()


@pytest.mark.parametrize("name", sorted(cs.SAMPLER_FAILS))
def test_the_consensus_solves_what_the_sampler_does_not(name):
    (a, b, ca, cb, R, t, inlier), kw, ref = cs.solved("fails", name)
    for seed in cs.SAMPLER_SEEDS:
        got = ar.align(a, b, ca, cb, n_hypotheses=100000, seed=seed, inlier_distance=0.10, edge_similarity=0.9, n_best=1, refine_iterations=3)
        assert got["records"][0]["n_inliers"] < 3, (seed, got["records"][0])
    assert np.array_equal(ref["mask"] != 0, inlier)
    dt, ang = cs.pose_error(ref["records"][0]["T"], R, t)
    assert dt <= 0.05 and ang <= 0.5


def test_the_reference_is_quick_at_two_thousand_pairs():
    a, b, ca, cb = cs.scene(2000, 0.01, 45)[:4]
    t0 = time.perf_counter()
    cr.consensus(a, b, ca, cb, **cs.SETTINGS)
    assert time.perf_counter() - t0 < 5.0            # (well under a second on an idle box; the bound leaves room for a loaded one)


def test_the_weights_follow_a_renumbering_of_the_pairs():
    a, b, ca, cb = cs.scene(300, 0.05, 41)[:4]
    kw = dict(cs.SETTINGS, n_best=4)
    ref = cr.consensus(a, b, ca, cb, **kw)
    perm = np.random.default_rng(5).permutation(300)
    got = cr.consensus(a, b, ca[perm], cb[perm], **kw)
    assert ref["weight"].any()
    assert np.array_equal(got["weight"], ref["weight"][perm]) and np.array_equal(got["degree"], ref["degree"][perm])
    assert {k: v for k, v in got["info"].items()} == ref["info"]
    # the same sets, named by the pairs' points: only the order among ties may differ, and there is no tie at the top here
    pair = lambda res, cas, cbs: sorted((int(cas[m]), int(cbs[m])) for m in res["members"][0] if m >= 0)
    assert pair(got, ca[perm], cb[perm]) == pair(ref, ca, cb)
    assert np.array_equal(got["mask"], ref["mask"][perm])


def test_the_second_order_counts_are_a_triple_loops():
    a, b, ca, cb = cs.scene(20, 0.6, 42)[:4]
    m_of_u, p, q = ar.used_pairs(a, b, ca, cb)
    C = cr.compatibility(p, q, ca[m_of_u].astype(np.int64), cb[m_of_u].astype(np.int64), 0.10, 1.0)
    S = cr.second_order(C)
    assert C.any() and np.array_equal(C, C.T) and not C.diagonal().any()
    brute = np.zeros((20, 20), np.int64)
    for u in range(20):
        for v in range(20):
            if C[u, v]:
                for x in range(20):
                    brute[u, v] += int(C[u, x] and C[v, x])
    assert np.array_equal(S, brute) and S.max() >= 2
    ref = cr.consensus(a, b, ca, cb, **cs.SETTINGS)
    assert np.array_equal(ref["weight"][m_of_u], brute.sum(axis=1)) and np.array_equal(ref["degree"][m_of_u], C.sum(axis=1))


def test_fewer_than_three_used_pairs_and_an_empty_graph_return_nothing():
    a, b, ca, cb = cs.scene(50, 0.5, 44)[:4]
    got = cr.consensus(a, b, ca[:2], cb[:2], **cs.SETTINGS)
    assert got["records"] == [] and got["info"]["n_used"] == 2 and got["info"]["n_seeds"] == 0 and (got["members"] == -1).all()
    got = cr.consensus(a, np.roll(b, 7, axis=0), ca, cb, **dict(cs.SETTINGS, compat_distance=1e-9))
    i = got["info"]
    assert i["n_edges"] == 0 and i["n_seeds"] == 50 == i["n_skipped"] and i["n_scored"] == 0 and got["records"] == []
    assert not got["mask"].any() and not got["degree"].any() and not got["weight"].any()
