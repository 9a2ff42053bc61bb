"""The numpy reference of the outlier filters (tests/outliers_ref.py) against an independent computation: scipy's cKDTree in double, fsum for
the tree sum, the oracle's kd-tree for the neighbours, and a planted scene whose outliers are known."""
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

import outliers_ref as orf
from oracle import pyoracle as po


def planted_scene():
    """2 000 points of a 10 m x 10 m plane with 1 cm noise and 20 points 1.5 - 4 m above it, shuffled: (cloud, planted mask)"""
    rng = np.random.default_rng(7)
    plane = np.column_stack([rng.uniform(0, 10, 2000), rng.uniform(0, 10, 2000), rng.normal(0, 0.01, 2000)])
    high = np.column_stack([rng.uniform(0, 10, 20), rng.uniform(0, 10, 20), rng.uniform(1.5, 4.0, 20)])
    pts = np.concatenate([plane, high]).astype(np.float32)
    planted = np.arange(len(pts)) >= 2000
    o = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[o]), planted[o]


def scipy_statistical(pts, k, std_mul, search_radius=0.0):
    """the same rule in double with scipy's tree: (scores, used-in-statistics, threshold)"""
    p = pts.astype(np.float64)
    d, _ = cKDTree(p).query(p, k + 1)
    d = d[:, 1:]
    ok = np.ones(len(p), bool) if search_radius == 0.0 else d[:, -1] < search_radius
    m = d.mean(axis=1)
    mean, sd = m[ok].mean(), m[ok].std(ddof=1)
    return m, ok, mean + std_mul * sd


@pytest.mark.parametrize("seed,n,k,std_mul", [(1, 3000, 8, 1.0), (2, 2500, 5, 2.0), (3, 4000, 16, 0.5), (4, 1500, 1, 1.5)])
def test_the_reference_agrees_with_scipy_in_double(seed, n, k, std_mul):
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-5, 5, (n, 3)) * [1.0, 1.0, 0.2]).astype(np.float32)
    ref = orf.outlier_reference(pts, "statistical", k=k, std_mul=std_mul)
    m, ok, thr = scipy_statistical(pts, k, std_mul)
    assert np.allclose(ref["scores"], m, rtol=1e-5, atol=0) and math.isclose(ref["threshold"], thr, rel_tol=1e-5)
    close = np.abs(m - thr) <= 1e-6 * thr
    assert close.mean() <= 0.01                      # (otherwise the comparison below would hide a failure)
    assert np.array_equal(ref["mask"][~close], (m <= thr)[~close])
    assert 0 < ref["n_out"] < n and ref["n_finite"] == n and ref["n_sparse"] == 0


def test_the_bounded_reference_agrees_with_scipy_in_double():
    pts, planted = planted_scene()
    ref = orf.outlier_reference(pts, "statistical", k=8, std_mul=2.0, search_radius=1.0)
    m, ok, thr = scipy_statistical(pts, 8, 2.0, 1.0)
    assert np.array_equal(np.isnan(ref["scores"]), ~ok) and ref["n_sparse"] == int((~ok).sum()) == 20
    assert np.array_equal(~ok, planted)
    assert math.isclose(ref["threshold"], thr, rel_tol=1e-5)
    close = ok & (np.abs(m - thr) <= 1e-6 * thr)
    assert close.mean() <= 0.01
    assert np.array_equal(ref["mask"][~close], (ok & (m <= thr))[~close])


def test_the_radius_reference_agrees_with_scipy_in_double():
    rng = np.random.default_rng(11)
    pts = rng.uniform(-3, 3, (2500, 3)).astype(np.float32)
    radius = 0.4
    tree = cKDTree(pts.astype(np.float64))
    d, _ = tree.query(pts.astype(np.float64), 40)
    cnt = (d[:, 1:] < radius).sum(axis=1)
    edge = (np.abs(d[:, 1:] - radius) <= 1e-6 * radius).any(axis=1)
    assert edge.mean() <= 0.01
    for m in (1, 3, 8):
        ref = orf.outlier_reference(pts, "radius", radius=radius, min_neighbors=m)
        assert np.array_equal(ref["mask"][~edge], (cnt >= m)[~edge])
        assert np.array_equal(ref["scores"][~edge], np.minimum(cnt, m)[~edge].astype(np.float32))
        assert 0 < ref["n_out"] < len(pts)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 1000, 4097, 100_003])
def test_the_tree_sum_equals_fsum(n):
    a = np.random.default_rng(n).uniform(0, 1, n)
    exact = math.fsum(a)
    assert abs(orf.tree_sum(a) - exact) <= n * 2.0 ** -53 * exact
    assert orf.tree_sum(a[:0]) == 0.0


def test_the_tree_sum_is_the_pairwise_tree():
    a = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 0.0, 1.0])
    assert orf.tree_sum(a) == ((1.0 + 2.0 ** -53) + (2.0 ** -53 + 0.0)) + ((1.0 + 0.0) + (0.0 + 0.0))
    b = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]
    assert orf.tree_sum(b) == 1.0 + 2.0 ** -52 and sum(b) == 1.0          # (left to right every addend is lost)


def test_the_planted_points_are_what_the_statistical_filter_drops():
    pts, planted = planted_scene()
    ref = orf.outlier_reference(pts, "statistical", k=8, std_mul=2.0)
    assert np.array_equal(~ref["mask"], planted) and ref["n_out"] == 2000
    assert np.nanmax(ref["scores"][~planted]) < ref["threshold"] < np.nanmin(ref["scores"][planted])
    print("threshold %.3f, largest plane score %.3f, smallest planted score %.3f"
          % (ref["threshold"], np.nanmax(ref["scores"][~planted]), np.nanmin(ref["scores"][planted])))
    assert np.array_equal(ref["kept"].view(np.uint32), pts[~planted].view(np.uint32))


def test_the_oracle_tree_gives_the_reference_the_same_neighbours():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-4, 4, (3000, 3)).astype(np.float32)
    pts[100:140] = pts[7]                            # 40 copies of one point: more than k + 1
    a = orf.outlier_reference(pts, "statistical", k=8, std_mul=1.0)
    b = orf.outlier_reference(pts, "statistical", k=8, std_mul=1.0, neighbours=lambda p, kk: po.KdTree(p).knn(p, kk))
    assert np.array_equal(a["scores"].view(np.uint32), b["scores"].view(np.uint32)) and np.array_equal(a["mask"], b["mask"])
    assert (a["mean"], a["stddev"], a["threshold"]) == (b["mean"], b["stddev"], b["threshold"])
    assert np.all(a["scores"][100:140] == 0.0) and a["scores"][7] == 0.0


def test_self_exclusion_is_by_index():
    """with more than k duplicates a point is not among its own k + 1 nearest: the last entry goes, not the first"""
    pts = np.zeros((12, 3), np.float32)
    pts[10:] = [[1, 0, 0], [0, 2, 0]]
    idx, d2 = orf.brute_neighbours(pts, 4)
    assert not (idx[9] == 9).any() and (idx[0] == 0).any()
    o = orf.others(idx, d2, 3)
    assert np.array_equal(o[9], [0, 0, 0]) and np.array_equal(o[10], [1, 1, 1]) and np.array_equal(o[11], [4, 4, 4])


def test_clouds_without_statistics_and_unused_points():
    pts = np.random.default_rng(2).uniform(0, 1, (6, 3)).astype(np.float32)
    pts[2, 1] = np.nan
    pts[4, 0] = np.inf
    ref = orf.outlier_reference(pts, "statistical", k=4, std_mul=1.0)          # 4 used points, k = 4: no statistics
    assert ref["n_finite"] == 4 and ref["n_out"] == 4 and np.isnan(ref["scores"]).all() and np.isnan(ref["threshold"])
    assert np.array_equal(ref["mask"], [1, 1, 0, 1, 0, 1])
    ref = orf.outlier_reference(pts, "statistical", k=3, std_mul=5.0)
    assert ref["n_out"] == 4 and np.isnan(ref["scores"][[2, 4]]).all() and not np.isnan(ref["scores"][[0, 1, 3, 5]]).any()
    ref = orf.outlier_reference(pts, "statistical", k=4, std_mul=1.0, search_radius=10.0)      # bounded: fewer than k others is sparse
    assert ref["n_sparse"] == 4 and ref["n_out"] == 0 and np.isnan(ref["mean"])
    ref = orf.outlier_reference(np.zeros((0, 3), np.float32))
    assert ref["n_in"] == 0 and ref["n_out"] == 0 and ref["kept"].shape == (0, 3)
