"""The numpy reference of the FPFH descriptors and of the feature matching (tests/fpfh_ref.py) against what the rule promises: block sums,
invariance under a rigid motion, hand-computed pairs, and the cap on edge-near points for every scene the device tests use.

Measured with this reference on the 4 000-point parking lot (scene_parkinglot(4000, 1500, extent 12, frame_range 5)), normals from
tests/normals_ref.py at k = 16, the copy moved by the inverse of PK01_GT (points and normals, both stored as float32), k = 16:
    own index for 100.000 % of the 4 000 rows (at k = 8: 97.925 % - coarse histograms repeat on the ground plane);
    per-row maximum difference of the descriptors: 6.5e-5 at the 99th percentile (2.3e-4 at most);
    edge-near points: 0 of 4 000 at k = 8 and at k = 16, on both copies.
The test asserts the share minus half a percentage point and ten times the difference."""
import numpy as np
import pytest

import fpfh_ref as fr
import helpers as h
import normals_ref as nr
from test_normals_reference import lattice, line, sphere, tilted_plane

OWN_INDEX_SHARE = 1.0 - 0.005
ROW_DIFF_P99 = 10 * 6.5e-5
EDGE_CAP = 0.01


def lot_cloud():
    return h.scene_parkinglot(n_map=4000, n_frame=1500, extent=12.0, frame_range=5.0)[0]


def normals_of(cloud, k=16):
    return nr.normals_reference(cloud, k=k)["normals"]


def moved_copy(cloud, normals):
    T = np.linalg.inv(h.pose6d_matrix(**h.PK01_GT))
    R, t = T[:3, :3], T[:3, 3]
    return (cloud.astype(np.float64) @ R.T + t).astype(np.float32), (normals.astype(np.float64) @ R.T).astype(np.float32)


def uniform(n, seed=0):
    return (np.random.default_rng(2000 + seed + n).uniform(-2, 2, (n, 3)) * [1.0, 1.0, 0.3]).astype(np.float32)


# the clouds of tests/test_gpu_fpfh.py and tests/test_gpu_feature_match.py, by name: (cloud, normals, k)
def gpu_scenes():
    out = {}
    for name, make in (("plane", tilted_plane), ("sphere", sphere), ("lattice", lattice), ("line", line), ("lot", lot_cloud)):
        cloud = make()
        out[name] = (cloud, normals_of(cloud, 8 if name == "line" else 16), 16)
    for n in (63, 64, 65, 257, 1000, 4099):
        cloud = uniform(n)
        out["uniform%d" % n] = (cloud, normals_of(cloud, 5), 16)
    lot = out["lot"]
    out["lot_moved"] = moved_copy(lot[0], lot[1]) + (16,)
    return out


@pytest.fixture(scope="module")
def lot():
    cloud = lot_cloud()
    normals = normals_of(cloud)
    mc, mn = moved_copy(cloud, normals)
    return dict(cloud=cloud, normals=normals, a=fr.fpfh_reference(cloud, normals, k=16), b=fr.fpfh_reference(mc, mn, k=16), moved=(mc, mn))


def test_every_block_sums_to_100(lot):
    for r in (lot["a"], lot["b"]):
        f = r["fpfh"]
        ok = ~np.isnan(f[:, 0])
        assert ok.sum() == r["n_out"] == 4000 and r["n_empty"] == 0
        assert not np.isnan(f[ok]).any() and np.all(np.isnan(f[~ok]))
        sums = f[ok].astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
        # 11 floats of at most 100, each within half an ulp (2^-18 at 64 .. 128) of its double
        assert np.abs(sums - 100.0).max() <= 11 * 2.0 ** -18


def test_a_rigid_motion_of_points_and_normals_leaves_the_descriptors(lot):
    a, b = lot["a"]["fpfh"], lot["b"]["fpfh"]
    diff = np.abs(a - b).max(axis=1)
    print("row difference: p99 %.3g, max %.3g" % (np.percentile(diff, 99), diff.max()))
    assert np.percentile(diff, 99) <= ROW_DIFF_P99


def test_the_moved_copy_matches_its_own_rows(lot):
    m = fr.match_reference(lot["b"]["fpfh"], lot["a"]["fpfh"])
    share = np.mean(m["idx"] == np.arange(4000))
    print("own index: %.5f, mutual %d" % (share, m["n_mutual"]))
    assert m["n_a_valid"] == m["n_b_valid"] == 4000
    assert share >= OWN_INDEX_SHARE
    assert np.all(m["d"] <= m["d2"]) and np.all(m["idx"] != m["idx2"])


@pytest.mark.parametrize("k", [8, 16])
def test_the_lot_has_no_edge_near_point(lot, k):
    for cloud, normals in ((lot["cloud"], lot["normals"]), lot["moved"]):
        r = fr.fpfh_reference(cloud, normals, k=k)
        assert r["edge_near"].sum() == 0 and r["excluded"].sum() == 0


def test_the_cap_on_edge_near_points_holds_for_every_scene_of_the_device_tests():
    for name, (cloud, normals, k) in gpu_scenes().items():
        for kk in sorted({5, k}):
            r = fr.fpfh_reference(cloud, normals, k=kk)
            assert r["excluded"].sum() <= EDGE_CAP * max(r["n_used"], 1), (name, kk, int(r["excluded"].sum()), r["n_used"])


# ---- hand-computed cases
Z = [0.0, 0.0, 1.0]


def one_hot(*bins):
    f = np.zeros(33, np.float32)
    f[list(bins)] = 100.0
    return f


def test_two_points():
    """d = (1, 0, 0), both normals z: a1 = a2 = 0, phi = 0; v = d x n = (0, -1, 0), w = n x v = (1, 0, 0), alpha = 0, theta = atan2(0, 1) = 0:
    every feature in its middle bin (5.5 -> 5); m = 2, so each point's SPFH is 100 there, and the other point's SPFH is the whole FPFH"""
    r = fr.fpfh_reference(np.array([[0, 0, 0], [1, 0, 0]], np.float32), np.array([Z, Z], np.float32), k=3)
    assert r["n_used"] == 2 and r["n_out"] == 2 and r["n_empty"] == 0 and list(r["m"]) == [2, 2]
    for i in (0, 1):
        assert list(np.flatnonzero(r["counts"][i])) == [5, 16, 27] and r["counts"][i].sum() == 3
        assert np.array_equal(r["fpfh"][i], one_hot(5, 16, 27))
    assert list(r["neighbours"][0]) == [0, 1, -1] and list(r["neighbours"][1]) == [1, 0, -1]


def test_a_normal_parallel_to_d_counts_no_pair():
    """d = (0, 0, 1) = n: v = d x n = 0, the pair is skipped; no SPFH anywhere, so both points are EMPTY"""
    r = fr.fpfh_reference(np.array([[0, 0, 0], [0, 0, 1]], np.float32), np.array([Z, Z], np.float32), k=3)
    assert r["n_used"] == 2 and r["n_empty"] == 2 and r["n_out"] == 0
    assert not r["counts"].any() and not r["has_spfh"].any() and np.isnan(r["fpfh"]).all()


def test_duplicates_are_neighbours_but_no_pairs():
    """points 0 and 1 coincide: each counts the pair with point 2 only (m = 3: s = 100 / 2 = 50 per count); point 2 counts both (2 * 50 =
    100).  The FPFH of 0 skips 1 (d2 == 0) and takes 2's SPFH; the FPFH of 2 adds 50 + 50"""
    r = fr.fpfh_reference(np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32), np.array([Z, Z, Z], np.float32), k=3)
    assert list(r["m"]) == [3, 3, 3] and list(r["neighbours"][1]) == [0, 1, 2] and list(r["neighbours"][2]) == [2, 0, 1]
    assert [int(r["counts"][i][5]) for i in range(3)] == [1, 1, 2] and r["counts"].sum() == 12
    for i in range(3):
        assert np.array_equal(r["fpfh"][i], one_hot(5, 16, 27))


@pytest.mark.parametrize("ny,bin_", [(-1.0, 21), (1.0, 11)])
def test_alpha_is_clamped_at_plus_and_minus_one(ny, bin_):
    """n_0 = z, n_1 = (0, -+1, 0), d = (1, 0, 0): seen from 0, v = (0, -1, 0) and alpha = v . n_1 = +-1 exactly; 11 * ((1 + 1) * 0.5) = 11 is
    clamped into bin 10, 11 * 0 = 0 is bin 0.  Seen from 1 the same alpha.  n_0 . n_1 = 0 and w . n_2 = 0: theta = atan2(0, 0) = 0"""
    r = fr.fpfh_reference(np.array([[0, 0, 0], [1, 0, 0]], np.float32), np.array([Z, [0.0, ny, 0.0]], np.float32), k=3)
    for i in (0, 1):
        assert list(np.flatnonzero(r["counts"][i])) == [5, bin_, 27]
        assert np.array_equal(r["fpfh"][i], one_hot(5, bin_, 27))


def test_points_without_a_finite_normal_are_neither_queries_nor_candidates():
    cloud = uniform(200)
    normals = normals_of(cloud, 5)
    normals[[3, 50], 1] = np.nan
    cloud[7, 2] = np.inf
    r = fr.fpfh_reference(cloud, normals, k=8)
    assert r["n_in"] == 200 and r["n_used"] == 197 and r["n_out"] + r["n_empty"] == 197
    assert np.isnan(r["fpfh"][[3, 7, 50]]).all() and not np.isin(r["neighbours"], [3, 7, 50]).any()
    keep = np.ones(200, bool)
    keep[[3, 7, 50]] = False
    alone = fr.fpfh_reference(cloud[keep], normals[keep], k=8)
    assert np.array_equal(alone["fpfh"].view(np.uint32), r["fpfh"][keep].view(np.uint32))


def test_a_bounded_search_keeps_the_neighbours_it_has():
    cloud = np.concatenate([uniform(300), [[30.0, 0.0, 0.0]], [[40.0, 0.0, 0.0], [40.05, 0.0, 0.0]]]).astype(np.float32)
    normals = np.tile(np.array(Z, np.float32), (len(cloud), 1))
    normals[:300] = normals_of(cloud[:300], 5)
    r = fr.fpfh_reference(cloud, normals, k=16, search_radius=0.6)
    assert r["m"][300] == 1 and r["m"][301] == 2 and (r["m"][:300] == 16).any() and ((r["m"][:300] > 1) & (r["m"][:300] < 16)).any()
    assert np.isnan(r["fpfh"][300]).all() and not r["has_spfh"][300]


# ---- the matcher
def test_the_matcher_ranks_by_distance_then_index_and_skips_invalid_rows():
    rng = np.random.default_rng(3)
    b = rng.uniform(0, 100, (40, 33)).astype(np.float32)
    b[7] = b[2]
    b[11, 4] = np.nan
    b[30, 0] = 8.0
    a = b[[2, 7, 11, 30]].copy()
    a[3, 0] += 1.0
    m = fr.match_reference(a, b)
    assert list(m["idx"]) == [2, 2, -1, 30] and list(m["idx2"][:2]) == [7, 7] and m["idx2"][2] == -1
    assert m["d"][0] == m["d2"][0] == 0.0 and np.isnan(m["d"][2]) and np.isnan(m["d2"][2]) and m["d"][3] == 1.0
    assert list(m["mutual"]) == [1, 0, 0, 1] and m["n_mutual"] == 2       # (b[2]'s best row of a is 0, not 1: the tie goes to the lower index)
    assert (m["n_a_valid"], m["n_b_valid"]) == (3, 39)
    one = fr.match_reference(a, b[11:13])
    assert list(one["idx"]) == [1, 1, -1, 1] and list(one["idx2"]) == [-1] * 4 and np.all(np.isinf(one["d2"][[0, 1, 3]]))
    none = fr.match_reference(a, b[11:12])
    assert list(none["idx"]) == [-1] * 4 and np.all(np.isinf(none["d"][[0, 1, 3]])) and np.isnan(none["d"][2]) and none["n_mutual"] == 0
