"""The numpy reference of the FPFH descriptors over a radius support (tests/fpfh_radius_ref.py) against what the rule promises: the k-form's
counts where the two supports coincide, PCL's float formula within a derived bound, no wrap at the largest sums, hand-computed cases, and
the cap on edge-near points for every scene the device tests use (the scenes are defined here, once, and the device tests import them)."""
import functools

import numpy as np
import pytest

import fpfh_radius_ref as rr
import fpfh_ref as fr
import normals_ref as nr
from test_fpfh_reference import EDGE_CAP, lot_cloud, uniform
from test_normals_reference import lattice, line, sphere, tilted_plane

CAP_SCENE_CAP = 40


def unit_normals(n, seed=0):
    v = np.random.default_rng(77 + seed + n).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def radius_for(n):
    """the radius at which n uniform points in uniform()'s 4 x 4 x 1.2 box have about 20 neighbours inside the box"""
    return float(min((20.0 * 19.2 / (4.18879 * n)) ** (1.0 / 3.0), 8.0))


def next_radius(radius):
    """the first double above `radius` whose square rounds to the float after (float)(radius * radius)"""
    want = np.nextafter(rr.r2_of(radius), np.float32(np.inf))
    lo, hi = np.float64(radius), np.sqrt(np.float64(want)) * (1.0 + 1e-7)          # r2_of(lo) < want <= r2_of(hi): bisect the doubles between
    assert rr.r2_of(lo) < want <= rr.r2_of(hi)
    while np.nextafter(lo, np.inf) < hi:
        mid = lo + (hi - lo) / 2
        lo, hi = (lo, mid) if rr.r2_of(mid) >= want else (mid, hi)
    return float(hi)


def clump(m, radius, seed=0, background=120):
    """m points inside a ball of diameter 0.9 radius - each has exactly the m of them as neighbours - and a sparse background far away"""
    rng = np.random.default_rng(900 + m + seed)
    d = rng.normal(size=(m, 3))
    d *= (0.45 * radius * rng.uniform(0, 1, (m, 1)) ** (1.0 / 3.0)) / np.linalg.norm(d, axis=1, keepdims=True)
    far = rng.uniform(-1, 1, (background, 3)) * [6.0 * radius, 6.0 * radius, radius] + [20.0 * radius, 0.0, 0.0]
    return np.concatenate([far[:background // 2], d, far[background // 2:]]).astype(np.float32)


def cap_cloud():
    """radius 1, max_neighbors 40: A - 40 points in a small ball, m = 40 each, the cap itself; B - 41 points along 0.8 of a line, m >= 41
    each: crowded; P at the line's far side sees itself and a few of B, crowded neighbours only.  -> (cloud, rows of A, of B, of P)"""
    rng = np.random.default_rng(40)
    A = clump(40, 1.0, background=0) + np.float32([10.0, 0.0, 0.0])
    B = np.column_stack([np.linspace(0.0, 0.8, 41), rng.uniform(-0.01, 0.01, 41), rng.uniform(-0.01, 0.01, 41)])
    P = [[1.6, 0.0, 0.0]]
    cloud = np.concatenate([A, B, P]).astype(np.float32)
    return cloud, np.arange(0, 40), np.arange(40, 81), np.array([81])


def near_pairs_cloud(radius):
    """uniform(300) with two planted pairs: rows 300, 301 closer than radius / 256 (the clamped weight), rows 302, 303 just outside it"""
    base = uniform(300)
    a, b = base[10] + np.float32([0.0, 0.0, 1.5]), base[20] + np.float32([0.0, 0.0, -1.5])
    return np.concatenate([base, [a, a + np.float32([radius / 300.0, 0, 0]), b, b + np.float32([radius / 200.0, 0, 0])]]).astype(np.float32)


def duplicates_cloud(copies):
    cloud = uniform(600)
    at = np.random.default_rng(copies).choice(600, copies, replace=False)
    cloud[at] = cloud[at[0]]
    return cloud, at


def nan_rows(cloud, seed=1):
    """NaN rows and single non-finite coordinates planted"""
    rng = np.random.default_rng(seed)
    out = np.insert(cloud, rng.choice(len(cloud), 9, replace=False), np.float32(np.nan), axis=0)
    out[len(out) // 2, 1] = np.inf
    out[0, 2] = np.nan
    return out


def nan_normals(cloud, k=12):
    """the k-rule normals of the cloud (tests/normals_ref.py) with seven non-finite components planted"""
    normals = nr.normals_reference(cloud, k=k)["normals"]
    hit = np.random.default_rng(5).choice(len(cloud), 7, replace=False)
    normals[hit, np.arange(7) % 3] = [np.nan, np.inf, -np.inf, np.nan, np.nan, np.inf, np.nan]
    return normals


SCENE_RADIUS = {"plane": 0.45, "sphere": 0.4, "lattice": 0.6, "lot": 1.5}
SCENE_CLOUD = {"plane": tilted_plane, "sphere": sphere, "lattice": lattice, "lot": lot_cloud}


@functools.lru_cache(maxsize=None)
def scene(name):
    """a scene of the device tests by name -> (cloud, normals, radius, max_neighbors); the arrays are shared: do not write to them"""
    kind, _, arg = name.partition(":")
    if kind == "uniform":
        n = int(arg)
        return uniform(n), unit_normals(n), radius_for(n), rr.MAX_CAP
    if kind == "clump":
        cloud = clump(int(arg), 1.0)
        return cloud, unit_normals(len(cloud)), 1.0, rr.MAX_CAP
    if kind == "edge":
        return lattice((4, 4, 4)), unit_normals(64), (0.5 if arg == "at" else next_radius(0.5)), rr.MAX_CAP
    if kind == "cap":
        cloud = cap_cloud()[0]
        return cloud, unit_normals(len(cloud)), 1.0, CAP_SCENE_CAP
    if kind == "duplicates":
        cloud = duplicates_cloud(int(arg))[0]
        return cloud, unit_normals(600), radius_for(600), rr.MAX_CAP
    if kind == "near":
        cloud = near_pairs_cloud(0.5)
        return cloud, unit_normals(len(cloud)), 0.5, rr.MAX_CAP
    if kind == "line":
        cloud = line()
        s = np.float32(1.0 / np.sqrt(6.0))
        return cloud, np.tile(np.array([s, 2 * s, -s], np.float32), (len(cloud), 1)), 1.0, rr.MAX_CAP
    cloud = nan_rows(SCENE_CLOUD[kind]())
    return cloud, nan_normals(cloud), SCENE_RADIUS[kind], rr.MAX_CAP


SIZES = [1, 2, 3, 63, 64, 65, 257, 4099]
SUPPORTS = [31, 32, 33, 255, 256, 257]
GPU_SCENES = (["uniform:%d" % n for n in SIZES] + ["clump:%d" % m for m in SUPPORTS] + ["edge:at", "edge:above", "cap", "duplicates:3",
              "duplicates:40", "near", "line"] + sorted(SCENE_CLOUD))


@functools.lru_cache(maxsize=None)
def reference(name):
    cloud, normals, radius, cap = scene(name)
    return rr.fpfh_radius_reference(cloud, normals, radius, cap)


# ---- the scenes are what their names say, and the reference stays inside the edge-near cap on each
@pytest.mark.parametrize("name", GPU_SCENES)
def test_the_cap_on_edge_near_points_holds_for_every_scene_of_the_device_tests(name):
    r = reference(name)
    assert r["excluded"].sum() <= EDGE_CAP * max(r["n_used"], 1), (name, int(r["excluded"].sum()), r["n_used"])
    assert r["n_out"] + r["n_empty"] == r["n_used"] and r["n_crowded"] <= r["n_empty"]
    f = r["fpfh"]
    ok = ~np.isnan(f[:, 0])
    assert ok.sum() == r["n_out"] and not np.isnan(f[ok]).any() and np.isnan(f[~ok]).all()
    if ok.any():
        # 11 floats of at most 100, each within half an ulp (2^-18 at 64 .. 128) of its double
        assert np.abs(f[ok].astype(np.float64).reshape(-1, 3, 11).sum(axis=2) - 100.0).max() <= 11 * 2.0 ** -18


def test_the_scenes_have_the_supports_their_names_promise():
    for n in SIZES[4:]:
        r = reference("uniform:%d" % n)
        assert 10 <= r["m_sum"] / r["n_used"] <= 30, (n, r["m_sum"] / r["n_used"])
    for m in SUPPORTS:
        assert reference("clump:%d" % m)["m_max"] == m
    at, above = reference("edge:at"), reference("edge:above")
    assert rr.r2_of(scene("edge:at")[2]) == np.float32(0.25) and rr.r2_of(scene("edge:above")[2]) == np.nextafter(np.float32(0.25), np.float32(1))
    # an inner point of the lattice: 6 + 12 + 8 neighbours closer than two steps and itself; four points along an axis leave it one
    # neighbour at exactly two steps on each
    assert at["m_max"] == 27 and above["m_max"] == 27 + 3 and np.all(above["m"] == at["m"] + 3)
    cloud, A, B, P = cap_cloud()
    r = reference("cap")
    assert np.all(r["m"][A] == 40) and np.all(r["m"][B] == 41) and r["crowded"][B].all() and not r["crowded"][A].any() and r["n_crowded"] == 41
    assert 2 <= r["m"][P[0]] <= 20 and r["has_spfh"][P[0]] and np.isnan(r["fpfh"][P[0]]).all() and np.isnan(r["fpfh"][B]).all()
    assert not np.isnan(r["fpfh"][A]).any() and r["n_empty"] == 42 and r["m_max"] == 41 and not r["counts"][B].any()
    for copies in (3, 40):
        at_rows = duplicates_cloud(copies)[1]
        assert np.all(reference("duplicates:%d" % copies)["m"][at_rows] >= copies)
    r = reference("near")
    assert list(r["clamped"][300:]) == [1, 1, 0, 0] and r["clamped"][:300].sum() == 0 and np.all(r["m"][300:] == 2)
    r = reference("line")
    assert r["n_used"] == 40 and r["n_empty"] == 40 and r["m_max"] > 2 and not r["has_spfh"].any()
    for name in SCENE_CLOUD:
        r = reference(name)
        assert r["n_in"] - r["n_used"] >= 16 and r["n_out"] > 0.9 * r["n_used"] and r["m_max"] > 32, (name, r["n_out"], r["n_used"], r["m_max"])


# ---- against the k-form
def test_where_no_point_has_more_than_32_neighbours_the_counts_are_the_k_forms():
    """with m <= 32 everywhere the k-form at k = 32 and search_radius = radius keeps every point inside the bound: the same neighbours, so
    the same counts, m and SPFH flags (the sums differ: floats there, integers here)"""
    cloud, normals = uniform(1000), unit_normals(1000)
    radius = 0.35
    r = rr.fpfh_radius_reference(cloud, normals, radius)
    k = fr.fpfh_reference(cloud, normals, k=32, search_radius=radius)
    assert 8 < r["m_max"] <= 32 and r["n_crowded"] == 0
    assert np.array_equal(r["m"], k["m"]) and np.array_equal(r["counts"], k["counts"]) and np.array_equal(r["has_spfh"], k["has_spfh"])
    assert np.array_equal(r["edge_near"], k["edge_near"]) and np.array_equal(r["excluded"], k["excluded"])
    assert r["m_sum"] == k["m"].sum()


# ---- against PCL's formula in floating point
def pcl_formula(cloud, normals, radius, counts, m):
    """sum_j (1 / d2_ij) * 100 c_b(j) / (m_j - 1) over the same neighbour sets in double, each block normalised to 100"""
    R2 = rr.r2_of(radius)
    s = 100.0 * counts.astype(np.float64) / (m - 1).astype(np.float64)[:, None]
    F = np.zeros((len(cloud), 33))
    for i, j, d2 in rr._pairs(np.ascontiguousarray(cloud[:, :3]), R2):
        far = d2 > 0
        rr._add_rows(F, i[far], s[j[far]] / d2[far].astype(np.float64)[:, None])
    S = np.repeat(np.stack([F[:, 11 * t:11 * t + 11].sum(axis=1) for t in range(3)], axis=1), 11, axis=1)
    return 100.0 * F / S


def test_the_integer_rule_stays_close_to_the_float_formula():
    """The bound, on the 0 .. 100 scale, for a point with m - 1 = M contributing neighbours, none of them clamped, every neighbour with all
    its pairs counted (so that each block of c sums to m_j - 1 and each block of q to nearly 65536).
    Write a_j = R2 / d2_ij >= 1 for the float weight (PCL's 1 / d2 up to the factor R2, which the normalisation removes) and p_b(j) =
    c_b(j) / (m_j - 1) for the float SPFH share, sum_b p_b(j) = 1 per block.  The integer rule uses
        w_j = floor(16384 a_j)       = 16384 a_j (1 - e_j),      0 <= e_j < 1 / (16384 a_j) <= 2^-14            (step 6)
        q_b(j) = floor(65536 p_b(j)) = 65536 p_b(j) - f_bj,      0 <= f_bj < 1                                  (step 5)
    so F_b = 2^30 (sum_j a_j p_b(j) - E_b) with the shortfall 0 <= E_b < sum_j a_j (2^-14 p_b(j) + 2^-16) (the product of the two errors
    is dropped: it only makes the shortfall smaller).  With A = sum_j a_j, G_b = sum_j a_j p_b(j) (the float formula's unnormalised value,
    sum_b G_b = A per block): E_b < 2^-14 G_b + 2^-16 A, and the block's shortfall E = sum_b E_b < 2^-14 A + 11 * 2^-16 A.
    The outputs are 100 G_b / A (float) and 100 (G_b - E_b) / (A - E) (integer).  Their difference is
        100 | (G_b - E_b) A - G_b (A - E) | / (A (A - E)) = 100 | G_b E - E_b A | / (A (A - E)) <= 100 max(G_b E, E_b A) / (A (A - E)),
    and with G_b <= A both terms are below 100 (2^-14 + 11 * 2^-16) A^2 / (A (A - E)) = 100 * 15 * 2^-16 / (1 - E / A).  E / A < 15 * 2^-16,
    so the bound is 100 * 15 * 2^-16 / (1 - 15 * 2^-16) = 0.02289; the final double -> float rounding of either side adds at most half an
    ulp of 100 (2^-18 = 3.8e-6), and the float formula's own double rounding is below 1e-12.  Bound: 0.0229 + 2 * 2^-18 < 0.023."""
    bound = 100.0 * 15 * 2.0 ** -16 / (1.0 - 15 * 2.0 ** -16) + 2 * 2.0 ** -18
    assert bound < 0.023
    cloud = uniform(1500)
    normals = nr.normals_reference(cloud, k=10)["normals"]          # (smooth normals: no pair of the scene has v = 0)
    radius = 0.55
    r = rr.fpfh_radius_reference(cloud, normals, radius)
    # the two conditions of the bound: no clamped pair, and every neighbour counts all its pairs (each block of c sums to m - 1)
    assert r["clamped"].sum() == 0 and r["n_crowded"] == 0 and r["n_used"] == 1500 and r["m"].min() >= 2
    assert np.all(r["counts"].reshape(-1, 3, 11).sum(axis=2) == (r["m"] - 1)[:, None])
    assert r["n_out"] == 1500 and r["m_sum"] / 1500 > 40
    want = pcl_formula(cloud, normals, radius, r["counts"], r["m"])
    diff = np.abs(r["fpfh"].astype(np.float64) - want).max()
    print("integer rule against the float formula: max |difference| = %.3g of 100 (bound %.3g), mean m %.1f" % (diff, bound, r["m_sum"] / 1500))
    assert diff <= bound


# ---- the largest sums
def test_the_largest_sums_do_not_wrap():
    """m = 65535 neighbours, every weight clamped to 2^30, every q of a bin at its largest, 65536: F_b = 65535 * 2^46 < 2^62, and a block's
    sum is the same number, because a block of q sums to at most 65536"""
    m = rr.MAX_CAP
    w = rr.weights(np.float32(1.0), np.full(4, np.float32(2.0 ** -40)))
    assert list(w) == [rr.W_CAP] * 4 and w.dtype == np.uint64
    q = rr.quantise(np.array([[m - 1] + [0] * 10] * 3).reshape(1, 33), np.array([m]))
    assert q.dtype == np.uint64 and list(q[0, ::11]) == [65536] * 3 and q.sum() == 3 * 65536
    F = np.zeros((1, 33), np.uint64)
    for _ in range(16):                                   # 65535 equal terms, as 15 * 4096 + 4095 of them
        F += (np.uint64(4096) if _ < 15 else np.uint64(4095)) * (w[0] * q)
    exact = m * 2 ** 30 * 65536
    assert exact == 65535 * 2 ** 46 < 2 ** 62 and [int(v) for v in F[0, ::11]] == [exact] * 3
    out, full = rr.normalise(F)
    assert full.all() and np.array_equal(out[0, ::11], np.float32([100.0] * 3)) and np.count_nonzero(out) == 3
    # a block whose eleven bins share the same neighbours: the block's sum is still the bound, not eleven times it
    q11 = rr.quantise(np.array([[(m - 1) // 11] * 11] * 3).reshape(1, 33), np.array([m]))
    assert int(q11[0, :11].sum()) <= 65536 and int(q11[0, :11].sum()) * m * 2 ** 30 < 2 ** 62


# ---- hand-computed cases
Z = [0.0, 0.0, 1.0]


def one_hot(*bins):
    f = np.zeros(33, np.float32)
    f[list(bins)] = 100.0
    return f


def test_two_points():
    """the k-form's case: every feature in its middle bin; m = 2, so q = 65536 there, w = floor(4 / 1 * 16384) for radius 2"""
    r = rr.fpfh_radius_reference(np.array([[0, 0, 0], [1, 0, 0]], np.float32), np.array([Z, Z], np.float32), radius=2.0)
    assert r["n_out"] == 2 and r["n_empty"] == 0 and list(r["m"]) == [2, 2] and r["m_sum"] == 4 and r["m_max"] == 2
    for i in (0, 1):
        assert list(np.flatnonzero(r["counts"][i])) == [5, 16, 27] and np.array_equal(r["fpfh"][i], one_hot(5, 16, 27))
    alone = rr.fpfh_radius_reference(np.array([[0, 0, 0], [1, 0, 0]], np.float32), np.array([Z, Z], np.float32), radius=1.0)
    assert list(alone["m"]) == [1, 1] and alone["n_empty"] == 2             # (strict: the point AT the radius is no neighbour)


def test_the_weight_and_the_quantisation():
    assert list(rr.weights(np.float32(1.0), np.float32([1.0, 0.5, 2.0 ** -16, 2.0 ** -17, 3.0]))) == [16384, 32768, 2 ** 30, 2 ** 30, 5461]
    assert list(rr.quantise(np.array([[1, 2, 3]]), np.array([4]))[0]) == [21845, 43690, 65536]
    assert next_radius(0.5) > 0.5 and rr.r2_of(np.nextafter(next_radius(0.5), 0.0)) == np.float32(0.25)


def test_parameters_outside_the_rule_are_refused():
    cloud, normals = uniform(10), unit_normals(10)
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius=1e-30), dict(radius=1.8e19),
               dict(max_neighbors=1), dict(max_neighbors=65536)):
        with pytest.raises(AssertionError):
            rr.fpfh_radius_reference(cloud, normals, **kw)
