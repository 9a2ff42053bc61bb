"""The numpy reference of the surface normals (tests/normals_ref.py, the rule of include/dcreg.h applied literally) checked against what
does not rest on its own arithmetic: an exact plane, numpy.linalg.eigh of the same covariances, the orientation on a sphere, and the
degenerate clouds.  The device is compared bitwise against this reference in tests/test_gpu_normals.py."""
import numpy as np
import pytest

import normals_ref as nr


def exact_plane(m=14, seed=3):
    """points ON the plane z = -2 over a jittered x/y lattice: e_z, the z row of the covariance and its eigenvalue are exactly 0"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(m) * 0.25, np.arange(m) * 0.25, indexing="ij")
    xy = np.stack([gx, gy], -1).reshape(-1, 2) + rng.uniform(-0.08, 0.08, (m * m, 2)) - 1.5
    return np.column_stack([xy, np.full(m * m, -2.0)]).astype(np.float32)


def tilted_plane(n=600, seed=5):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-2, 2, (n, 2))
    e1, e2, nn = np.array([1.0, 0.2, 0.1]), np.array([-0.1, 1.0, 0.4]), np.array([0.3, -0.5, 1.0])
    return (uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0, 0.01, (n, 1)) * nn + [0.5, -1.0, 4.0]).astype(np.float32)


SPHERE_CENTRE = np.array([3.0, -2.0, 1.5])


def sphere(n=700, seed=7, noise=0.005):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (SPHERE_CENTRE + d * (1.0 + rng.normal(0, noise, (n, 1)))).astype(np.float32)


def lattice(shape=(12, 12, 4), step=0.25):
    """a regular lattice whose spacing is exact in float: every distance ties, the index decides"""
    g = [np.arange(m, dtype=np.float32) * np.float32(step) for m in shape]
    return np.ascontiguousarray(np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3))


def line(n=40):
    t = np.arange(n, dtype=np.float64) * 0.125
    return np.column_stack([1.0 + t, -2.0 + 2.0 * t, 0.5 - t]).astype(np.float32)


SCENES = {"plane": tilted_plane, "sphere": sphere, "lattice": lattice}


def angle(a, b):
    c = np.abs(np.sum(a * b, axis=1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.arccos(np.minimum(c, 1.0))


def full(C):
    return np.stack([np.stack([C[:, 0], C[:, 1], C[:, 2]], -1), np.stack([C[:, 1], C[:, 3], C[:, 4]], -1),
                     np.stack([C[:, 2], C[:, 4], C[:, 5]], -1)], -2)


def test_an_exact_plane_gives_the_exact_normal():
    cloud = exact_plane()
    for k in (5, 10):
        r = nr.normals_reference(cloud, k=k)
        assert r["n_out"] == len(cloud) and r["n_sparse"] == 0
        assert np.all(r["normals"] == np.array([0.0, 0.0, 1.0], np.float32))
        assert np.all(r["curvature"] == 0.0) and np.all(r["eigenvalues"][:, 0] == 0.0) and np.all(r["eigenvalues"][:, 1] > 0.0)
        # from below the plane the same normals point down
        r = nr.normals_reference(cloud, k=k, viewpoint=(0.0, 0.0, -5.0))
        assert np.all(r["normals"] == np.array([0.0, 0.0, -1.0], np.float32))


@pytest.mark.parametrize("k", [5, 10])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_against_eigh_of_the_same_covariances(name, k):
    cloud = SCENES[name]()
    r = nr.normals_reference(cloud, k=k, viewpoint=None)
    assert r["n_out"] == len(cloud)
    assert np.all(r["off"] == 0.0)                               # six sweeps leave every off-diagonal exactly 0
    w, v = np.linalg.eigh(full(r["cov"]))
    lam = nr.ascending(r["lam"])
    assert np.all(lam[:, 0] <= lam[:, 1]) and np.all(lam[:, 1] <= lam[:, 2])
    assert np.all(np.abs(lam - w) <= 1e-12 * w[:, 2:3])
    assert np.array_equal(r["eigenvalues"], lam.astype(np.float32))
    gap = (w[:, 1] - w[:, 0]) / w[:, 2] > 1e-3
    assert name == "lattice" or gap.sum() > len(cloud) // 2          # (the lattice's neighbourhoods are symmetric: two equal eigenvalues)
    assert np.all(angle(r["normal64"][gap], v[gap, :, 0]) <= 1e-6)
    assert np.all(np.abs(np.linalg.norm(r["normal64"], axis=1) - 1.0) < 1e-14)
    cv = np.abs(r["lam"].min(axis=1)) / r["lam"].sum(axis=1)
    assert np.allclose(r["curvature"], cv, rtol=1e-6, atol=0)


def test_normals_on_a_sphere_point_to_the_viewpoint():
    cloud = sphere()
    r = nr.normals_reference(cloud, k=10, viewpoint=SPHERE_CENTRE)
    inward = SPHERE_CENTRE - cloud.astype(np.float64)
    assert np.all(np.sum(r["normals"] * inward, axis=1) > 0.9)
    free = nr.normals_reference(cloud, k=10, viewpoint=None)
    flipped = np.any(free["normals"] != r["normals"], axis=1)
    assert 0 < flipped.sum() < len(cloud)                        # the solver's sign is arbitrary, the orientation is not
    assert np.array_equal(np.abs(free["normals"]), np.abs(r["normals"])) and np.array_equal(free["curvature"], r["curvature"])


def test_a_dot_product_of_exactly_zero_keeps_the_sign():
    cloud = exact_plane()
    free = nr.normals_reference(cloud, k=5, viewpoint=None)
    assert np.all(free["normals"] == np.array([0.0, 0.0, 1.0], np.float32))
    # a viewpoint IN the plane: every dot product is (..)*0 + (..)*0 + 0*1 = 0
    r = nr.normals_reference(cloud, k=5, viewpoint=(7.0, -3.0, -2.0))
    assert np.array_equal(r["normals"], free["normals"])


def test_a_straight_line_takes_the_lowest_index():
    cloud = line()
    r = nr.normals_reference(cloud, k=5)
    assert r["n_out"] == len(cloud) and not np.isnan(r["normals"]).any() and not np.isnan(r["curvature"]).any()
    d = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    assert np.all(np.abs(r["normals"].astype(np.float64) @ d) < 1e-6)                 # perpendicular to the line
    assert np.all(np.abs(r["eigenvalues"][:, :2]) <= 1e-14 * r["eigenvalues"][:, 2:]) and np.all(r["curvature"] <= 1e-14)
    i0 = nr.smallest(r["lam"])
    tie = r["lam"][np.arange(len(cloud)), i0][:, None] == r["lam"]
    assert np.all(i0 == tie.argmax(axis=1))


def test_nan_rows_get_nan_and_the_rest_is_the_clean_clouds():
    cloud = tilted_plane(300)
    dirty = np.insert(cloud, [0, 17, 17, 299], np.float32(np.nan), axis=0)
    dirty[40, 1] = np.inf
    used = np.isfinite(dirty).all(axis=1)
    r, clean = nr.normals_reference(dirty, k=6), nr.normals_reference(dirty[used], k=6)
    assert (r["n_in"], r["n_finite"], r["n_sparse"], r["n_out"]) == (304, 299, 0, 299)
    assert np.isnan(r["normals"][~used]).all() and np.isnan(r["curvature"][~used]).all() and np.isnan(r["eigenvalues"][~used]).all()
    for key in ("normals", "curvature", "eigenvalues"):
        assert np.array_equal(r[key][used], clean[key])


def test_fewer_than_k_points_are_all_sparse():
    cloud = tilted_plane(7)
    r = nr.normals_reference(cloud, k=8)
    assert (r["n_finite"], r["n_sparse"], r["n_out"]) == (7, 7, 0) and np.isnan(r["normals"]).all()
    r = nr.normals_reference(cloud, k=7)
    assert (r["n_sparse"], r["n_out"]) == (0, 7) and not np.isnan(r["normals"]).any()
    r = nr.normals_reference(np.full((3, 3), np.nan, np.float32), k=3)
    assert (r["n_in"], r["n_finite"], r["n_sparse"], r["n_out"]) == (3, 0, 0, 0)
    r = nr.normals_reference(np.zeros((0, 3), np.float32), k=3)
    assert (r["n_in"], r["n_out"]) == (0, 0) and r["normals"].shape == (0, 3)


def far_cluster(k=8):
    """a plane and, 30 m away, a cluster of k - 1 points: sparse under a bound, served from across the gap without one"""
    rng = np.random.default_rng(9)
    far = (rng.uniform(-0.1, 0.1, (k - 1, 3)) + [30.0, 0.0, 0.0]).astype(np.float32)
    return np.concatenate([tilted_plane(400), far]), np.arange(400, 400 + k - 1)


def test_points_beyond_the_search_radius_are_sparse():
    cloud, far = far_cluster(8)
    r = nr.normals_reference(cloud, k=8, search_radius=1.0)
    assert r["n_sparse"] == 7 and np.array_equal(np.flatnonzero(np.isnan(r["curvature"])), far)
    free = nr.normals_reference(cloud, k=8)
    assert free["n_sparse"] == 0 and np.array_equal(free["normals"][:400], r["normals"][:400])
    # the comparison is strict: on a lattice with the bound AT the spacing only the point itself counts
    lat = lattice((4, 4, 4))
    assert nr.normals_reference(lat, k=3, search_radius=0.25)["n_out"] == 0
    assert nr.normals_reference(lat, k=3, search_radius=float(np.nextafter(np.float32(0.25), np.float32(1))))["n_out"] == 64


@pytest.mark.parametrize("copies", [3, 40])
def test_duplicates_fewer_and_more_than_k(copies):
    k = 8
    cloud = tilted_plane(300)
    at = np.random.default_rng(copies).choice(300, copies, replace=False)
    cloud[at] = cloud[at[0]]
    r = nr.normals_reference(cloud, k=k)
    assert r["n_out"] == 300
    if copies > k:
        # every neighbour is a copy: the covariance is exactly zero, the solver leaves V = I, the lowest index wins, no NaN
        assert np.all(r["eigenvalues"][at] == 0.0) and np.all(r["curvature"][at] == 0.0)
        assert np.all(np.abs(r["normals"][at]) == np.array([1.0, 0.0, 0.0], np.float32))
        assert np.all(r["cov"][at] == 0.0)
    else:
        assert np.all(r["eigenvalues"][at, 2] > 0.0) and not np.isnan(r["normals"][at]).any()
        assert len(np.unique(r["normals"][at], axis=0)) == 1     # copies share their neighbourhood: the index decides it, for all alike
