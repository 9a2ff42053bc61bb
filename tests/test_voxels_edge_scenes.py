"""The scenes of tests/voxels_edge_scenes.py have teeth, on the CPU: the points that a cheaper voxel computation would misplace are
there and counted, the wrappers pass the leaf on as a double, the widest map is exactly as wide as include/dcreg.h allows, the tables
have the sizes that were meant, and the reference's mean and covariance (tests/voxels_ref.py) stay within derived rounding bounds of a
numpy.longdouble two-pass computation 1e5 m from the origin.  numpy only, no device."""
from fractions import Fraction

import numpy as np
import pytest

import voxels_edge_scenes as es
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api


# ---- 1. the leaves
@pytest.mark.parametrize("leaf,least", [(0.1, 200), (0.7, 50)])
def test_the_leaf_scenes_hold_points_that_a_cheaper_division_misplaces(leaf, least):
    """leaf 0.1: at least 200 points change voxel when q / leaf is a float32 division; leaf 0.7: at least 50 when it is a multiplication
    by 1.0 / 0.7 (none do at 0.1: that leaf has no teeth for the reciprocal).  Of the floats at and next to the faces k * leaf below
    2 000 m, 102 change voxel under the reciprocal at leaf 0.7, the smallest at |x| = 10.5."""
    S = es.leafy(leaf)
    alt = S["alt"]
    assert alt is (es.voxel_float_division if leaf == 0.1 else es.voxel_reciprocal)
    for cloud in (S["tgt"], S["src"][:S["n_face"]]):
        moved = (alt(cloud, leaf) != vr.voxel_of(cloud, leaf)).any(axis=1)
        print("leaf %g: %d of %d points change voxel under %s" % (leaf, moved.sum(), len(cloud), alt.__name__))
        assert moved.sum() >= least
    assert len(S["tgt"]) < 4000 and np.abs(S["tgt"]).max() < 2000.0
    k, x = es.face_floats(leaf)
    if leaf == 0.7:
        t = es.teeth(x, leaf, es.voxel_reciprocal)
        assert t.sum() == 102 and np.abs(x[t]).min() == 10.5
    else:
        assert not es.teeth(x, leaf, es.voxel_reciprocal).any() and es.teeth(x, leaf, es.voxel_float_division).sum() > 10000
    # every face separates two kept voxels: a float on the wrong side changes the count and the mean of both
    m = S["vmap"]
    assert m["n_small"] == 0 and m["n_degenerate"] == 0 and m["n_kept"] == m["n_voxels"] == 2 * len(S["faces"])
    kept = {tuple(c) for c in m["coords"].tolist()}
    for a, kf in S["faces"]:
        for side in (kf - 1, kf):
            v = [es.CROSS] * 3
            v[a] = side
            assert tuple(v) in kept
    # the source: every face float finds a kept voxel, the points outside the box find none; the misplaced ones would find the neighbour
    idx = vr.find(m, S["src"])
    assert (idx[:S["n_face"]] >= 0).all() and (idx[S["n_face"]:] == -1).all() and len(idx) - S["n_face"] == 6
    moved = np.flatnonzero((alt(S["src"], leaf) != vr.voxel_of(S["src"], leaf)).any(axis=1))
    table = {tuple(c): j for j, c in enumerate(m["coords"].tolist())}
    other = np.array([table[tuple(int(c) for c in alt(S["src"][i:i + 1], leaf)[0])] for i in moved])
    assert (other != idx[moved]).all()


def test_the_wrappers_hand_the_leaf_over_as_the_double_it_is():
    """a leaf narrowed to float32 on its way into the library would move the faces themselves: 0.1f != 0.1"""
    for leaf in (0.1, 0.7, es.WIDE_LEAF, es.WIDE_LEAF_ONE_MORE):
        assert api.voxel_map_params(leaf, vs.EPS, 2).leaf == leaf and list(api.voxel_params(leaf).leaf) == [leaf] * 3
    assert api.voxel_map_params(*es.leafy(0.1)["params"]).min_points == es.LEAF_MIN_POINTS == 2
    assert np.float64(np.float32(0.1)) != 0.1 and np.float64(np.float32(0.7)) != 0.7


# ---- 2. the key widths
def test_the_wide_maps_span_exactly_the_limit_and_one_voxel_more():
    W = es.wide((1 << 20) - 2)
    assert W["span"] == (es.WIDE_SPAN_MAX,) * 3 == ((1 << 21) - 1,) * 3 and len(W["tgt"]) == 27
    m = W["vmap"]
    assert m["n_kept"] == m["n_voxels"] == 4 and sorted(m["count"].tolist()) == [6, 6, 6, 9]
    assert m["coords"].min() == -1048576 and m["coords"].max() == 1048574
    assert np.array_equal(W["tgt"].astype(np.float64), np.round(W["tgt"].astype(np.float64) / es.WIDE_GRID) * es.WIDE_GRID)      # on the grid
    span = tuple(int(b - a).bit_length() for a, b in zip(*vs.box_of(W["tgt"], es.WIDE_LEAF)))
    assert span == (21, 21, 21)                                        # 63 bits of voxel key, 64 with the cloud bit
    idx = vr.find(m, W["src"])
    assert set(idx.tolist()) == {-1, 0, 1, 2, 3} and (idx == -1).sum() > 30
    B = es.wide((1 << 20) - 1)
    assert B["span"] == (1 << 21,) * 3 and B["vmap"]["n_kept"] == 4
    # the same 27 points through the slightly smaller leaf: one voxel more on every axis
    mn, mx = vs.box_of(W["tgt"], es.WIDE_LEAF_ONE_MORE)
    assert (mx - mn + 1).tolist() == [1 << 21] * 3 and es.WIDE_LEAF_ONE_MORE < es.WIDE_LEAF


# ---- 3. the tables
def test_the_table_scenes_have_the_sizes_that_were_meant():
    def slots(n_kept):
        s = 2
        while s < 2 * n_kept:
            s <<= 1
        return s

    want = {"single": (1, 2), "lattice_minus": (4095, 8192), "lattice_plus": (4097, 16384)}
    for name, (n_kept, n_slots) in want.items():
        S = es.TABLES[name]()
        assert S["vmap"]["n_kept"] == n_kept and slots(n_kept) == n_slots, name
        idx = vr.find(S["vmap"], vr.transform(S["T"][:3, :3], S["T"][:3, 3], S["src"]))
        assert (idx >= 0).any() and (idx == -1).any(), name
    assert slots(vs.lattice()["vmap"]["n_kept"]) == 8192
    # the added voxel and the missing one: lattice_plus keeps both, lattice_minus neither
    P, M = es.lattice_plus(), es.lattice_minus()
    tail = slice(len(vs.lattice()["src"]), None)
    q = vr.transform(P["T"][:3, :3], P["T"][:3, 3], P["src"])[tail]
    ip, im = vr.find(P["vmap"], q), vr.find(M["vmap"], q)
    assert (ip[:8] >= 0).sum() >= 6 and (im[:8] == -1).all() and (ip[8:] >= 0).sum() >= 6 and (im[8:] == -1).all()
    F = es.full()
    assert int(F["vmap"]["count"].max()) == es.N_FULL and len(F["tgt"]) == es.N_FULL + len(vs.planted()["tgt"])
    j = int(np.argmax(F["vmap"]["count"]))
    assert F["vmap"]["coords"][j].tolist() == list(es.FULL_VOXEL)
    idx = vr.find(F["vmap"], vr.transform(F["T"][:3, :3], F["T"][:3, 3], F["src"]))
    assert (idx == j).sum() > 250


# ---- 4. far from the origin
def test_the_far_lot_keeps_what_the_lot_keeps_shifted():
    F = es.far_lot()
    m = F["vmap"]
    assert (m["n_voxels"], m["n_kept"]) == (668, 384)
    assert m["coords"].min(axis=0).tolist() == [99878, -60407, 32] and m["coords"].max(axis=0).tolist() == [99901, -60384, 32]
    for pose, n_eff in (("GT", 396), ("INIT", 366)):
        want = vr.linearize(m, F["src"], F[pose])
        assert want["n_eff"] == n_eff and (want["flag"] == 0).any(), pose
    assert vr.linearize(m, F["src"], F["INIT"], 1, F["mb"])["n_eff"] == 278
    # the points sit on the float32 lattice of their magnitude: 2^-7 m on x, 2^-8 m on y
    assert np.spacing(np.abs(F["tgt"][:, 0])).max() == 2.0 ** -7 and np.spacing(np.abs(F["tgt"][:, 1])).max() == 2.0 ** -8


def gamma(n, u):
    nu = n * u
    return nu / (1 - nu)


def test_the_rule_is_accurate_far_from_the_origin():
    """The reference's mean and raw covariance (before the eigen-solve) of every kept voxel of the far lot against a numpy.longdouble
    two-pass computation.  x_j: the voxel's n points as doubles (exact), u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and
    Stability of Numerical Algorithms, lemma 3.1), A = the arithmetic mean.

    The mean.  The left-to-right sum takes n - 1 additions, the division one more rounding: every term passes through at most n of them,
        |mu - A(x)| <= gamma_n * A(|x|) =: E.
    The covariance.  With e = mu - A(x) and d_j = x_j - A(x): sum (x_j - mu)_a (x_j - mu)_b = sum d_ja d_jb + n e_a e_b, because sum d_j = 0 -
    the mean's error enters at second order only.  Every computed term (x_ja - mu_a)(x_jb - mu_b) passes through at most n + 3 roundings
    (the two differences, the product, n - 1 additions, the division), and |x_ja - mu_a| <= |d_ja| + E_a, so with D = A(|d|)
        |C_ab - A(d_a d_b)| <= gamma_(n+3) * (A(|d_a| |d_b|) + E_a D_b + E_b D_a + E_a E_b) + E_a E_b.
    The yardstick's own error is the same two expressions with numpy.longdouble's u (2^-64 on x86) and is added to the bound; the
    comparison is carried out in rational arithmetic.  Measured over the 384 kept voxels (at most 17 points each): the mean's error
    reaches 0.122 of its bound (6.7e-12 m), the covariance's 0.392 of its bound."""
    F = es.far_lot()
    m = F["vmap"]
    ld = np.longdouble
    u, u_ld = Fraction(1, 2 ** 53), Fraction(float(np.finfo(ld).eps)) / 2
    assert u_ld <= u
    v = vr.voxel_of(F["tgt"], vs.LEAF).astype(np.int64)
    fr = lambda x: Fraction(float(x))

    def fr_ld(x):
        """a longdouble as a rational number, exactly (its 64 bits split over two doubles)"""
        hi = np.float64(x)
        return Fraction(float(hi)) + Fraction(float(np.float64(x - ld(hi))))

    worst_mu, worst_c, worst_abs = 0.0, 0.0, 0.0
    for j, c in enumerate(m["coords"]):
        x = F["tgt"][(v == c).all(axis=1)].astype(ld)
        n = len(x)
        assert n == m["count"][j]
        mean = x.sum(axis=0) / ld(n)
        d = x - mean
        mean_abs = np.abs(x).sum(axis=0) / ld(n)
        D = [fr_ld(t) for t in np.abs(d).sum(axis=0) / ld(n)]
        E, E_ld = [], []
        for a in range(3):
            E.append(gamma(n, u) * fr_ld(mean_abs[a]))
            E_ld.append(gamma(n, u_ld) * fr_ld(mean_abs[a]))
            err = abs(fr(m["mean64"][j, a]) - fr_ld(mean[a]))
            bound = E[a] + E_ld[a]
            assert err <= bound, (j, a, float(err), float(bound))
            worst_mu, worst_abs = max(worst_mu, float(err / bound)), max(worst_abs, float(err))
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            want = (d[:, a] * d[:, b]).sum() / ld(n)
            A = fr_ld((np.abs(d[:, a]) * np.abs(d[:, b])).sum() / ld(n))
            bound = gamma(n + 3, u) * (A + E[a] * D[b] + E[b] * D[a] + E[a] * E[b]) + E[a] * E[b]
            bound += gamma(n + 3, u_ld) * (A + E_ld[a] * D[b] + E_ld[b] * D[a] + E_ld[a] * E_ld[b]) + E_ld[a] * E_ld[b]      # (the yardstick's own)
            err = abs(fr(m["cov_raw"][j, k]) - fr_ld(want))
            assert err <= bound, (j, k, float(err), float(bound))
            if bound > 0:
                worst_c = max(worst_c, float(err / bound))
    print("far lot, %d voxels: the mean's error reaches %.3g of its bound (%.3g m), the covariance's %.3g of its bound"
          % (len(m["coords"]), worst_mu, worst_abs, worst_c))
    assert worst_mu > 0.0 and worst_c > 0.0                            # (the comparison is not between a thing and itself)
