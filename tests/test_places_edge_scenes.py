"""The scenes of tests/places_edge_scenes.py have teeth, on the CPU: every decided point is on an edge and is moved to another bin (or
across the range gate) by at least one plausible other evaluation of include/dcreg.h's rule, every other point of an edge cloud is at
least 1e-9 from every edge, mpmath at 60 digits explains each expected bin (the mathematical coordinate on the edge, the double one
below, on or above it), the height and many-cloud scenes hold what was meant, the search scenes cross the three thresholds of the host
loop from both sides, and the small-grid distance table is the literal rule.  numpy and mpmath only, no device."""
import mpmath as mp
import numpy as np
import pytest

import places_edge_scenes as es
import places_ref as pr

mp.mp.dps = 60
U = 2.0 ** -53


def point(scene, x, y):
    """index of the float32 point (x, y) in the scene, by bits"""
    want = np.array([x, y], np.float32).tobytes()
    hit = [k for k in range(len(scene["xy"])) if scene["xy"][k].tobytes() == want]
    assert len(hit) == 1, (x, y, hit)
    return hit[0]


# ---- 1. decided points
@pytest.mark.parametrize("name", sorted(es.GRIDS))
def test_every_decided_point_is_on_an_edge_and_some_alternative_moves_it(name):
    S = es.edge_scene(name)
    p, nd, xy = S["params"], S["n_decided"], S["xy"]
    moved = np.logical_or.reduce(list(S["moved"].values()))
    print("%s: %d decided points, %d clean ones, %d edge points dropped (nothing moves them); moved by %s"
          % (name, nd, len(xy) - nd, S["n_dropped"], {k: int(v.sum()) for k, v in S["moved"].items() if v.any()}))
    assert nd >= 30 and len(moved) == nd and moved.all()
    assert np.array_equal(S["bin"], es.bins(xy, p))
    # the condition on every edge cloud, from the reference alone: decided, or at least 1e-9 from every edge
    assert es.clean_or_decided(S)
    assert len(S["clouds_each"]) == len(xy) and all(len(c) == 1 for c in S["clouds_each"])
    assert np.array_equal(np.concatenate(S["clouds_each"])[:, :2].view(np.uint32), xy.view(np.uint32))
    for c in S["clouds_all"]:
        assert np.array_equal(c[:, :2].view(np.uint32), xy.view(np.uint32)) and c[:, 2].min() >= 1.0 and len(set(c[:, 2].tolist())) == len(c)
    # the reference's own descriptor puts every point alone where the literal rule does
    for k in (0, nd - 1, nd, len(xy) - 1):
        d = pr.descriptor(S["clouds_each"][k], p).reshape(-1)
        assert np.flatnonzero(d).tolist() == ([int(S["bin"][k])] if S["bin"][k] >= 0 else [])
    # where a decided point's angle is not pinned by Annex F (an axis), the header (a diagonal) or absorption (1e-30 beside the +x axis),
    # its sector coordinate is far from every edge: only its ring or the gate is decided there
    x, y = xy[:nd, 0], xy[:nd, 1]
    pinned = (x == 0) | (y == 0) | (np.abs(x) == np.abs(y)) | ((x > 0) & (np.abs(y) == es.TINY))
    _, _, b = pr.bin_coords(np.concatenate([xy[:nd], np.zeros((nd, 1), np.float32)], 1), p)
    assert np.all(pinned | (np.abs(b - np.round(b)) > es.GUARD))


def test_every_alternative_moves_points_of_some_grid_and_the_named_examples_are_there():
    total = {k: 0 for k in es.ALTERNATIVES}
    for name in es.GRIDS:
        for k, v in es.edge_scene(name)["moved"].items():
            total[k] += int(v.sum())
    print(total)
    assert all(n >= 4 for n in total.values()), total
    D = es.edge_scene("default")
    p = D["params"]
    assert D["moved"]["sector_reciprocal"].sum() >= 100 and D["moved"]["max_inclusive"].sum() >= 10
    # the three points of the default grid whose mathematical sector coordinates are 15, 30 and 60
    for (x, y), b_repr, sector in [((0, 4), "14.999999999999998", 14), ((-4, 0), "29.999999999999996", 29), ((4, -1e-30), "59.99999999999999", 59)]:
        k = point(D, x, y)
        _, _, b = pr.bin_coords(np.array([[x, y, 0]], np.float32), p)
        assert k < D["n_decided"] and repr(float(b[0])) == b_repr and D["bin"][k] == 1 * p.n_sectors + sector
    assert D["moved"]["fmod_wrap"][point(D, 4, -1e-30)] and D["moved"]["signbit_wrap"][point(D, 4, -0.0)]
    assert D["bin"][point(D, 4, -0.0)] == p.n_sectors and D["bin"][point(D, -4, -0.0)] == p.n_sectors + 29
    # the gate: rho2 == max_range^2 is outside, the float below it is in the last ring; rho2 == min_range^2 is inside
    for x, y in [(80, 0), (48, 64), (-64, 48), (0, -80)]:
        assert D["bin"][point(D, x, y)] == -1 and D["moved"]["max_inclusive"][point(D, x, y)]
    below = np.nextafter(np.float32(80), np.float32(0))
    assert D["bin"][point(D, 0, below)] == 19 * p.n_sectors + 14 and D["bin"][point(D, 0, np.nextafter(np.float32(80), np.float32(90)))] == -1
    G = es.edge_scene("gated")
    for x, y in [(5, 0), (3, 4), (-4, 3)]:
        k = point(G, x, y)
        assert G["bin"][k] >= 0 and G["moved"]["min_exclusive"][k]
    assert G["bin"][point(G, 0, np.nextafter(np.float32(5), np.float32(0)))] == -1
    # ring edges reached exactly: 27.5 * 28 / 55 == 14, in a grid where 28 / 55 computed first gives 13.999999999999998
    F = es.edge_scene("fiftyfive")
    for x, y in [(27.5, 0), (16.5, 22), (-22, 16.5)]:
        k = point(F, x, y)
        assert F["bin"][k] // 12 == 14 and F["moved"]["ring_ratio"][k]
    # the last ring's clamp: (1, 1) with max_range = fl(sqrt 2) has rho2 = 2 < max_range^2 = 2.0000000000000004 and a == 4.0 == n_rings
    R2 = es.edge_scene("root2")
    k = point(R2, 1, 1)
    _, a, _ = pr.bin_coords(np.array([[1, 1, 0]], np.float32), R2["params"])
    assert a[0] == 4.0 and R2["bin"][k] == 3 * 8 + 1 and R2["moved"]["root_gate"][k]
    # the origin: atan2(+-0, +0) = +-0 and atan2(+-0, -0) = +-pi
    O = es.edge_scene("eighths")
    assert [int(O["bin"][point(O, x, y)]) for x, y in [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]] == [0, 0, 4, 4]


@pytest.mark.parametrize("name", sorted(es.GRIDS))
def test_mpmath_explains_every_expected_bin(name):
    """The reference's a and b of every decided point against mpmath at 60 digits.  a passes through four roundings (the sum of the
    squares, sqrt, the product, the quotient), b through at most six with those of atan2 and of the double 2 pi: |double - exact| <=
    8 * 2^-53 * max(1, exact).  An edge coordinate's exact value lies within 2e-9 of the integer (on it, but for the points 1e-30 beside
    the +x axis), and the bin follows from which side of it the double value fell."""
    S = es.edge_scene(name)
    p, nd = S["params"], S["n_decided"]
    xy = S["xy"][:nd]
    used, a, b = pr.bin_coords(np.concatenate([xy, np.zeros((nd, 1), np.float32)], 1), p)
    tally = {"gate": 0}
    for k in range(nd):
        x, y = mp.mpf(float(xy[k, 0])), mp.mpf(float(xy[k, 1]))
        r2 = x * x + y * y
        a_m = mp.sqrt(r2) * p.n_rings / mp.mpf(p.max_range)
        th = mp.atan2(y, x)
        b_m = (th + 2 * mp.pi if th < 0 else th) * p.n_sectors / (2 * mp.pi)
        origin = xy[k, 0] == 0 and xy[k, 1] == 0                      # (its angle is Annex F's convention, not a limit)
        assert abs(a[k] - a_m) <= 8 * U * max(1, a_m), (name, xy[k])
        assert origin or abs(b[k] - b_m) <= 8 * U * max(1, b_m), (name, xy[k], b[k], b_m)
        on_gate = r2 == mp.mpf(p.min_range) ** 2 or r2 == mp.mpf(p.max_range) ** 2 or float(r2) in (p.min_range * p.min_range, p.max_range * p.max_range)
        explained = on_gate
        tally["gate"] += bool(on_gate)
        for what, v, v_m in (("a", a[k], a_m), ("b", b[k], b_m)):
            if used[k] and abs(v - np.round(v)) <= es.GUARD and not (what == "b" and origin):
                edge = int(np.round(v))
                assert abs(v_m - edge) <= 2e-9, (name, xy[k], what)
                side = "below" if v < edge else "on" if v == edge else "above"
                exact = "exact on" if v_m == edge else "exact below" if v_m < edge else "exact above"
                tally[what + ": " + exact + ", double " + side] = tally.get(what + ": " + exact + ", double " + side, 0) + 1
                assert np.floor(v) == (edge - 1 if side == "below" else edge)
                explained = True
            elif used[k] and what == "b" and origin:
                explained = True
        assert explained, (name, xy[k])
    print(name, tally)
    assert sum(tally.values()) >= nd


# ---- 2. heights and many clouds
def test_the_height_scenes_hold_what_was_meant():
    H = es.height_scenes()
    for name, (p, clouds) in H.items():
        assert all(pr.ambiguous(c, p, es.GUARD) == 0 for c in clouds), name
    p, clouds = H["below"]
    d = pr.descriptor(clouds[0], p)
    assert (d < 0).sum() >= 8 and (d == 0).sum() >= 2 and not (d > 0).any() and d[1, 2] == 0 and d[2, 2] == 0
    assert pr.descriptor(clouds[1], p)[1, 3] == np.float32(-1.0)
    d = pr.descriptor(H["mixed"][1][0], H["mixed"][0])
    assert d[0, 0] == 2.0 and d[1, 4] == 4.0 and d[2, 1] == 1.0 and d[2, 3] == np.float32(np.float64(np.float32(5.001)) - 5.0) and (d != 0).sum() == 4
    assert not pr.descriptor(H["mixed"][1][1], H["mixed"][0]).any()       # values -3 and 0: the bin's largest is 0, as if it were empty
    d = pr.descriptor(H["ends"][1][0], H["ends"][0])
    want = {(0, 0): es.F32_DENORMAL, (0, 1): -es.F32_DENORMAL, (1, 0): es.F32_MAX, (1, 1): -es.F32_MAX, (2, 2): np.float32(3e-45),
            (0, 3): -es.F32_DENORMAL, (2, 4): es.F32_MAX}
    assert all(d[k].tobytes() == np.float32(v).tobytes() for k, v in want.items()) and (d != 0).sum() == len(want)
    d = pr.descriptor(H["minus_zero"][1][0], H["minus_zero"][0])
    assert np.signbit(d[0, 0]) and np.signbit(d[1, 1]) and d[0, 0] == 0 and d[2, 2] == 3.0 and np.signbit(d).sum() == 2
    p, clouds = H["crowd"]
    d = pr.descriptor(clouds[0], p)
    assert len(clouds[0]) == 6004 and (d != 0).sum() == 5 and d[2, 4] == np.float32(clouds[0][:, 2].max() + np.float32(2.0))
    assert (pr.descriptor(H["every"][1][0], H["every"][0]) != 0).all()
    p, clouds = H["one"]
    assert pr.descriptor(clouds[0], p).tolist() == [[float(np.float32(np.float64(clouds[0][:50, 2].max()) + 2.0))]]
    assert pr.descriptor(clouds[1], p).tolist() == [[1.0]] and pr.descriptor(clouds[2], p).tolist() == [[0.0]]
    assert pr.info(clouds, p) == {"n_in": 57, "n_finite": 57, "n_used": 53}


def test_the_many_clouds_straddle_every_tile():
    p, clouds = es.many_clouds()
    n = np.array([len(c) for c in clouds])
    assert len(clouds) == es.N_CROWD and n.max() == 3 and (n == 0).sum() > 1000 and all(pr.ambiguous(c, p, es.GUARD) == 0 for c in clouds)
    nan = sum(1 for c in clouds if len(c) and np.isnan(c).all())
    assert nan > 300
    off = np.concatenate([[0], np.cumsum(n)])
    tiles = -(-off[-1] // 2048)
    assert tiles >= 3
    for t in range(tiles):                          # clouds with a point in tile t
        first, last = np.searchsorted(off, t * 2048, "right") - 1, np.searchsorted(off, min(off[-1], (t + 1) * 2048) - 1, "right") - 1
        assert last - first > 800
    i = pr.info(clouds, p)
    assert i["n_finite"] < i["n_in"] and i["n_used"] == i["n_finite"]


# ---- 3. the search scenes
def launches(ne, k):
    """selection launches of one query batch: chunks of 4 096 candidates, k kept of each, until one chunk is left"""
    n, count = ne, 0
    while True:
        chunks = -(-n // 4096)
        count += 1
        n = chunks * k
        if chunks == 1:
            return count


def test_the_search_scenes_cross_the_thresholds_from_both_sides():
    assert launches(5000, 64) == 2 and launches(262_144, 64) == 2 and launches(262_145, 64) == 3 and launches(262_145, 5) == 2
    assert es.N_LEVELS == 262_146
    batch = (1 << 24) // 262_145
    assert batch == 63 and (1 << 24) // 262_144 == 64
    assert [-(-nq // batch) for nq in (63, 64, 127)] == [1, 2, 3]
    assert (1 << 24) // 40 > 70_000                                    # 40 entries: every query count of the test is one batch
    db, qs, pick = es.levels_scene()
    assert np.array_equal(db[pick == pick[5]], np.repeat(db[5:6], (pick == pick[5]).sum(), 0)) and db.shape == (es.N_LEVELS, 2, 3) and qs.shape == (6, 2, 3) and not qs[2].any()
    rows = np.ascontiguousarray(db).reshape(len(db), -1).view(np.dtype((np.void, 24))).ravel()
    _, inverse, count = np.unique(rows, return_inverse=True, return_counts=True)
    assert 55_000 < len(count) <= 60_000 and count.max() >= 12
    # the copies of an entry lie in different chunks of 4 096: ties cross chunks and levels
    copies = np.flatnonzero(inverse == inverse[200_000])
    assert len(copies) >= 2 and len(set((copies // 4096).tolist())) >= 2
    for nq in (63, 64, 127, 65_535, 65_536, 65_537, 70_000):
        distinct, pick = es.drawn_queries(nq, 64 if nq > 1000 else 8, 60)
        assert len(pick) == nq and set(pick.tolist()) == set(range(len(distinct))) and pick[0] != pick[-1]
        assert all(pick[q] != pick[q - 1] for q in range(63, nq, 63))
        assert len(np.unique(distinct.reshape(len(distinct), -1), axis=0)) == len(distinct)


def test_the_small_grid_table_is_the_literal_rule():
    db, qs, _ = es.levels_scene()
    rng = np.random.default_rng(7)
    sample = np.concatenate([[0, 77, 200_000, es.N_LEVELS - 1], rng.integers(0, es.N_LEVELS, 60), np.flatnonzero(~db.any(axis=(1, 2)))[:2]])
    D = pr.small_table(qs, db[sample])
    assert D.shape == (6, len(sample), 3)
    worst = 0.0
    for q in range(len(qs)):
        for k, e in enumerate(sample):
            worst = max(worst, np.abs(D[q, k] - pr.distances(qs[q], db[e])).max())
    print("small_table against distances: %.3g" % worst)
    assert worst <= 1e-15
    assert np.abs(D - pr.distance_table(qs, db[sample])).max() <= 1e-15
    assert D[0, 2].min() <= 1e-15 and D[1, 1, 1] <= 1e-15 and np.array_equal(D[2], np.ones((len(sample), 3)))
