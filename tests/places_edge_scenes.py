"""Seeded scenes that put the place descriptors of include/dcreg.h where their rules decide something: points on ring edges, on sector
edges and on the range gate whose bin is still fixed by the header's literal double evaluation, heights at the ends of the float range,
and thousands of tiny clouds in one call.  numpy only; tests/test_places_edge_scenes.py shows on the CPU that the scenes have teeth, and
tests/test_gpu_places_edges.py holds the device to them.

A *decided* point lies on an edge (its ring or sector coordinate within 1e-9 of an integer under tests/places_ref.py, or rho2 equal to a
bound of the range gate) and some plausible other evaluation of the same rule puts it in another bin or on the other side of the gate.
Its bin is what the literal rule gives, and a device that evaluates the rule in another order gets it wrong.  Where the rule is pinned
bit for bit: the squares and their sum are one rounding, sqrt is correctly rounded by IEEE 754, the products and quotients are single
operations in the order the header writes them, and atan2 is fixed by C Annex F.10.1.4 at the points used here - on the axes (+-0, +-pi,
+-pi/2 rounded) - and, for |x| == |y|, is the correctly rounded pi/4 or 3 pi/4 that include/dcreg.h asks for by name.  Edge points that no
alternative moves prove nothing and are dropped; every other point of a scene is at least 1e-9 from every edge."""
from fractions import Fraction

import numpy as np

import places_ref as pr
from dcreg_amd import api

TWO_PI = pr.TWO_PI
GUARD = 1e-9
TINY = np.float32(1e-30)
TRIPLES = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29))
DIAGONALS = (2.0 ** -10, 0.5, 1.0, 3.0, 5.0, 7.0, 11.0, 20.0, 40.0)

# the grids of the decided points.  thirty7 / thirty13: a ring width that binary cannot represent; gated: the 3-4-5 point on min_range;
# eighths and widest: the diagonals are sector edges; fiftyfive: 27.5 * 28 / 55 is 14 but 27.5 * (28 / 55) is below it; root2:
# sqrt(rho2) == max_range in double although rho2 < max_range^2, the one way to the last ring's clamp (a == n_rings)
GRIDS = {"default": api.place_params(), "thirty7": api.place_params(7, 13, 30.0), "thirty13": api.place_params(13, 7, 30.0),
         "gated": api.place_params(16, 40, 20.0, 5.0, 2.0), "eighths": api.place_params(12, 8, 30.0),
         "fiftyfive": api.place_params(28, 12, 55.0), "root2": api.place_params(4, 8, float(np.sqrt(2.0))),
         "widest": api.place_params(64, 128, 64.0), "one": api.place_params(1, 1, 50.0)}


def bins(xy, p, ring_mul=None, sector_mul=None, single=False, root_gate=False, max_inclusive=False, min_exclusive=False, signbit_wrap=False,
         fmod_wrap=False):
    """the bin of every point of xy [n, 2] float32 (-1: outside the range gate).  Without options this is the header's rule as
    places_ref.bin_coords evaluates it; every option swaps one step for something a kernel could plausibly do instead"""
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    r2 = x * x + y * y
    lo, hi = p.min_range * p.min_range, p.max_range * p.max_range
    rho = np.sqrt(r2.astype(np.float32)).astype(np.float64) if single else np.sqrt(r2)
    if root_gate:
        used = (rho >= p.min_range) & (rho < p.max_range)
    else:
        used = (r2 > lo if min_exclusive else r2 >= lo) & (r2 <= hi if max_inclusive else r2 < hi)
    a = rho * ring_mul if ring_mul is not None else rho * p.n_rings / p.max_range
    th = np.arctan2(xy[:, 1], xy[:, 0]).astype(np.float64) if single else np.arctan2(y, x)
    th = np.fmod(th + TWO_PI, TWO_PI) if fmod_wrap else np.where(np.signbit(th) if signbit_wrap else th < 0.0, th + TWO_PI, th)
    b = th * sector_mul if sector_mul is not None else th * p.n_sectors / TWO_PI
    ring = np.minimum(np.floor(a).astype(np.int64), p.n_rings - 1)
    sector = np.minimum(np.floor(b).astype(np.int64), p.n_sectors - 1)
    return np.where(used, ring * p.n_sectors + sector, -1)


# The other evaluations.  The first five are the ones a faster kernel is most likely to use; the last four are the comparisons the
# header spells out (min_range^2 <= rho2 < max_range^2, "plus 2 pi when negative": -0.0 is not negative, and an angle that the sum
# rounds to 2 pi stays there for the clamp) turned the other way
ALTERNATIVES = {
    "sector_reciprocal": lambda p: dict(sector_mul=p.n_sectors * (1.0 / TWO_PI)),
    "sector_ratio": lambda p: dict(sector_mul=p.n_sectors / TWO_PI),
    "ring_ratio": lambda p: dict(ring_mul=p.n_rings / p.max_range),
    "single": lambda p: dict(single=True),
    "root_gate": lambda p: dict(root_gate=True),
    "max_inclusive": lambda p: dict(max_inclusive=True),
    "min_exclusive": lambda p: dict(min_exclusive=True),
    "signbit_wrap": lambda p: dict(signbit_wrap=True),
    "fmod_wrap": lambda p: dict(fmod_wrap=True),
}


def _neighbours(v):
    v = np.asarray(v, np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def _exact32(fr):
    """the float32 that equals the rational number fr, or None"""
    v = np.float32(float(fr))
    return v if np.isfinite(v) and Fraction(float(v)) == fr else None


def candidates(p):
    """float32 points [n, 2] on and next to the edges of p's grid: the axes with both zeros, +-1e-30 beside the +x axis, Pythagorean
    points whose radius is a ring edge or a bound of the gate, the diagonals - each with its float neighbours"""
    R = p.n_rings
    ks = range(R + 1) if R <= 32 else (0, 1, 2, R // 2, R - 1, R)
    width = Fraction(p.max_range) / R
    edges = [k * width for k in ks] + [Fraction(p.min_range)]
    radii = _neighbours(np.array([float(e) for e in edges], np.float32))
    radii = np.unique(radii[radii >= 0.0])
    pts = []
    for other in (np.float32(0.0), np.float32(-0.0)):
        o = np.full(len(radii), other, np.float32)
        pts += [np.stack([radii, o], 1), np.stack([-radii, o], 1), np.stack([o, radii], 1), np.stack([o, -radii], 1)]
    for other in (TINY, -TINY):              # beside the +x axis only: there atan2 is +-y / x and 2 pi absorbs it, whatever the library
        pts.append(np.stack([radii[radii > 0.0], np.full(int((radii > 0.0).sum()), other, np.float32)], 1))
    for e in edges:
        for ta, tb, tc in TRIPLES:
            xa, xb = _exact32(e * ta / tc), _exact32(e * tb / tc)
            if e == 0 or xa is None or xb is None:
                continue
            for u, v in ((xa, xb), (xb, xa)):
                un, vn = _neighbours([u]), _neighbours([v])
                for su in (1, -1):
                    for sv in (1, -1):
                        pts.append(np.stack([su * un, np.full(3, sv * v, np.float32)], 1))
                        pts.append(np.stack([np.full(3, su * u, np.float32), sv * vn], 1))
    d = np.array(DIAGONALS, np.float32)
    for su in (1, -1):
        for sv in (1, -1):
            pts.append(np.stack([su * d, sv * d], 1))
    xy = np.ascontiguousarray(np.concatenate(pts, 0), np.float32)
    _, first = np.unique(xy.view(np.uint32).astype(np.uint64) @ np.array([1 << 32, 1], np.uint64), return_index=True)      # (by bits: both zeros stay)
    return xy[np.sort(first)]


def on_edge(xy, p):
    """points on an edge: used with a or b within GUARD of an integer (places_ref.ambiguous counts exactly these), or rho2 equal to a
    bound of the gate"""
    cloud = np.concatenate([xy, np.zeros((len(xy), 1), np.float32)], 1)
    used, a, b = pr.bin_coords(cloud, p)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    r2 = x * x + y * y
    near = (np.abs(a - np.round(a)) <= GUARD) | (np.abs(b - np.round(b)) <= GUARD)
    return (used & near) | (r2 == p.min_range * p.min_range) | (r2 == p.max_range * p.max_range)


_cache = {}


def edge_scene(name):
    """-> dict: params, xy (the scene's points, decided ones first), n_decided, bin (the literal rule's), moved {alternative: bool per
    decided point}, n_dropped (edge points that no alternative moves: not in the scene), clouds_each (one cloud per point) and
    clouds_all (every point in one cloud, heights rising and falling along it).  Heights lie in [1, 2): with the grid's z_offset every
    value is positive, so one point alone shows its bin"""
    if name in _cache:
        return _cache[name]
    p = GRIDS[name]
    xy = candidates(p)
    lit = bins(xy, p)
    edge = on_edge(xy, p)
    moved = {k: bins(xy, p, **make(p)) != lit for k, make in ALTERNATIVES.items()}
    any_moved = np.logical_or.reduce(list(moved.values()))
    decided, rest = edge & any_moved, ~edge
    order = np.concatenate([np.flatnonzero(decided), np.flatnonzero(rest)])
    pts, nd = xy[order], int(decided.sum())
    z = (1.0 + np.arange(len(pts)) / len(pts)).astype(np.float32)
    each = [np.array([[x, y, h]], np.float32) for (x, y), h in zip(pts, z)]
    both = [np.concatenate([pts, z[:, None]], 1), np.concatenate([pts, z[::-1, None]], 1)]
    out = {"params": p, "xy": pts, "n_decided": nd, "bin": lit[order], "moved": {k: v[order][:nd] for k, v in moved.items()},
           "n_dropped": int((edge & ~any_moved).sum()), "clouds_each": each, "clouds_all": both}
    _cache[name] = out
    return out


def clean_or_decided(scene):
    """the condition on every edge cloud, from the reference alone: beyond the decided points no used point lies within GUARD of an edge"""
    p, nd = scene["params"], scene["n_decided"]
    rest = np.concatenate([scene["xy"][nd:], np.ones((len(scene["xy"]) - nd, 1), np.float32)], 1)
    return pr.ambiguous(rest, p, GUARD) == 0 and not on_edge(scene["xy"][nd:], p).any() and bool(on_edge(scene["xy"][:nd], p).all())


# ---- heights
def inside(p, ring, sector, rng):
    """a point 0.2 .. 0.8 into the bin (ring, sector) on both coordinates -> (x, y)"""
    ring, sector = np.asarray(ring), np.asarray(sector)
    rho = (ring + rng.uniform(0.2, 0.8, ring.shape)) * p.max_range / p.n_rings
    th = (sector + rng.uniform(0.2, 0.8, ring.shape)) * TWO_PI / p.n_sectors
    return rho * np.cos(th), rho * np.sin(th)


def _cloud(p, ring, sector, z, rng):
    x, y = inside(p, ring, sector, rng)
    return np.stack([x, y, np.asarray(z, np.float64)], 1).astype(np.float32)


F32_MAX, F32_DENORMAL = np.float32(3.4028235e38), np.float32(1e-45)


def height_scenes():
    """-> {name: (params, clouds)}.  below: every value negative (z_offset -5), so an occupied bin keeps its largest negative value and
    only an empty one is 0; mixed: bins with values of both signs; ends: denormal and largest-finite heights with z_offset 0 (the
    conversions are exact); minus_zero: a bin whose only value is -0.0 keeps that sign; crowd: 6 000 points in one bin and a few beside
    it; every: one point in every bin; one: the 1 x 1 grid"""
    if "heights" in _cache:
        return _cache["heights"]
    rng = np.random.default_rng(41)
    out = {}
    p = api.place_params(3, 5, 10.0, 0.0, -5.0)
    ring, sector = rng.integers(0, 3, 40), rng.integers(0, 5, 40)
    ring[sector == 2] = 0                                             # bins (1, 2) and (2, 2) stay empty
    out["below"] = (p, [_cloud(p, ring, sector, rng.uniform(0.0, 3.0, 40), rng), _cloud(p, [1], [3], [4.0], rng)])
    z = np.array([1.0, 7.0, 2.0, 9.0, 6.0, 5.0, 4.999, 5.001])
    out["mixed"] = (p, [_cloud(p, [0, 0, 1, 1, 2, 2, 2, 2], [0, 0, 4, 4, 1, 1, 3, 3], z, rng), _cloud(p, [1, 1], [1, 1], [5.0, 2.0], rng)])
    p0 = api.place_params(3, 5, 10.0, 0.0, 0.0)
    ends = [F32_DENORMAL, -F32_DENORMAL, F32_MAX, -F32_MAX, F32_DENORMAL, np.float32(3e-45), -F32_MAX, -F32_DENORMAL, F32_MAX, np.float32(1.0)]
    out["ends"] = (p0, [_cloud(p0, [0, 0, 1, 1, 2, 2, 0, 0, 2, 2], [0, 1, 0, 1, 2, 2, 3, 3, 4, 4], ends, rng)])
    pm = api.place_params(3, 5, 10.0, 0.0, -0.0)
    out["minus_zero"] = (pm, [_cloud(pm, [0, 1, 1, 2], [0, 1, 1, 2], [-0.0, -0.0, -1.0, 3.0], rng)])
    pc = api.place_params(4, 6, 12.0)
    crowd = _cloud(pc, np.full(6000, 2), np.full(6000, 4), rng.uniform(-1.9, 3.0, 6000), rng)
    beside = _cloud(pc, [2, 2, 1, 3], [3, 5, 4, 4], [0.5, 0.25, 0.75, 1.5], rng)
    out["crowd"] = (pc, [np.concatenate([crowd[:3000], beside, crowd[3000:]]), crowd[:2049], beside])
    rr, ss = np.divmod(np.arange(24), 6)
    out["every"] = (pc, [_cloud(pc, rr, ss, rng.uniform(-1.9, 3.0, 24), rng)[rng.permutation(24)]])
    p1 = api.place_params(1, 1, 50.0, 0.0, 2.0)
    far = np.array([[60.0, 1.0, 99.0], [-30.0, -41.0, 9.0]], np.float32)                        # outside the range
    low = _cloud(p1, [0, 0], [0, 0], [-1.0, -1.5], rng)
    out["one"] = (p1, [np.concatenate([_cloud(p1, np.zeros(50, int), np.zeros(50, int), rng.uniform(-1.0, 3.0, 50), rng), far, low[1:]]), low, far])
    _cache["heights"] = out
    return out


# ---- many clouds
N_CROWD = 5000


def many_clouds():
    """-> (params, clouds): 5 000 clouds of 0 .. 3 points in one call, about every ninth of them nothing but NaN, so that every tile of
    2 048 points straddles more than a thousand clouds and every point finds its cloud by itself"""
    if "many" in _cache:
        return _cache["many"]
    p = api.place_params()
    rng = np.random.default_rng(43)
    clouds = []
    for k in range(N_CROWD):
        n = int(rng.integers(0, 4))
        c = _cloud(p, rng.integers(0, p.n_rings, n), rng.integers(0, p.n_sectors, n), rng.uniform(-1.5, 4.0, n), rng).reshape(n, 3)
        if n and k % 9 == 4:
            c[:] = np.nan
        clouds.append(c)
    _cache["many"] = (p, clouds)
    return _cache["many"]


# ---- the search past its limits: grids of 2 x 3 bins
SMALL = api.place_params(2, 3, 10.0)
N_LEVELS = 262_146                    # a database one entry larger than the 262 145 that need a third selection launch with k = 64


def small_descriptors(n, seed, n_distinct=None):
    """n descriptors of SMALL's grid: heights in [0, 6), a fifth of the bins 0 (so columns and whole descriptors are empty now and
    then).  n_distinct: drawn with replacement from that many, so that most appear several times"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 6.0, (n_distinct or n, SMALL.n_rings, SMALL.n_sectors)).astype(np.float32)
    base[rng.uniform(size=base.shape) < 0.2] = 0.0
    if n_distinct is None:
        return base, np.arange(n)
    pick = rng.integers(0, n_distinct, n)
    return base[pick], pick


def levels_scene():
    """-> (db [262 146, 2, 3] drawn from 60 000 distinct descriptors - 4.4 copies of each on average, spread over the whole index range,
    so exact ties cross every chunk and level of the selection - 6 queries: two entries' copies, an all-zero one, three random - and
    pick [262 146]: entries with the same number are copies of one descriptor)"""
    if "levels" in _cache:
        return _cache["levels"]
    db, pick = small_descriptors(N_LEVELS, 51, 60_000)
    qs, _ = small_descriptors(6, 52)
    qs[0], qs[1], qs[2] = db[200_000], np.roll(db[77], -1, axis=1), 0.0
    _cache["levels"] = (db, qs, pick)
    return _cache["levels"]


def drawn_queries(nq, n_distinct, seed):
    """-> (distinct [n_distinct, 2, 3], pick [nq]): query q is distinct[pick[q]]; every distinct one is used, the first and the last
    query differ, and so do the two on either side of every multiple of 63 (the batch of a 262 145-entry range)"""
    distinct, _ = small_descriptors(n_distinct, seed)
    distinct[1] = 0.0
    rng = np.random.default_rng(seed + 1)
    pick = rng.integers(0, n_distinct, nq)
    pick[:min(nq, n_distinct)] = np.arange(min(nq, n_distinct))
    for q in range(1, nq):
        if q % 63 == 0 and pick[q] == pick[q - 1]:
            pick[q] = (pick[q] + 1) % n_distinct
    if nq > 1 and pick[-1] == pick[0]:
        pick[-1] = (pick[0] + 1) % n_distinct
    return distinct, pick
