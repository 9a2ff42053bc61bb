"""Boundary scenes for the four gates of one linearisation (search.hpp plane_of_set / row_of_plane, oracle orc_point_row): the radius
gate (d2[4] < R^2), the normal-norm gate (|x| < min_normal_norm), the thickness gate (maxd < max_plane_thickness_sq) and the weight
gate (s > weight_min).  TEST INFRASTRUCTURE ONLY, like tests/emul.py.

A scene is a target of isolated patches - five neighbours each, spaced far beyond 2 R (1 + cert_margin) - and one source point per
patch; the source is linearised at the identity pose, so every query is its source point.  Each patch probes one gate: one float32
coordinate (a "knob") moves the gate's quantity across its threshold.  The oracle is run on each patch's own small cloud to find, by
bisection over adjacent float32 values of the knob, where its flag flips; the builder emits the knob values 0-3 float steps either
side of the flip.  For the normal-norm, thickness and weight gates it also places cases whose EXACT quantity lies at +-1/2 of each
relative margin of MARGINS (1e-13 .. 1e-7) from the threshold (plane_margin_case: neighbour coordinates in four binades, each placed
by a secant search on exact evaluations); and for the normal-norm gate, axis-aligned planes at exactly 40 m give |x| = 1/40 exactly
against min_normal_norm = 0.025 (a double that is not 1/40).

The exact quantities are those of the exact least-squares plane of [q_j] x = -1 of the float inputs: normal equations in
fractions.Fraction, square roots by mpmath at 50 digits."""
from fractions import Fraction as Fr

import mpmath
import numpy as np

from oracle import pyoracle as po

mpmath.mp.dps = 50

MARGINS = (1e-13, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7)
CERT_MARGIN = 0.05
FLAG_OF_GATE = {"radius": 0, "norm": 2, "thickness": 3, "weight": 4}     # the flag a failed gate gives


# ---------------------------------------------------------------- float32 steps
def fstep(v, k):
    """v (a nonzero float32) moved k float32 steps away from zero (k < 0: towards zero)."""
    v = np.float32(v)
    b = np.array([v]).view(np.int32)[0]
    return np.array([b + np.int32(k)], np.int32).view(np.float32)[0]


def fsteps(v, k):
    """v moved k steps in the direction of +infinity."""
    return fstep(v, k if v > 0 else -k)


# ---------------------------------------------------------------- exact quantities
def _solve3(A, b):
    """exact solution of a 3x3 system of Fractions (Gaussian elimination, exact pivots)"""
    M = [list(A[i]) + [b[i]] for i in range(3)]
    for c in range(3):
        p = next(i for i in range(c, 3) if M[i][c] != 0)
        M[c], M[p] = M[p], M[c]
        for i in range(3):
            if i != c and M[i][c] != 0:
                f = M[i][c] / M[c][c]
                M[i] = [M[i][j] - f * M[c][j] for j in range(4)]
    return [M[i][3] / M[i][i] for i in range(3)]


def exact_plane(Q):
    """x of the exact least-squares solution of [q_j] x = -1 (Q: the five float neighbours) -> three Fractions"""
    P = [[Fr(float(v)) for v in row] for row in np.asarray(Q, np.float32).reshape(5, 3)]
    A = [[sum(p[i] * p[j] for p in P) for j in range(3)] for i in range(3)]
    b = [-sum(p[i] for p in P) for i in range(3)]
    return _solve3(A, b)


def exact_quantities(Q, q, w_slope):
    """exact gate quantities of one patch -> dict: ps = |x|, thick = max_j (n . q_j + d)^2, r = n . q + d, s = 1 - w_slope |r|
    (mpmath at 50 digits; thick is rational)"""
    x = exact_plane(Q)
    ps2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
    P = [[Fr(float(v)) for v in row] for row in np.asarray(Q, np.float32).reshape(5, 3)]
    thick = max((x[0] * p[0] + x[1] * p[1] + x[2] * p[2] + 1) ** 2 for p in P) / ps2
    qq = [Fr(float(v)) for v in np.asarray(q, np.float32)]
    num = x[0] * qq[0] + x[1] * qq[1] + x[2] * qq[2] + 1
    ps = mpmath.sqrt(mpmath.mpf(ps2.numerator) / ps2.denominator)
    r = mpmath.mpf(num.numerator) / num.denominator / ps
    s = 1 - mpmath.mpf(Fr(w_slope).numerator) / Fr(w_slope).denominator * abs(r)
    return {"x": x, "ps": ps, "thick": mpmath.mpf(thick.numerator) / thick.denominator, "r": r, "s": s}


def _mp(v):
    f = Fr(float(v))
    return mpmath.mpf(f.numerator) / f.denominator


def exact_margin(gate, Q, q, prm):
    """(exact quantity - threshold) / threshold of the gate a case probes, from its float inputs.  radius: the quantity is the float
    d2 of the 5th neighbour (both sides compute it with the same IEEE float operations), compared with R^2 in double."""
    if gate == "radius":
        d2 = max(float(np.sum((np.asarray(p, np.float32) - np.asarray(q, np.float32)) ** 2, dtype=np.float32)) for p in Q)
        R2 = _mp(prm["search_radius"]) ** 2
        return (_mp(d2) - R2) / R2
    e = exact_quantities(Q, q, prm["weight_slope"])
    if gate == "norm":
        thr = _mp(prm["min_normal_norm"]); v = e["ps"]
    elif gate == "thickness":
        thr = _mp(prm["max_plane_thickness_sq"]); v = e["thick"]
    else:
        thr = _mp(prm["weight_min"]); v = e["s"]
    return (v - thr) / thr


# ---------------------------------------------------------------- parameters and the oracle on one patch
def params(search_radius=1.0, max_plane_thickness_sq=0.2 * 0.2, min_normal_norm=1e-6, weight_slope=0.9, weight_min=0.1,
           use_weight_derivative=0):
    return dict(search_radius=float(search_radius), max_plane_thickness_sq=float(max_plane_thickness_sq),
                min_normal_norm=float(min_normal_norm), weight_slope=float(weight_slope), weight_min=float(weight_min),
                use_weight_derivative=int(use_weight_derivative))


def oracle_params(prm, euler_rpy=None):
    p = po.default_lin_params(prm["search_radius"], prm["use_weight_derivative"], euler_rpy=euler_rpy)
    p.max_plane_thickness_sq = prm["max_plane_thickness_sq"]; p.min_normal_norm = prm["min_normal_norm"]
    p.weight_slope = prm["weight_slope"]; p.weight_min = prm["weight_min"]
    return p


def oracle_flag(Q, q, prm):
    tree = po.KdTree(np.asarray(Q, np.float32))
    out = po.linearize(tree, np.asarray(q, np.float32).reshape(1, 3), np.eye(3), np.zeros(3), oracle_params(prm), debug=True)
    return int(out["flag"][0])


# ---------------------------------------------------------------- patch geometry
def _unit(rng):
    while True:
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        if np.abs(n).min() > 0.2:
            return n


def _frame(rng, tilted, c):
    if tilted:
        n = _unit(rng)
        a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.8 else np.array([0.0, 1.0, 0.0])
        u = np.cross(n, a); u /= np.linalg.norm(u); v = np.cross(n, u)
    else:
        ax = rng.integers(3)
        n = np.eye(3)[ax]; u = np.eye(3)[(ax + 1) % 3]; v = np.eye(3)[(ax + 2) % 3]
        c = np.round(np.asarray(c) * 8) / 8
    return np.asarray(c, np.float64), n, u, v


class Centres:
    """patch centres 10-50 m out, pairwise farther apart than `spacing` (the patches stay isolated: every query's six nearest and
    its search bound stay inside its own patch)"""

    def __init__(self, rng, spacing):
        self.rng, self.spacing, self.taken = rng, spacing, []

    def ok(self, c):
        return all(np.linalg.norm(c - t) > self.spacing for t in self.taken)

    def take(self, c):
        assert self.ok(c), c
        self.taken.append(np.asarray(c, np.float64))
        return c

    def sample(self, dist=None, axis_value=None):
        for _ in range(100000):
            d = self.rng.normal(size=3); d /= np.linalg.norm(d)
            c = d * (dist if dist is not None else self.rng.uniform(10, 50))
            if axis_value is not None:
                c[self.rng.integers(3)] = axis_value * self.rng.choice([-1.0, 1.0])
            if self.ok(c) and np.abs(c).min() > 3.0:     # (no coordinate near 0: knobs step in float steps of similar size)
                return self.take(c)
        raise RuntimeError("no room for another patch")


_OFFS = np.array([[0.35, 0.05], [-0.3, 0.2], [0.05, -0.38], [-0.22, -0.25], [0.28, 0.3]])


def _patch_points(c, n, u, v, scale, h):
    """five neighbours on the plane through c (in-plane offsets x scale, normal offsets h[j]) -> float32 [5,3]"""
    return np.array([c + a * scale * u + b * scale * v + h[j] * n for j, (a, b) in enumerate(_OFFS)]).astype(np.float32)


class Probe:
    """one patch as a function of an integer knob k: (Q [5,3] float32, q [3] float32)"""

    def __init__(self, gate, prm, Q, q, which, coord, label):
        self.gate, self.prm, self.Q, self.q, self.which, self.coord, self.label = gate, prm, Q, q, which, coord, label

    def at(self, k):
        Q, q = self.Q.copy(), self.q.copy()
        if self.which == "q":
            q[self.coord] = fsteps(q[self.coord], k)
        elif self.which == "all":          # the whole patch along one axis (axis-aligned norm probes: stays exactly planar)
            Q[:, self.coord] = fsteps(Q[0, self.coord], k)
        else:
            Q[self.which, self.coord] = fsteps(Q[self.which, self.coord], k)
        return Q, q


def make_probe(gate, prm, rng, tilted, centres):
    R = prm["search_radius"]
    if gate == "norm":   # the plane 40 m from the origin: |x| = 1 / 40
        c = centres.sample(dist=40.0) if tilted else centres.sample(dist=30.0, axis_value=40.0)
    else:
        c = centres.sample()
    c, n, u, v = _frame(rng, tilted, c)
    if gate == "norm":
        if tilted:                                       # the plane through c, normal to c: 40 m from the origin
            n = c / np.linalg.norm(c)
            a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.8 else np.array([0.0, 1.0, 0.0])
            u = np.cross(n, a); u /= np.linalg.norm(u); v = np.cross(n, u)
        else:
            ax = int(np.argmax(np.abs(c)))               # the coordinate that is +-40
            n, u, v = np.eye(3)[ax] * np.sign(c[ax]), np.eye(3)[(ax + 1) % 3], np.eye(3)[(ax + 2) % 3]
    sgn = rng.choice([-1.0, 1.0])
    h = np.zeros(5)
    q = c.copy()
    if gate == "radius":
        Q = _patch_points(c, n, u, v, 0.6 * R, h)
        d = 0.7 * u + 0.714 * v; d /= np.linalg.norm(d)
        Q[4] = (c + R * d).astype(np.float32)             # the 5th neighbour R away in the plane
        which, coord = 4, int(np.argmax(np.abs(d)))
    elif gate == "norm":
        Q = _patch_points(c, n, u, v, 0.8 * R, h)
        which, coord = ("all", int(np.argmax(np.abs(n)))) if not tilted else (0, int(np.argmax(np.abs(n))))
    elif gate == "thickness":
        t = np.sqrt(prm["max_plane_thickness_sq"])
        sc = 0.8 * R * (0.25 if t < 0.1 else 1.0)
        # the largest residual is linear in the offset of the one point off the plane: calibrate it on a unit offset
        P1 = np.array([[a * sc, b * sc, 1.0 if j == 2 else 0.0] for j, (a, b) in enumerate(_OFFS)])
        A = np.c_[P1[:, :2], np.ones(5)]
        res = P1[:, 2] - A @ np.linalg.lstsq(A, P1[:, 2], rcond=None)[0]
        h[2] = sgn * t / np.abs(res).max()
        for _ in range(5):                                 # (the fit of [q] x = -1 is not the regression above: refine on it)
            Q = _patch_points(c, n, u, v, sc, h)
            h[2] *= np.sqrt(t * t / float(exact_quantities(Q, q, 1.0)["thick"]))
        Q = _patch_points(c, n, u, v, sc, h)
        which, coord = 2, int(np.argmax(np.abs(n)))
    else:
        r_thr = (1.0 - prm["weight_min"]) / prm["weight_slope"]
        Q = _patch_points(c, n, u, v, 0.5, h)
        q = c + sgn * r_thr * n
        which, coord = "q", int(np.argmax(np.abs(n)))
    q = np.asarray(q, np.float32)
    return Probe(gate, prm, Q, q, which, coord, "%s/%s" % ("tilted" if tilted else "axis", gate))


def find_flip(probe):
    """adjacent knob values (k_a, k_a + 1) where the oracle's flag changes, or None"""
    span = 64
    f0 = oracle_flag(*probe.at(0), probe.prm)
    while True:
        if oracle_flag(*probe.at(-span), probe.prm) != f0:
            lo, hi, fl = -span, 0, oracle_flag(*probe.at(-span), probe.prm)
            break
        if oracle_flag(*probe.at(span), probe.prm) != f0:
            lo, hi, fl = 0, span, f0
            break
        span *= 2
        if span > 1 << 21:
            return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        fm = oracle_flag(*probe.at(mid), probe.prm)
        if fm == fl:
            lo = mid
        else:
            hi = mid
    flags = {oracle_flag(*probe.at(lo), probe.prm), oracle_flag(*probe.at(hi), probe.prm)}
    return (lo, hi) if flags == {1, FLAG_OF_GATE[probe.gate]} else None      # a flip of this gate, not of another


# ---------------------------------------------------------------- exact-margin cases of the plane gates (norm, thickness, weight)
_OFFS_L = np.array([[0.35, 0.0], [-0.3, 0.0], [0.05, -0.38], [-0.22, -0.25], [0.28, 0.3]])   # points 0 and 1 share a line along u


def _solve_knob(f, Q, q, pt, i):
    """moves Q[pt, i] over float32 values to the root of the exact residual f(Q, q) (secant steps on exact evaluations; the root is
    then bracketed by adjacent floats) -> the best float placed in Q"""
    def at(v):
        Q[pt, i] = v
        return f(Q, q)
    v0 = Q[pt, i]; f0 = at(v0)
    v1 = fsteps(v0, 64); f1 = at(v1)
    best = min([(abs(f0), v0), (abs(f1), v1)], key=lambda t: t[0])
    for _ in range(12):
        if f1 == f0:
            break
        vn = _mp(v1) - f1 * (_mp(v1) - _mp(v0)) / (f1 - f0)
        if not abs(vn) < 1e30:
            break
        vn = np.float32(float(vn))
        if vn == v1 or not np.isfinite(vn) or np.sign(vn) != np.sign(v1):
            break
        v0, f0, v1 = v1, f1, vn
        f1 = at(v1)
        best = min(best, (abs(f1), v1), key=lambda t: t[0])
    for k in (-2, -1, 1, 2):
        v = fsteps(best[1], k)
        best = min(best, (abs(at(v)), v), key=lambda t: t[0])
    Q[pt, i] = best[1]


def plane_margin_case(gate, prm, rng, centres, target):
    """plane_margin_case_once until the case sits within 2 |target| of the threshold, its neighbours moved by at most 5 cm from where the
    patch put them (the root of the coarse step is the near one) and the oracle's flag is one of this gate's two"""
    for _ in range(50):
        Q, q, Q0 = plane_margin_case_once(gate, prm, rng, centres, target)
        if (np.abs(Q.astype(np.float64) - Q0).max() < 0.05 and abs(float(exact_margin(gate, Q, q, prm))) <= 2 * abs(target)
                and oracle_flag(Q, q, prm) in (1, FLAG_OF_GATE[gate])):
            return Q, q
        centres.taken.pop()
    raise RuntimeError("no %s case at margin %g" % (gate, target))


def plane_margin_case_once(gate, prm, rng, centres, target):
    """a normal-norm, thickness or weight patch on a tilted plane whose EXACT quantity lies at (1 + target) x its threshold.  The patch crosses
    a coordinate plane (coordinate a = 0) with u perpendicular to that axis, so that neighbours 0 and 1 sit on it; their coordinate a
    is set to ~2e-7 and ~1.4e-9 m, float steps of ~1e-14 and ~2e-16 m.  A coarse coordinate (~10-50 m, steps ~4e-6 m) of one
    neighbour, the coordinate a of a third (~0.1-0.5 m) and then those of neighbours 0 and 1 each take up, rounded exactly, what the
    coarser ones left.  -> (Q, q, the patch before the knobs moved)"""
    R = prm["search_radius"]
    t = np.sqrt(prm["max_plane_thickness_sq"])
    f = lambda Q, q: exact_margin(gate, Q, q, prm) - mpmath.mpf(target)
    while True:
        ax = int(rng.integers(3))
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        if not 0.3 <= abs(n[ax]) <= 0.6 or np.abs(n).min() < 0.1:
            continue
        u = np.cross(n, np.eye(3)[ax]); u /= np.linalg.norm(u); v = np.cross(n, u)
        if gate == "norm":
            c = 40.0 * n - 40.0 * n[ax] / v[ax] * v                # on the plane 40 m out, with c[ax] = 0
        else:
            c = rng.normal(size=3); c[ax] = 0.0; c *= rng.uniform(12, 48) / np.linalg.norm(c)
        if np.abs(np.delete(c, ax)).min() > 3.0 and 10 < np.linalg.norm(c) < 50 and centres.ok(c):
            break
    centres.take(c)
    sc = 0.8 * R * (0.25 if (gate == "thickness" and t < 0.1) else 1.0)
    h = np.zeros(5)
    if gate == "weight":
        sc = 0.5
        q = np.asarray(c + 0.02 * u + rng.choice([-1.0, 1.0]) * (1.0 - prm["weight_min"]) / prm["weight_slope"] * n, np.float32)
    else:
        q = np.asarray(c + 0.02 * sc * u, np.float32)
    pts = lambda h: np.array([c + a * sc * u + b * sc * v + h[j] * n for j, (a, b) in enumerate(_OFFS_L)]).astype(np.float32)
    if gate == "thickness":
        h[2] = rng.choice([-1.0, 1.0]) * t
        for _ in range(6):
            h[2] *= np.sqrt(t * t / float(exact_quantities(pts(h), q, 1.0)["thick"]))
    Q = pts(h)
    Q[0, ax] = np.float32(1.5 * 2.0 ** -23) * rng.choice([-1, 1])
    Q[1, ax] = np.float32(1.5 * 2.0 ** -30) * rng.choice([-1, 1])
    Q0 = Q.astype(np.float64)
    coarse = 2 if gate == "thickness" else 4
    mid = max((3, 4, 2), key=lambda j: abs(Q[j, ax]) if abs(Q[j, ax]) < 0.5 else -1.0)
    for pt, i in ((coarse, int(np.argmax(np.abs(n)))), (mid, ax), (0, ax), (1, ax)):
        _solve_knob(f, Q, q, pt, i)
    return Q, q, Q0


# ---------------------------------------------------------------- scenes
class Scene:
    """target [n,3] float32, source [m,3] float32 (query i = source i at the identity pose), per case: gate, label, built-for margin
    (None: a float-step case), exact margin, the oracle's flag on the patch alone"""

    def __init__(self, name, prm):
        self.name, self.prm = name, prm
        self.patches = []          # (Q, q, gate, label, margin_built, k_from_flip)

    def add(self, Q, q, gate, label, margin_built=None, step=None):
        self.patches.append((Q, q, gate, label, margin_built, step))

    def finish(self):
        self.target = np.concatenate([p[0] for p in self.patches]).astype(np.float32)
        self.source = np.array([p[1] for p in self.patches], np.float32)
        return self


def _spacing(prm):
    R = prm["search_radius"]
    return 2 * R * (1 + CERT_MARGIN) + 2 * (max(R, 1.5) + 0.5) + 2.0


def build_scene(name, prm, gates, seed, n_tilted=3, n_axis=2, ladder=0, steps=3):
    """one scene with patches probing `gates` under parameters `prm`: per probe slot (tilted / axis-aligned) a fresh patch for every
    offset 0..steps float steps on either side of the oracle's flip; and `ladder` patches on either side of the threshold at every
    exact margin of MARGINS"""
    rng = np.random.default_rng(seed)
    centres = Centres(rng, _spacing(prm))
    sc = Scene(name, prm)
    for gate in gates:
        for tilted in [True] * n_tilted + [False] * n_axis:
            for j in range(steps + 1):
                for side in (-1, 1):
                    for _attempt in range(20):
                        probe = make_probe(gate, prm, rng, tilted, centres)
                        flip = find_flip(probe)
                        if flip is not None:
                            break
                    assert flip is not None, (name, probe.label)
                    k = flip[0] - j if side < 0 else flip[1] + j
                    Q, q = probe.at(k)
                    sc.add(Q, q, gate, probe.label, None, side * (j + 1))
            if gate == "norm" and not tilted:
                # planes exactly 40 m out: |x| = 1/40 exactly, against the double 0.025
                for _ in range(2):
                    probe = make_probe(gate, prm, rng, False, centres)
                    Q, q = probe.at(0)
                    Q[:, probe.coord] = np.float32(40.0) * np.sign(Q[0, probe.coord])
                    sc.add(Q, q, gate, probe.label, 1e-13, 0)
        if ladder:
            for m in MARGINS:
                for sgn in (-0.5, 0.5) * ladder:
                    Q, q = plane_margin_case(gate, prm, rng, centres, sgn * m)
                    sc.add(Q, q, gate, "tilted/%s" % gate, m, 0)
    return sc.finish()


def r_zero_scene(prm, seed=77):
    """queries exactly on (axis-aligned) and within a few float steps of planes: r = 0 or nearly, the branch of ds"""
    rng = np.random.default_rng(seed)
    centres = Centres(rng, _spacing(prm))
    sc = Scene("r0 wd=%d" % prm["use_weight_derivative"], prm)
    for tilted in (False, False, True, True):
        for k in range(-3, 4):
            c, n, u, v = _frame(rng, tilted, centres.sample())
            Q = _patch_points(c, n, u, v, 0.5, np.zeros(5))
            ax = int(np.argmax(np.abs(n)))
            q = np.asarray(c, np.float32).copy()
            if not tilted:
                q[ax] = Q[0, ax]
            q[ax] = fsteps(q[ax], k)
            sc.add(Q, q, "weight", "%s/r0" % ("tilted" if tilted else "axis"), None, k)
    return sc.finish()


def all_scenes():
    """every boundary scene of the suite: (scene) list; deterministic"""
    P = params
    out = []
    for i, R in enumerate((1.0, 0.3, 0.7)):
        out.append(build_scene("radius R=%g" % R, P(search_radius=R), ["radius"], seed=10 + i))
    out.append(build_scene("norm 1/40", P(min_normal_norm=1.0 / 40.0), ["norm"], seed=20, ladder=3))
    out.append(build_scene("thickness 0.04", P(), ["thickness"], seed=30, ladder=2))
    out.append(build_scene("thickness 0.02^2", P(max_plane_thickness_sq=0.02 ** 2), ["thickness"], seed=31, ladder=2))
    for j, (slope, wmin) in enumerate(((0.9, 0.1), (0.5, 0.3))):
        for wd in (0, 1):
            prm = P(search_radius=2.5, weight_slope=slope, weight_min=wmin, use_weight_derivative=wd)
            out.append(build_scene("weight %g/%g wd=%d" % (slope, wmin, wd), prm, ["weight"], seed=40 + 2 * j + wd, ladder=1))
    for wd in (0, 1):
        out.append(r_zero_scene(P(search_radius=2.5, use_weight_derivative=wd), seed=77 + wd))
    return out
