"""The systems of the solver-seam edge tests: small 6 x 6 normal equations H x = g whose entries are integers or integers times a power of
two, so that H is exact in double and the 50-digit reference (solver_ref.py) sees the very matrix the library sees.

Geometric systems are sums of point-to-plane rows [p x n, n] with integer points p and integer normals n: an axis or a Pythagorean
triple (3, 4, 0), (2, 2, 1), ... left unnormalised - the row of the unit normal times its integer length c, that is the point weighted by
c^2.  g = sum of row * residual with small integer residuals, so that g lies in the range of H as it does in a registration.

Every entry of SYSTEMS is (name, family, H, g); CONFIGS are the four configurations every system runs under."""
import itertools

import numpy as np

# (KAPPA_TARGET, always_compute_schur): 1 is the default (the preconditioner is a multiple of I per block)
CONFIGS = [(1.0, 0), (10.0, 1), (1.0, 1), (10.0, 0)]
THRES_COND, THRES_EIG = 10.0, 120.0          # the defaults (utils.hpp:83-84): the threshold families are laid around them


def _resid(k):
    return (k * 7 + 3) % 5 - 2


def rows_system(points, normals):
    rows = np.array([np.concatenate([np.cross(p, n), n]) for p, n in zip(points, normals)], dtype=np.int64)
    r = np.array([_resid(k) for k in range(len(rows))], dtype=np.int64)
    H = rows.T @ rows
    g = rows.T @ r
    assert np.abs(H).max() < 2 ** 50
    return H.astype(np.float64), g.astype(np.float64)


def _grid(a, b):
    return list(itertools.product(a, b))


X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def plane():            # z = 0, normal z: rank 3, the null space is spanned by axes (rot z, trans x, trans y)
    pts = [(x, y, 0) for x, y in _grid(range(-2, 3), range(-2, 3))]
    return rows_system(pts, [Z] * len(pts))


def plane_tilted():     # 3x + 4y = 0, normal (3, 4, 0): rank 3, no axis in the null space
    pts = [(4 * a, -3 * a, b) for a, b in _grid(range(-2, 3), range(-2, 3))]
    return rows_system(pts, [(3, 4, 0)] * len(pts))


def corridor():         # walls x = +-2 and the floor z = 0: rank 5, translation along y is free
    walls = [(s * 2, y, z) for s in (-1, 1) for y, z in _grid(range(-2, 3), range(0, 3))]
    floor = [(x, y, 0) for x, y in _grid(range(-2, 3), range(-2, 3))]
    return rows_system(walls + floor, [X] * len(walls) + [Z] * len(floor))


def sphere():           # about the origin, n parallel to p: the rotation block and the cross block are exactly 0
    pts = [(3, 4, 0), (0, 3, 4), (4, 0, 3), (2, 2, 1), (1, 2, 2), (-2, 1, 2), (6, 2, 3), (-3, 0, 4), (0, -4, 3), (2, -1, -2), (-1, -2, 2), (0, 0, -5)]
    return rows_system(pts, pts)


def cylinder():         # radius 5 about z: rank 4, rotation about z and translation along z are free
    ring = [(5, 0, 0), (0, 5, 0), (-5, 0, 0), (0, -5, 0), (3, 4, 0), (-4, 3, 0), (4, -3, 0), (-3, -4, 0)]
    pts, nrm = [], []
    for z in range(-2, 3):
        for q in ring:
            pts.append((q[0], q[1], z))
            nrm.append(tuple(v // 5 for v in q) if 0 in q[:2] else q)
    return rows_system(pts, nrm)


def line():             # points on the x axis: the rotation about it is free
    nrm = [Y, Z, (0, 3, 4), X]
    pts = [(t, 0, 0) for t in range(-4, 8)]
    return rows_system(pts, [nrm[k % 4] for k in range(len(pts))])


def rank_one():         # one row, repeated
    row = np.array([1, 2, -1, 2, 1, 3], dtype=np.float64)
    return 4.0 * np.outer(row, row), 6.0 * row


def box():              # six faces, points off centre: full rank, the control
    pts, nrm = [], []
    for s in (-1, 1):
        for a, b in _grid(range(-1, 3), range(0, 3)):
            pts += [(2 * s, a, b), (a, 2 * s, b), (a, b + 1, 2 * s)]
            nrm += [X, Y, Z]
    return rows_system(pts, nrm)


def _ulp(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


G = np.array([1.0, -2.0, 3.0, -1.0, 2.0, 1.0])
# one value at the threshold, one ulp and 2^-10 (about 1e-3) relative either side
VARIANTS = [("at", lambda v: v), ("ulp_above", lambda v: _ulp(v, 1)), ("ulp_below", lambda v: _ulp(v, -1)),
            ("1e-3_above", lambda v: v * (1 + 2.0 ** -10)), ("1e-3_below", lambda v: v * (1 - 2.0 ** -10))]


def threshold_systems():
    """diagonal H - a diagonal matrix conjugated by a signed permutation is the diagonal permuted, hence `placements` -: every eigenvalue is an
    entry, every quotient below is a double divided by a power of two, and both the library and the reference see them exactly"""
    out = []
    lo = 128.0
    for tag, f in VARIANTS:
        hi = f(THRES_COND * lo)                                   # hi / lo against DEGENERACY_THRES_COND
        # the pair in the rotation block (Schur / diagonal-block detection of that block, and the full spectrum's extremes), in the
        # translation block, and split over both (the blocks themselves stay benign: only the full-spectrum detections see it)
        out.append(("cond_%s_rot" % tag, np.diag([lo, hi, 256.0, 384.0, 512.0, 1024.0])))
        out.append(("cond_%s_trans" % tag, np.diag([256.0, 512.0, 1024.0, hi, 384.0, lo])))
        out.append(("cond_%s_split" % tag, np.diag([hi, 512.0, 1024.0, 256.0, lo, 384.0])))
        e = f(THRES_EIG)                                          # an eigenvalue against DEGENERACY_THRES_EIG
        out.append(("eig_%s_rot" % tag, np.diag([512.0, e, 256.0, 384.0, 768.0, 1024.0])))
        out.append(("eig_%s_trans" % tag, np.diag([256.0, 512.0, 1024.0, 768.0, 384.0, e])))
    return [(n, "threshold", H, G.copy()) for n, H in out]


def repeated_systems():
    v1, v2 = np.array([1.0, 1, 1, 1, 0, 0]), np.array([1.0, -1, 0, 0, 1, 1])      # |v|^2 = 4, orthogonal
    dense = 5.0 * np.eye(6) - np.outer(v1, v1) - np.outer(v2, v2)                   # Q diag(5, 5, 5, 5, 1, 1) Q^T, dense
    return [("aaabbb", "repeated", np.diag([64.0, 64, 64, 256, 256, 256]), G.copy()),
            ("identity", "repeated", np.eye(6), G.copy()),
            ("dense_5555_11", "repeated", dense, G.copy())]


def nonfinite_systems():
    """the box with one non-finite entry: in the rotation block, the translation block, the cross block (both mirror entries), and g"""
    H0, g0 = box()
    out = []
    for vname, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        for pname, pos in (("rot", (0, 1)), ("trans", (4, 4)), ("cross", (1, 4)), ("g", None)):
            H, g = H0.copy(), g0.copy()
            if pos is None:
                g[2] = v
            else:
                H[pos] = H[pos[::-1]] = v
            out.append(("%s_%s" % (vname, pname), "nonfinite", H, g))
    return out


def _systems():
    out = [(f.__name__, f.__name__, *f()) for f in (plane, plane_tilted, corridor, sphere, cylinder, line, rank_one, box)]
    out += threshold_systems() + repeated_systems()
    H, g = box()
    out += [("box_2^-40", "scale", H * 2.0 ** -40, g * 2.0 ** -40), ("box_2^40", "scale", H * 2.0 ** 40, g * 2.0 ** 40)]   # about 1e-12 and 1e12, exactly
    out.append(("zero", "improper", np.zeros((6, 6)), np.zeros(6)))
    out.append(("indefinite", "improper", H - 64.0 * np.eye(6), g.copy()))         # the box minus a multiple of I: some eigenvalues negative
    return out


SYSTEMS = _systems()                    # finite
NONFINITE = nonfinite_systems()
DETERMINATE = ("threshold", "repeated", "scale", "box", "corridor")      # families in which no cell may be undecidable
