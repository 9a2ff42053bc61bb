"""numpy reference of the surface normals (include/dcreg.h, "surface normals and curvature"): the rule, literally.

For one cloud of n points and the parameters k (3 .. 32), search_radius (>= 0, 0 = unbounded), orient and viewpoint[3] (double):
  - a point is USED when x, y and z are all finite; the others get NaN in every output.  "Index" is the input index;
  - distances are the float d2 that dcreg_knn computes ((dx*dx + dy*dy) + dz*dz, every operation rounded to float); candidates are ranked by
    the total order (d2, index);
  - the neighbours of point i are the first k used points of the cloud in that order with d2 < bound, the point itself a candidate like any
    other (d2 = 0); bound = min((float)(search_radius^2), 3.0e38f) for search_radius > 0 and 3.0e38f (the bound of every unbounded search
    of the library) for search_radius = 0.  A used point with fewer than k such neighbours is SPARSE: NaN outputs, counted in n_sparse;
  - covariance, in double, every multiply and add rounded once: e_j = (double)q_j - (double)p_i for the neighbours q_1 .. q_k in rank
    order; s = e_1 + e_2 + ... left to right; m = s / k; d_j = e_j - m; C_ab = (sum_j d_ja * d_jb) / k left to right, for xx xy xz yy yz zz;
  - cyclic Jacobi, exactly six sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the third index, V = I at the start:
        t = 0 if a_pq == 0, else theta = (a_qq - a_pp) / (2 * a_pq), t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta*theta + 1))
        c = 1 / sqrt(t*t + 1); s = t * c
        a_pp <- a_pp - t*a_pq; a_qq <- a_qq + t*a_pq; a_pq <- 0
        a_rp <- c*a_rp - s*a_rq; a_rq <- s*a_rp(old) + c*a_rq
        v_ip <- c*v_ip - s*v_iq; v_iq <- s*v_ip(old) + c*v_iq      (i = 0, 1, 2)
    lambda = the diagonal; the normal is the column of V at the smallest lambda (ties: the lowest index), not renormalised;
  - trace = (lambda_0 + lambda_1) + lambda_2; curvature = |lambda_min| / trace, 0 when trace == 0;
  - orientation towards the viewpoint: the normal is negated when ((vx - px)*nx + (vy - py)*ny) + (vz - pz)*nz < 0 in double (a dot
    product of exactly 0 keeps the sign); viewpoint None = DCREG_NORMAL_ORIENT_NONE leaves the solver's sign;
  - outputs per point in input order: normal (float)[3], curvature (float), eigenvalues (float)[3] ascending - the three lambda through the
    exchanges (0,1), (1,2), (0,1), each swapping when the second is smaller than the first;
  - n_out = the points that received a normal = n_finite - n_sparse.
"""
import numpy as np

UNBOUNDED = np.float32(3.0e38)
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))      # (p, q, r)
SWEEPS = 6


def d2_f32(a, b):
    """[len(a), len(b)] float32: the d2 of dcreg_knn between float32 points"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    d2 = dx * dx + dy * dy
    return d2 + dz * dz


def brute_neighbours(pts, k, chunk=512):
    """the k nearest points of every point of pts (itself a candidate) in (d2, index) order: (idx [m, k] int64, d2 [m, k] float32);
    slots beyond the cloud's size hold -1 / +inf"""
    m = len(pts)
    idx = np.full((m, k), -1, np.int64)
    d2 = np.full((m, k), np.inf, np.float32)
    take = min(k, m)
    for s in range(0, m, chunk):
        with np.errstate(over="ignore", invalid="ignore"):
            d = d2_f32(pts[s:s + chunk], pts)
        o = np.argsort(d, axis=1, kind="stable")[:, :take]         # stable: equal d2 in ascending index
        idx[s:s + chunk, :take] = o
        d2[s:s + chunk, :take] = np.take_along_axis(d, o, axis=1)
    return idx, d2


def bound_of(search_radius):
    if search_radius > 0.0:
        with np.errstate(over="ignore"):
            b = np.float32(np.float64(search_radius) * np.float64(search_radius))
        return b if b <= UNBOUNDED else UNBOUNDED
    return UNBOUNDED


def covariance(p, q):
    """p [m, 3] float32, q [m, k, 3] float32 (rank order) -> C [m, 6] float64 (xx xy xz yy yz zz)"""
    k = q.shape[1]
    e = q.astype(np.float64) - p.astype(np.float64)[:, None, :]
    s = e[:, 0, :].copy()
    for j in range(1, k):
        s = s + e[:, j, :]
    m = s / np.float64(k)
    d = e - m[:, None, :]
    out = np.empty((len(p), 6), np.float64)
    for c, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        acc = d[:, 0, a] * d[:, 0, b]
        for j in range(1, k):
            acc = acc + d[:, j, a] * d[:, j, b]
        out[:, c] = acc / np.float64(k)
    return out


def jacobi(C):
    """C [m, 6] -> (lam [m, 3], V [m, 3, 3] columns, off [m, 3] = a_01 a_02 a_12 after the sweeps)"""
    m = len(C)
    a = np.empty((m, 3, 3), np.float64)
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2], a[:, 1, 1], a[:, 1, 2], a[:, 2, 2] = (C[:, i] for i in range(6))
    a[:, 1, 0], a[:, 2, 0], a[:, 2, 1] = a[:, 0, 1], a[:, 0, 2], a[:, 1, 2]
    V = np.zeros((m, 3, 3), np.float64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q, r in PAIRS:
                app, aqq, apq = a[:, p, p].copy(), a[:, q, q].copy(), a[:, p, q].copy()
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(apq == 0.0, 0.0, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                a[:, p, p] = app - t * apq
                a[:, q, q] = aqq + t * apq
                a[:, p, q] = a[:, q, p] = 0.0
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                a[:, r, p] = a[:, p, r] = c * arp - s * arq
                a[:, r, q] = a[:, q, r] = s * arp + c * arq
                for i in range(3):
                    vp, vq = V[:, i, p].copy(), V[:, i, q].copy()
                    V[:, i, p] = c * vp - s * vq
                    V[:, i, q] = s * vp + c * vq
    lam = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1)
    off = np.stack([a[:, 0, 1], a[:, 0, 2], a[:, 1, 2]], axis=1)
    return lam, V, off


def smallest(lam):
    """index of the smallest lambda, ties to the lowest index"""
    i0 = np.zeros(len(lam), np.int64)
    rows = np.arange(len(lam))
    for j in (1, 2):
        i0 = np.where(lam[:, j] < lam[rows, i0], j, i0)
    return i0


def ascending(lam):
    """the exchanges (0,1), (1,2), (0,1), each swapping when the second is smaller than the first"""
    v = [lam[:, 0].copy(), lam[:, 1].copy(), lam[:, 2].copy()]
    for a, b in ((0, 1), (1, 2), (0, 1)):
        sw = v[b] < v[a]
        v[a], v[b] = np.where(sw, v[b], v[a]), np.where(sw, v[a], v[b])
    return np.stack(v, axis=1)


def normals_reference(xyz, k=5, search_radius=0.0, viewpoint=(0.0, 0.0, 0.0)):
    """-> dict normals [n, 3] float32, curvature [n] float32, eigenvalues [n, 3] float32, n_in, n_finite, n_sparse, n_out, and the doubles
    behind them for the rows that received a normal (`rows`): cov [m, 6], lam [m, 3], off [m, 3], normal64 [m, 3]"""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    p3 = xyz[:, :3]
    used = np.isfinite(p3).all(axis=1)
    ui = np.flatnonzero(used)
    pts = np.ascontiguousarray(p3[ui])
    m = len(pts)
    normals = np.full((n, 3), np.nan, np.float32)
    curv = np.full(n, np.nan, np.float32)
    eig = np.full((n, 3), np.nan, np.float32)
    out = dict(n_in=n, n_finite=m, n_sparse=m, n_out=0, rows=np.zeros(0, np.int64), cov=np.zeros((0, 6)), lam=np.zeros((0, 3)),
               off=np.zeros((0, 3)), normal64=np.zeros((0, 3)))
    if m >= k:
        idx, d2 = brute_neighbours(pts, k)
        ok = d2[:, k - 1] < bound_of(search_radius)
        sel = np.flatnonzero(ok)
        p = pts[sel]
        q = pts[idx[sel]]
        C = covariance(p, q)
        lam, V, off = jacobi(C)
        i0 = smallest(lam)
        rows = np.arange(len(sel))
        nrm = V[rows, :, i0]
        lmin = lam[rows, i0]
        trace = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
        with np.errstate(all="ignore"):
            cv = np.where(trace == 0.0, 0.0, np.abs(lmin) / trace)
        if viewpoint is not None:
            v = np.asarray(viewpoint, np.float64)
            pd = p.astype(np.float64)
            dot = ((v[0] - pd[:, 0]) * nrm[:, 0] + (v[1] - pd[:, 1]) * nrm[:, 1]) + (v[2] - pd[:, 2]) * nrm[:, 2]
            nrm = np.where((dot < 0.0)[:, None], -nrm, nrm)
        at = ui[sel]
        normals[at] = nrm.astype(np.float32)
        curv[at] = cv.astype(np.float32)
        eig[at] = ascending(lam).astype(np.float32)
        out.update(n_sparse=m - len(sel), n_out=len(sel), rows=at, cov=C, lam=lam, off=off, normal64=nrm)
    out.update(normals=normals, curvature=curv, eigenvalues=eig)
    return out
