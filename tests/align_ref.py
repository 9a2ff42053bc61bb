"""The alignment rule of include/dcreg.h ("pose from correspondences") in numpy, operation by operation: what the device's records, mask
and counters are compared with, bit for bit.  Steps 1 to 5 are vectorised over the hypotheses - numpy's float64 element-wise operations
round once each and fuse nothing -, step 7 is written with Python floats, which are IEEE doubles.  Nothing here needs a device."""
import math

import numpy as np

U64 = np.uint64
GOLDEN = U64(0x9E3779B97F4A7C15)


def splitmix(seed, k):
    """x(k) = mix(seed + k * 0x9E3779B97F4A7C15), k an array of uint64"""
    with np.errstate(over="ignore"):
        z = U64(seed) + np.asarray(k, U64) * GOLDEN
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def draws(seed, n_hypotheses, m_u):
    """u[h, j] = ((x(3 h + j + 1) >> 32) * M_u) >> 32"""
    h = np.arange(n_hypotheses, dtype=U64)
    k = U64(3) * h[:, None] + np.arange(1, 4, dtype=U64)[None, :]
    return (((splitmix(seed, k) >> U64(32)) * U64(m_u)) >> U64(32)).astype(np.int64)


def used_pairs(a, b, corr_a, corr_b):
    """step 1 -> (m_of_u, p [M_u, 3] float64, q [M_u, 3] float64)"""
    a, b = np.asarray(a), np.asarray(b)
    ca, cb = np.asarray(corr_a, np.int64), np.asarray(corr_b, np.int64)
    ok = (ca >= 0) & (ca < a.shape[0]) & (cb >= 0) & (cb < b.shape[0])
    m = np.flatnonzero(ok)
    p = a[ca[m], :3].astype(np.float64).reshape(-1, 3)
    q = b[cb[m], :3].astype(np.float64).reshape(-1, 3)
    fin = np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1)
    return m[fin], p[fin], q[fin]


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _triad(x0, x1, x2):
    """-> (ok, e1, e2, e3)"""
    u, v = x1 - x0, x2 - x0
    w = _cross(u, v)
    uu, vv, ww = _dot(u, u), _dot(v, v), _dot(w, w)
    ok = ~(ww <= 1e-4 * (uu * vv))
    with np.errstate(invalid="ignore", divide="ignore"):
        e1 = u / np.sqrt(uu)[:, None]
        e3 = w / np.sqrt(ww)[:, None]
    return ok, e1, _cross(e3, e1), e3


def hypotheses(p, q, seed, n_hypotheses, s):
    """steps 2 to 4 -> (u [H, 3], status [H]: 0 scored, 1 degenerate, 2 rejected, R [H, 3, 3], t [H, 3])"""
    u = draws(seed, n_hypotheses, p.shape[0])
    status = np.zeros(n_hypotheses, np.int64)
    equal = (u[:, 0] == u[:, 1]) | (u[:, 1] == u[:, 2]) | (u[:, 2] == u[:, 0])
    status[equal] = 1
    P, Q = p[u], q[u]                                         # [H, 3 pairs, 3]
    if s > 0.0:
        keep = np.ones(n_hypotheses, bool)
        for i, j in ((0, 1), (1, 2), (2, 0)):
            g, k = P[:, i] - P[:, j], Q[:, i] - Q[:, j]
            la, lb = np.sqrt(_dot(g, g)), np.sqrt(_dot(k, k))
            keep &= (la >= s * lb) & (lb >= s * la)
        status[(status == 0) & ~keep] = 2
    ok_p, e1, e2, e3 = _triad(P[:, 0], P[:, 1], P[:, 2])
    ok_q, f1, f2, f3 = _triad(Q[:, 0], Q[:, 1], Q[:, 2])
    status[(status == 0) & ~(ok_p & ok_q)] = 1
    with np.errstate(invalid="ignore"):
        R = (f1[:, :, None] * e1[:, None, :] + f2[:, :, None] * e2[:, None, :]) + f3[:, :, None] * e3[:, None, :]
        cp = ((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0
        cq = ((Q[:, 0] + Q[:, 1]) + Q[:, 2]) / 3.0
        t = cq - ((R[:, :, 0] * cp[:, None, 0] + R[:, :, 1] * cp[:, None, 1]) + R[:, :, 2] * cp[:, None, 2])
    return u, status, R, t


def residuals2(R, t, p, q):
    """step 5's e2 of every pair under every pose: R [S, 3, 3], t [S, 3] -> [S, M_u]"""
    r = []
    for c in range(3):
        r.append((((R[:, c, 0, None] * p[None, :, 0] + R[:, c, 1, None] * p[None, :, 1]) + R[:, c, 2, None] * p[None, :, 2]) + t[:, c, None])
                 - q[None, :, c])
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]


def scores(R, t, p, q, d):
    """step 5 -> (count [S] int64, cost [S] uint64)"""
    dd = d * d
    count, cost = np.zeros(R.shape[0], np.int64), np.zeros(R.shape[0], U64)
    step = max(1, (1 << 22) // max(p.shape[0], 1))
    for s0 in range(0, R.shape[0], step):
        e2 = residuals2(R[s0:s0 + step], t[s0:s0 + step], p, q)
        inl = e2 <= dd
        count[s0:s0 + step] = inl.sum(axis=1)
        term = np.floor((np.where(inl, e2, 0.0) / dd) * 1048576.0).astype(U64)
        cost[s0:s0 + step] = term.sum(axis=1, dtype=U64)
    return count, cost


def _jacobi4_rot(a, v, p, q):
    apq = a[p][q]
    t = 0.0
    if apq != 0.0:
        theta = (a[q][q] - a[p][p]) / (2.0 * apq)
        t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    tp = t * apq
    a[p][p] = a[p][p] - tp
    a[q][q] = a[q][q] + tp
    a[p][q] = a[q][p] = 0.0
    for r in range(4):
        if r == p or r == q:
            continue
        rp, rq = a[r][p], a[r][q]
        a[r][p] = a[p][r] = c * rp - s * rq
        a[r][q] = a[q][r] = s * rp + c * rq
    for k in range(4):
        x, y = v[k][p], v[k][q]
        v[k][p] = c * x - s * y
        v[k][q] = s * x + c * y


def _e2_one(R, t, p, q):
    return residuals2(np.asarray(R, np.float64).reshape(1, 3, 3), np.asarray(t, np.float64).reshape(1, 3), p, q)[0]


def refine_step(R, t, p, q, dd):
    """one step of 7 -> (R, t) as nested lists / a list, or None with fewer than three inliers"""
    inl = np.flatnonzero(_e2_one(R, t, p, q) <= dd)
    if inl.size < 3:
        return None
    n = float(inl.size)
    pl, ql = p[inl].tolist(), q[inl].tolist()
    cp, cq = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for pi, qi in zip(pl, ql):
        for c in range(3):
            cp[c] = cp[c] + pi[c]
            cq[c] = cq[c] + qi[c]
    cp = [x / n for x in cp]
    cq = [x / n for x in cq]
    S = [[0.0] * 3 for _ in range(3)]
    for pi, qi in zip(pl, ql):
        dp = [pi[c] - cp[c] for c in range(3)]
        dq = [qi[c] - cq[c] for c in range(3)]
        for a in range(3):
            for b in range(3):
                S[a][b] = S[a][b] + dp[a] * dq[b]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    N[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    N[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    N[0][1] = N[1][0] = S[1][2] - S[2][1]
    N[0][2] = N[2][0] = S[2][0] - S[0][2]
    N[0][3] = N[3][0] = S[0][1] - S[1][0]
    N[1][2] = N[2][1] = S[0][1] + S[1][0]
    N[1][3] = N[3][1] = S[2][0] + S[0][2]
    N[2][3] = N[3][2] = S[1][2] + S[2][1]
    V = [[1.0 if a == b else 0.0 for b in range(4)] for a in range(4)]
    for _ in range(8):
        for pp in range(3):
            for qq in range(pp + 1, 4):
                _jacobi4_rot(N, V, pp, qq)
    best = 0
    for k in range(1, 4):
        if N[k][k] > N[best][best]:
            best = k
    w, x, y, z = V[0][best], V[1][best], V[2][best], V[3][best]
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    nq = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nq, x / nq, y / nq, z / nq
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    t = [cq[r] - ((R[r][0] * cp[0] + R[r][1] * cp[1]) + R[r][2] * cp[2]) for r in range(3)]
    return R, t


def align(a, b, corr_a, corr_b, n_hypotheses=100000, seed=0, inlier_distance=0.5, edge_similarity=0.9, n_best=1, refine_iterations=3):
    """The whole rule -> dict records (as Context.align_correspondences returns them), mask [n_pairs] uint8, info"""
    n_pairs = len(corr_a)
    m_of_u, p, q = used_pairs(a, b, corr_a, corr_b)
    info = {"n_pairs": n_pairs, "n_used": int(p.shape[0]), "n_drawn": 0, "n_degenerate": 0, "n_rejected": 0, "n_scored": 0, "n_returned": 0}
    mask = np.zeros(n_pairs, np.uint8)
    if p.shape[0] < 3:
        return {"records": [], "mask": mask, "info": info}
    d, dd = float(inlier_distance), float(inlier_distance) * float(inlier_distance)
    u, status, R, t = hypotheses(p, q, seed, n_hypotheses, float(edge_similarity))
    hs = np.flatnonzero(status == 0)
    info.update(n_drawn=int(n_hypotheses), n_degenerate=int((status == 1).sum()), n_rejected=int((status == 2).sum()), n_scored=int(hs.size))
    count, cost = scores(R[hs], t[hs], p, q, d)
    order = np.lexsort((hs, cost, -count))[:n_best]           # (count descending, cost ascending, h ascending)
    records = []
    for k, o in enumerate(order):
        h = int(hs[o])
        Rk, tk = R[h].tolist(), t[h].tolist()
        refined = 0
        for _ in range(refine_iterations):
            step = refine_step(Rk, tk, p, q, dd)
            if step is None:
                break
            Rk, tk = step
            refined += 1
        e2 = _e2_one(Rk, tk, p, q)
        inl = np.flatnonzero(e2 <= dd)
        total = 0.0
        for x in e2[inl].tolist():
            total = total + x
        T = np.eye(4)
        T[:3, :3] = np.asarray(Rk)
        T[:3, 3] = np.asarray(tk)
        records.append({"T": T, "hypothesis": h, "pairs": tuple(int(m_of_u[x]) for x in u[h]), "count": int(count[o]), "cost": int(cost[o]),
                        "n_inliers": int(inl.size), "refined": refined, "rmse": math.sqrt(total / float(inl.size)) if inl.size else 0.0})
        if k == 0:
            mask[m_of_u[inl]] = 1
    info["n_returned"] = len(records)
    return {"records": records, "mask": mask, "info": info}
