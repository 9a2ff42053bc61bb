"""The consensus rule of include/dcreg.h ("consensus pose from a compatibility graph") in numpy, operation by operation: what the device's
records, mask, member lists, degrees, weights and counters are compared with, bit for bit.  The graph's quantities are bits and integers
(the counts come from a float32 matrix product, exact below 2^24: every count is below 2^15); the fit, the score and the refinement are
align_ref's, which states steps 5 and 7 of the RANSAC rule.  Nothing here needs a device."""
import math

import numpy as np

import align_ref as ar

IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def lengths(x):
    """l[u, v] = sqrt((g_x g_x + g_y g_y) + g_z g_z), g = x_u - x_v"""
    gx, gy, gz = (x[:, None, c] - x[None, :, c] for c in range(3))
    return np.sqrt((gx * gx + gy * gy) + gz * gz)


def compatibility(p, q, ia, ib, compat_distance, min_length):
    """step 2 -> C [M_u, M_u] bool; ia, ib: corr_a, corr_b of the used pairs"""
    la, lb = lengths(p), lengths(q)
    C = (ia[:, None] != ia[None, :]) & (ib[:, None] != ib[None, :]) & (la >= min_length) & (lb >= min_length) & (np.abs(la - lb) <= compat_distance)
    np.fill_diagonal(C, False)
    return C


def second_order(C):
    """step 3 -> S [M_u, M_u] int64, S(u, v) = C(u, v) * |{x: C(u, x) and C(v, x)}|"""
    f = C.astype(np.float32)
    return np.where(C, np.rint(f @ f).astype(np.int64), 0)


def members_of(C, S, s, consensus_size):
    """step 4 for seed s -> its members in ascending u (s among them)"""
    row = S[s]
    s_max = int(row.max())
    cand = np.flatnonzero(C[s] & (row >= 1) & (2 * row >= s_max))
    cand = cand[np.lexsort((cand, -row[cand]))][:consensus_size - 1]        # (S descending, v ascending)
    return np.sort(np.append(cand, s))


def fit(p, q, members):
    """step 5: the Horn fit of the RANSAC rule's step 7 over the members, once - align_ref.refine_step with every pair an inlier"""
    return ar.refine_step(IDENTITY, [0.0, 0.0, 0.0], p[members], q[members], math.inf)


def consensus(a, b, corr_a, corr_b, compat_distance=0.5, min_length=1.0, inlier_distance=0.5, n_seeds=64, consensus_size=16, n_best=1,
              refine_iterations=3):
    """The whole rule -> dict records (as Context.consensus_correspondences returns them), mask [n_pairs] uint8, info, members
    [n_best, consensus_size] int32, degree [n_pairs] uint32, weight [n_pairs] uint32"""
    n_pairs = len(corr_a)
    m_of_u, p, q = ar.used_pairs(a, b, corr_a, corr_b)
    m_u = int(p.shape[0])
    info = {"n_pairs": n_pairs, "n_used": m_u, "n_edges": 0, "max_degree": 0, "n_seeds": 0, "n_skipped": 0, "n_scored": 0, "n_returned": 0}
    out = {"records": [], "mask": np.zeros(n_pairs, np.uint8), "info": info, "members": np.full((n_best, consensus_size), -1, np.int32),
           "degree": np.zeros(n_pairs, np.uint32), "weight": np.zeros(n_pairs, np.uint32)}
    if m_u < 3:
        return out
    ia, ib = np.asarray(corr_a, np.int64)[m_of_u], np.asarray(corr_b, np.int64)[m_of_u]
    C = compatibility(p, q, ia, ib, float(compat_distance), float(min_length))
    deg = C.sum(axis=1).astype(np.int64)
    S = second_order(C)
    w = S.sum(axis=1)
    out["degree"][m_of_u], out["weight"][m_of_u] = deg, w
    seeds = np.lexsort((np.arange(m_u), -w))[:min(n_seeds, m_u)]             # (w descending, u ascending)
    info.update(n_edges=int(deg.sum()) // 2, max_degree=int(deg.max()), n_seeds=int(seeds.size))
    sets, R, t = [], [], []
    for r, s in enumerate(seeds.tolist()):
        mem = members_of(C, S, s, consensus_size)
        if mem.size < 3:
            info["n_skipped"] += 1
            continue
        Rs, ts = fit(p, q, mem)
        sets.append((r, s, mem))
        R.append(Rs)
        t.append(ts)
    info["n_scored"] = len(sets)
    if not sets:
        return out
    d, dd = float(inlier_distance), float(inlier_distance) * float(inlier_distance)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    count, cost = ar.scores(R, t, p, q, d)
    ranks = np.array([x[0] for x in sets])
    order = np.lexsort((ranks, cost, -count))[:n_best]                       # (count descending, cost ascending, r ascending)
    for k, o in enumerate(order.tolist()):
        r, s, mem = sets[o]
        Rk, tk = R[o].tolist(), t[o].tolist()
        refined = 0
        for _ in range(refine_iterations):
            step = ar.refine_step(Rk, tk, p, q, dd)
            if step is None:
                break
            Rk, tk = step
            refined += 1
        e2 = ar._e2_one(Rk, tk, p, q)
        inl = np.flatnonzero(e2 <= dd)
        total = 0.0
        for x in e2[inl].tolist():
            total = total + x
        T = np.eye(4)
        T[:3, :3] = np.asarray(Rk)
        T[:3, 3] = np.asarray(tk)
        out["records"].append({"T": T, "seed": int(m_of_u[s]), "seed_rank": r, "weight": int(w[s]), "n_members": int(mem.size),
                               "count": int(count[o]), "cost": int(cost[o]), "n_inliers": int(inl.size), "refined": refined,
                               "rmse": math.sqrt(total / float(inl.size)) if inl.size else 0.0})
        out["members"][k, :mem.size] = m_of_u[mem]
        if k == 0:
            out["mask"][m_of_u[inl]] = 1
    info["n_returned"] = len(out["records"])
    return out
