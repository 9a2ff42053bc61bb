"""numpy reference of the FPFH descriptors and of the feature-space matching (include/dcreg.h, "FPFH descriptors and feature-space
matching"): the rules, literally.

Descriptors.  For a cloud of n points, one normal per point and the parameters k (3 .. 32, the point itself among the neighbours) and
search_radius (>= 0, 0 = unbounded):
  - a point is USED when its three coordinates and its three normal components are all finite; unused points are neither queries nor
    candidates and get NaN in all 33 outputs;
  - candidates are ranked by (d2, input index) with dcreg_knn's float d2; the neighbours are the first k used points with d2 < bound,
    bound = min((float)(search_radius^2), 3.0e38f) for search_radius > 0 and 3.0e38f for search_radius = 0.  A point with fewer than k
    candidates inside the bound keeps the m it has, 1 <= m <= k;
  - pair features, for the point p and each neighbour q with d2 > 0 in rank order, all in double, every operation rounded once, a dot
    product evaluated as (x + y) + z:
        d = q - p; f4 = sqrt(d.d); a pair with f4 == 0 is skipped
        a1 = (n_p.d) / f4; a2 = (n_q.d) / f4
        |a1| < |a2|: n1 = n_q, n2 = n_p, d = -d, phi = -a2; otherwise n1 = n_p, n2 = n_q, phi = a1
        v = d x n1; vn = sqrt(v.v); a pair with vn == 0 is skipped; v = v / vn per coordinate
        w = n1 x v; alpha = v.n2; theta = atan2(w.n2, n1.n2)
  - bins, each min(max(floor(.), 0), 10): t = 11 * ((theta + pi) / (2 * pi)), 11 * ((alpha + 1) * 0.5), 11 * ((phi + 1) * 0.5);
  - SPFH: c[33] integer counts - theta 0 .. 10, alpha 11 .. 21, phi 22 .. 32; s_b = (double)c_b * (100.0 / (double)(m - 1)).  A point with
    m < 2 or with no counted pair has no SPFH;
  - FPFH: F_b = sum_j (1.0 / (double)d2_j) * s_b(q_j) over the neighbours in rank order, skipping d2_j == 0 and every q_j without an SPFH;
    left to right, starting from the first term;
  - each block of 11 on its own: S = its sum, left to right; out_b = (float)(F_b * (100.0 / S)).  A point whose three S are not all > 0
    is EMPTY: NaN in all 33 outputs, counted in n_empty.
atan2 is the one operation that is not bit-reproducible between numpy and the device.  It matters only at an interior bin edge of theta,
so the reference also says per point whether one of its counted pairs has |t - round(t)| < 1e-9 with 0 < round(t) < 11 ("edge-near").

Matching.  Rows with a non-finite value are neither queries nor candidates (as queries: index -1, NaN);
D(i, j) = sum_c ((double)a_ic - (double)b_jc)^2 left to right, multiply and add rounded separately; candidates ranked by (D, j); best and
second-best, -1 / +inf where there is none; mutual[i] = the best row of a for b[idx_i] is i."""
import numpy as np

import normals_ref as nr

DIM = 33
EDGE_TOL = 1.0e-9


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _bin(x):
    return np.minimum(np.maximum(np.floor(x), 0.0), 10.0).astype(np.int64)


def pair_features(p, n_p, q, n_q):
    """double arrays [..., 3] -> (counted [...] bool apart from the d2 > 0 test, bins [..., 3] int64, t [...])"""
    with np.errstate(all="ignore"):
        d = q - p
        f4 = np.sqrt(_dot(d, d))
        a1 = _dot(n_p, d) / f4
        a2 = _dot(n_q, d) / f4
        sw = np.abs(a1) < np.abs(a2)
        n1 = np.where(sw[..., None], n_q, n_p)
        n2 = np.where(sw[..., None], n_p, n_q)
        d = np.where(sw[..., None], -d, d)
        phi = np.where(sw, -a2, a1)
        v = _cross(d, n1)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[..., None]
        w = _cross(n1, v)
        alpha = _dot(v, n2)
        theta = np.arctan2(_dot(w, n2), _dot(n1, n2))
        t = 11.0 * ((theta + np.pi) / (2.0 * np.pi))
        ok = (f4 != 0.0) & (vn != 0.0)
        tt = np.where(ok, t, 0.5)
        bins = np.stack([_bin(tt), _bin(np.where(ok, 11.0 * ((alpha + 1.0) * 0.5), 0.0)), _bin(np.where(ok, 11.0 * ((phi + 1.0) * 0.5), 0.0))], axis=-1)
    return ok, bins, tt


def fpfh_reference(xyz, normals, k=16, search_radius=0.0):
    """-> dict fpfh [n, 33] float32 (NaN: unused or empty), counts [n, 33] int64, m [n] int64 (0: unused), has_spfh [n] bool, edge_near [n]
    bool, excluded [n] bool (edge-near or with an edge-near neighbour), edge_pairs [n] int64 (counted pairs at an edge), n_in, n_used,
    n_empty, n_out, neighbours [n, k] int64 (input indices in rank order, -1: none)"""
    xyz = np.asarray(xyz, np.float32)
    normals = np.asarray(normals, np.float32)
    n = len(xyz)
    p3, n3 = xyz[:, :3], normals[:, :3]
    used = np.isfinite(p3).all(axis=1) & np.isfinite(n3).all(axis=1)
    ui = np.flatnonzero(used)
    pts, nrm = np.ascontiguousarray(p3[ui]), n3[ui].astype(np.float64)
    mu = len(pts)
    out = dict(fpfh=np.full((n, DIM), np.nan, np.float32), counts=np.zeros((n, DIM), np.int64), m=np.zeros(n, np.int64),
               has_spfh=np.zeros(n, bool), edge_near=np.zeros(n, bool), excluded=np.zeros(n, bool), edge_pairs=np.zeros(n, np.int64),
               n_in=n, n_used=mu, n_empty=0, n_out=0, neighbours=np.full((n, k), -1, np.int64))
    if mu == 0:
        return out
    idx, d2 = nr.brute_neighbours(pts, k)
    valid = (idx >= 0) & (d2 < nr.bound_of(search_radius))
    m = valid.sum(axis=1)
    ic = np.where(valid, idx, 0)
    P = pts.astype(np.float64)
    ok, bins, t = pair_features(P[:, None, :], nrm[:, None, :], P[ic], nrm[ic])
    counted = valid & (d2 > 0) & ok
    counts = np.zeros((mu, DIM), np.int64)
    rows = np.broadcast_to(np.arange(mu)[:, None], counted.shape)
    for blk in range(3):
        np.add.at(counts, (rows[counted], 11 * blk + bins[..., blk][counted]), 1)
    rt = np.rint(t)
    at_edge = counted & (np.abs(t - rt) < EDGE_TOL) & (rt > 0) & (rt < 11)
    edge = at_edge.any(axis=1)
    has = (m >= 2) & (counts.sum(axis=1) > 0)
    with np.errstate(all="ignore"):
        s = counts.astype(np.float64) * (100.0 / (m - 1).astype(np.float64))[:, None]
        F = np.full((mu, DIM), -0.0)              # (-0.0 + x = x bit for bit: the sums start with their first term)
        for j in range(k):
            take = valid[:, j] & (d2[:, j] > 0) & has[ic[:, j]]
            term = (1.0 / d2[:, j].astype(np.float64))[:, None] * s[ic[:, j]]
            F = np.where(take[:, None], F + term, F)
        S = []
        for blk in range(3):
            acc = F[:, 11 * blk].copy()
            for b in range(1, 11):
                acc = acc + F[:, 11 * blk + b]
            S.append(acc)
        full = (S[0] > 0) & (S[1] > 0) & (S[2] > 0)
        desc = np.concatenate([F[:, 11 * blk:11 * blk + 11] * (100.0 / S[blk])[:, None] for blk in range(3)], axis=1).astype(np.float32)
    desc[~full] = np.nan
    out["fpfh"][ui] = desc
    out["counts"][ui] = counts
    out["m"][ui] = m
    out["has_spfh"][ui] = has
    out["edge_near"][ui] = edge
    out["edge_pairs"][ui] = at_edge.sum(axis=1)
    out["excluded"][ui] = edge | (valid & edge[ic]).any(axis=1)
    out["neighbours"][ui] = np.where(valid, ui[ic], -1)
    out.update(n_empty=int(mu - full.sum()), n_out=int(full.sum()))
    return out


def distances(a, b):
    """[len(a), len(b)] float64: D of the rule between rows of 33 floats"""
    a = np.asarray(a, np.float32)[:, :DIM].astype(np.float64)
    b = np.asarray(b, np.float32)[:, :DIM].astype(np.float64)
    with np.errstate(all="ignore"):
        x = a[:, None, 0] - b[None, :, 0]
        D = x * x
        for c in range(1, DIM):
            x = a[:, None, c] - b[None, :, c]
            D = D + x * x
    return D


def _best_two(a, b, chunk=512):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    va, vb = np.isfinite(a[:, :DIM]).all(axis=1), np.isfinite(b[:, :DIM]).all(axis=1)
    na = len(a)
    idx = np.full((na, 2), -1, np.int32)
    d = np.full((na, 2), np.inf)
    jb = np.flatnonzero(vb)
    take = min(2, len(jb))
    if take:
        for s in range(0, na, chunk):
            D = distances(a[s:s + chunk], b[jb])
            o = np.argsort(D, axis=1, kind="stable")[:, :take]        # stable: equal D in ascending j
            idx[s:s + chunk, :take] = jb[o]
            d[s:s + chunk, :take] = np.take_along_axis(D, o, axis=1)
    idx[~va] = -1
    d[~va] = np.nan
    return idx, d, va, vb


def match_reference(a, b):
    """-> dict idx [n_a] int32, d [n_a] float64, idx2, d2, mutual [n_a] uint8, n_a_valid, n_b_valid, n_mutual"""
    idx, d, va, vb = _best_two(a, b)
    back = _best_two(b, a)[0][:, 0]
    i = np.arange(len(idx))
    mutual = (idx[:, 0] >= 0) & (back[np.maximum(idx[:, 0], 0)] == i) if len(back) else np.zeros(len(idx), bool)
    return dict(idx=idx[:, 0].copy(), d=d[:, 0].copy(), idx2=idx[:, 1].copy(), d2=d[:, 1].copy(), mutual=mutual.astype(np.uint8),
                n_a_valid=int(va.sum()), n_b_valid=int(vb.sum()), n_mutual=int(mutual.sum()))
