"""numpy reference of the FPFH descriptors over a radius support (include/dcreg.h, "FPFH over a radius support"): the rule, literally.

Unchanged from the k-form (tests/fpfh_ref.py): the used points, dcreg_knn's float d2, the pair features in double and the bins
(pair_features and _bin are imported), the atan2 freedom and the "edge-near" flags.  Parameters: radius, finite and > 0, with
R2 = (float)(radius * radius) > 0 and < 3.0e38f; max_neighbors in 2 .. 65535.
  1. neighbours of a used point i: every used point j with d2_ij < R2 (strict), itself and exact duplicates included; m_i their number;
  2. m_i > max_neighbors: the point is CROWDED - no SPFH, EMPTY, counted in n_crowded and n_empty, reported with m = max_neighbors + 1
     and counts 0;
  3. for every neighbour with d2 > 0 the pair features and bins; pairs with f4 == 0 or vn == 0 are skipped; c_b(i): 33 integer counts;
  4. a point has an SPFH when 2 <= m_i <= max_neighbors and at least one pair was counted;
  5. q_b(i) = (c_b(i) << 16) // (m_i - 1);
  6. w_ij = min((uint64) floor(((double)R2 / (double)d2_ij) * 16384.0), 2^30);
  7. F_b(i) = sum over the neighbours j with d2_ij > 0 and an SPFH of w_ij * q_b(j), in uint64 (any order: integers);
  8. S_t = the sum of block t; out_b = (float)((double)F_b * (100.0 / (double)S_t)); a point with any S_t == 0 is EMPTY: NaN;
  9. n_in, n_used, n_empty, n_crowded, n_out, m_max, m_sum."""
import numpy as np

import normals_ref as nr
from fpfh_ref import DIM, EDGE_TOL, pair_features

W_ONE, W_CAP = 16384.0, 2 ** 30
MIN_CAP, MAX_CAP = 2, 65535


def r2_of(radius):
    """R2 of the rule, a float32"""
    with np.errstate(all="ignore"):
        return np.float32(np.float64(radius) * np.float64(radius))


def weights(R2, d2):
    """w of step 6 for float32 d2 > 0 -> uint64"""
    with np.errstate(all="ignore"):
        x = np.floor((np.float64(R2) / np.asarray(d2, np.float32).astype(np.float64)) * W_ONE)
    return np.minimum(x, float(W_CAP)).astype(np.uint64)


def quantise(counts, m):
    """q of step 5 for int counts [.., 33] and m [..] >= 2 -> uint64"""
    return (np.asarray(counts).astype(np.uint64) << np.uint64(16)) // (np.asarray(m).astype(np.uint64) - np.uint64(1))[..., None]


def normalise(F):
    """step 8 for uint64 F [.., 33] -> (float32 [.., 33] with NaN rows where a block's sum is 0, full [..] bool)"""
    F = np.asarray(F, np.uint64)
    S = np.stack([F[..., 11 * t:11 * t + 11].sum(axis=-1, dtype=np.uint64) for t in range(3)], axis=-1)
    full = (S > 0).all(axis=-1)
    with np.errstate(all="ignore"):
        out = (F.astype(np.float64) * np.repeat(100.0 / S.astype(np.float64), 11, axis=-1)).astype(np.float32)
    out[~full] = np.nan
    return out, full


def _add_rows(out, i, values):
    """out[i] += values, for ascending i (np.nonzero's row order): exact in any integer type, and without np.add.at's pace"""
    if len(i):
        rows, first = np.unique(i, return_index=True)
        out[rows] += np.add.reduceat(values, first, axis=0)


def _pairs(pts, R2, chunk=256):
    """the (i, j, d2) of step 1 over the used points, chunk by chunk"""
    for s in range(0, len(pts), chunk):
        D = nr.d2_f32(pts[s:s + chunk], pts)
        i, j = np.nonzero(D < R2)
        yield i + s, j, D[i, j]


def fpfh_radius_reference(xyz, normals, radius=1.0, max_neighbors=MAX_CAP):
    """-> dict fpfh [n, 33] float32 (NaN: unused or empty), counts [n, 33] int64, m [n] int64 (0: unused; max_neighbors + 1: crowded),
    has_spfh [n] bool, crowded [n] bool, edge_near [n] bool, excluded [n] bool (edge-near or with an edge-near neighbour), edge_pairs [n]
    int64, clamped [n] int64 (pairs with the clamped weight), n_in, n_used, n_empty, n_crowded, n_out, m_max, m_sum"""
    xyz = np.asarray(xyz, np.float32)
    normals = np.asarray(normals, np.float32)
    R2 = r2_of(radius)
    assert np.isfinite(radius) and radius > 0 and 0 < R2 < np.float32(3.0e38) and MIN_CAP <= max_neighbors <= MAX_CAP
    n = len(xyz)
    p3, n3 = xyz[:, :3], normals[:, :3]
    used = np.isfinite(p3).all(axis=1) & np.isfinite(n3).all(axis=1)
    ui = np.flatnonzero(used)
    pts, nrm = np.ascontiguousarray(p3[ui]), n3[ui].astype(np.float64)
    mu = len(pts)
    out = dict(fpfh=np.full((n, DIM), np.nan, np.float32), counts=np.zeros((n, DIM), np.int64), m=np.zeros(n, np.int64),
               has_spfh=np.zeros(n, bool), crowded=np.zeros(n, bool), edge_near=np.zeros(n, bool), excluded=np.zeros(n, bool),
               edge_pairs=np.zeros(n, np.int64), clamped=np.zeros(n, np.int64), n_in=n, n_used=mu, n_empty=0, n_crowded=0, n_out=0, m_max=0,
               m_sum=0)
    if mu == 0:
        return out
    P = pts.astype(np.float64)
    m = np.zeros(mu, np.int64)
    counts = np.zeros((mu, DIM), np.int64)
    edge_pairs = np.zeros(mu, np.int64)
    for i, j, d2 in _pairs(pts, R2):
        m += np.bincount(i, minlength=mu)
        far = d2 > 0
        i, j = i[far], j[far]
        ok, bins, t = pair_features(P[i], nrm[i], P[j], nrm[j])
        for blk in range(3):
            counts += np.bincount(i[ok] * DIM + (11 * blk + bins[ok, blk]), minlength=mu * DIM).reshape(mu, DIM)
        rt = np.rint(t)
        edge_pairs += np.bincount(i[ok & (np.abs(t - rt) < EDGE_TOL) & (rt > 0) & (rt < 11)], minlength=mu)
    crowded = m > max_neighbors
    counts[crowded] = 0
    edge_pairs[crowded] = 0
    edge = edge_pairs > 0
    has = (m >= 2) & ~crowded & (counts.sum(axis=1) > 0)
    q = np.zeros((mu, DIM), np.uint64)
    q[has] = quantise(counts[has], m[has])
    F = np.zeros((mu, DIM), np.uint64)
    near_edge = np.zeros(mu, bool)
    clamped = np.zeros(mu, np.int64)
    for i, j, d2 in _pairs(pts, R2):
        near_edge |= np.bincount(i[edge[j]], minlength=mu) > 0
        take = (d2 > 0) & has[j]
        i, j, w = i[take], j[take], weights(R2, d2[take])
        _add_rows(F, i, w[:, None] * q[j])
        clamped += np.bincount(i[w == W_CAP], minlength=mu)
    F[crowded] = 0
    desc, full = normalise(F)
    m_rep = np.minimum(m, max_neighbors + 1)
    out["fpfh"][ui] = desc
    out["counts"][ui] = counts
    out["m"][ui] = m_rep
    out["has_spfh"][ui] = has
    out["crowded"][ui] = crowded
    out["edge_near"][ui] = edge
    out["edge_pairs"][ui] = edge_pairs
    out["excluded"][ui] = edge | near_edge
    out["clamped"][ui] = clamped
    out.update(n_empty=int(mu - full.sum()), n_crowded=int(crowded.sum()), n_out=int(full.sum()), m_max=int(m_rep.max()), m_sum=int(m_rep.sum()))
    return out
