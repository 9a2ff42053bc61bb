"""numpy reference of the outlier filters (include/dcreg.h, "outlier removal"): the rule, literally.

For one cloud of n points and the parameters mode, k, std_mul, radius, min_neighbors, search_radius:
  - a point is USED when x, y and z are all finite; the others are dropped and counted.  "Index" is the input index;
  - distances between used points are the float d2 that dcreg_knn computes ((dx*dx + dy*dy) + dz*dz, every operation rounded to float);
    neighbours are ranked by the total order (d2, index);
  - a point is never its own neighbour, by index and not by distance; exact duplicates are neighbours at distance 0.  With more than k
    duplicates of a point that point is not among its own k + 1 nearest: of the k + 1 nearest the entry with the point's own index is
    dropped if it is there, otherwise the last;
  - statistical: m_i = (float)((sum_j (double)sqrtf(d2_ij)) / k) over the k nearest others in ascending rank, summed left to right;
    search_radius > 0: only d2 < (float)(search_radius^2) counts, a used point with fewer than k such neighbours is sparse (dropped, counted,
    outside the statistics); search_radius = 0: unbounded, and a cloud with at most k used points has no statistics (all used points kept,
    scores and statistics NaN); mean = T(m) / n_stat, var = T((m - mean)^2) / (n_stat - 1) (0 for n_stat = 1), stddev = sqrt(var),
    threshold = mean + std_mul * stddev (a rounded multiply, a rounded add); kept iff (double)m_i <= threshold;
  - T(a): pad with +0.0 to the next power of two, then a[2j] + a[2j+1] until one value is left;
  - radius: kept iff at least min_neighbors other used points have d2 < (float)(radius^2); the score is the count capped at min_neighbors.
"""
import numpy as np


def tree_sum(a):
    """T(a) of the header"""
    b = np.asarray(a, dtype=np.float64).reshape(-1)
    p = 1
    while p < len(b):
        p *= 2
    b = np.concatenate([b, np.zeros(p - len(b))])
    while len(b) > 1:
        b = b[0::2] + b[1::2]
    return float(b[0]) if len(b) else 0.0


def d2_f32(a, b):
    """[len(a), len(b)] float32: the d2 of dcreg_knn between float32 points"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    d2 = dx * dx + dy * dy
    return d2 + dz * dz


def brute_neighbours(pts, kk, chunk=512):
    """the kk nearest points of every point of pts (itself included, as a search returns them) in (d2, index) order:
    (idx [m, kk] int64, d2 [m, kk] float32), slots beyond the cloud's size hold -1 / +inf"""
    m = len(pts)
    idx = np.full((m, kk), -1, np.int64)
    d2 = np.full((m, kk), np.inf, np.float32)
    take = min(kk, m)
    for s in range(0, m, chunk):
        d = d2_f32(pts[s:s + chunk], pts)
        o = np.argsort(d, axis=1, kind="stable")[:, :take]         # stable: equal d2 in ascending index
        idx[s:s + chunk, :take] = o
        d2[s:s + chunk, :take] = np.take_along_axis(d, o, axis=1)
    return idx, d2


def others(idx, d2, k):
    """the k nearest OTHERS from the k + 1 nearest: the entry with the point's own index is dropped if it is there, otherwise the last"""
    m = len(idx)
    own = idx == np.arange(m)[:, None]
    drop = np.where(own.any(axis=1), own.argmax(axis=1), k)
    keep = np.ones((m, k + 1), bool)
    keep[np.arange(m), drop] = False
    return d2[keep].reshape(m, k)


def outlier_reference(xyz, mode="statistical", k=8, std_mul=2.0, search_radius=0.0, radius=0.5, min_neighbors=3, neighbours=None):
    """-> dict mask [n] bool, scores [n] float32, kept [m, 3] float32, n_in, n_finite, n_sparse, n_out, mean, stddev, threshold.
    neighbours: None = brute force, or f(points [m, 3], kk) -> (idx, d2) of the kk nearest in (d2, index) order (the oracle's tree)"""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    p3 = xyz[:, :3]
    used = np.isfinite(p3).all(axis=1)
    ui = np.flatnonzero(used)
    pts = np.ascontiguousarray(p3[ui])
    m = len(pts)
    scores = np.full(n, np.nan, np.float32)
    mask = np.zeros(n, bool)
    out = dict(n_in=n, n_finite=m, n_sparse=0, mean=np.nan, stddev=np.nan, threshold=np.nan)
    if mode == "radius":
        r2 = np.float32(radius * radius)
        cnt = np.zeros(m, np.int64)
        for s in range(0, m, 512):
            cnt[s:s + 512] = (d2_f32(pts[s:s + 512], pts) < r2).sum(axis=1) - 1      # (a point's d2 to itself is 0 < r2)
        cnt = np.minimum(cnt, min_neighbors)
        scores[ui] = cnt.astype(np.float32)
        mask[ui] = cnt >= min_neighbors
    elif search_radius == 0.0 and m <= k:
        mask[ui] = True
    elif m > 0:
        idx, d2 = (neighbours or brute_neighbours)(pts, k + 1)
        d2 = others(np.asarray(idx, np.int64), np.asarray(d2, np.float32), k)
        sparse = np.zeros(m, bool)
        if search_radius > 0.0:
            sparse = ~(d2[:, k - 1] < np.float32(search_radius * search_radius))
        s = np.zeros(m, np.float64)
        with np.errstate(invalid="ignore"):
            root = np.sqrt(d2)                                   # float32 in, float32 out: the IEEE float square root
        for j in range(k):
            s += root[:, j].astype(np.float64)
        mi = (s / k).astype(np.float32)
        mi[sparse] = np.nan
        scores[ui] = mi
        stat = ~np.isnan(scores)
        n_stat = int(stat.sum())
        out["n_sparse"] = int(sparse.sum())
        if n_stat > 0:
            md = np.where(stat, scores.astype(np.float64), 0.0)
            mean = np.float64(tree_sum(md)) / np.float64(n_stat)
            dev = np.where(stat, scores.astype(np.float64) - mean, 0.0)
            var = np.float64(tree_sum(dev * dev)) / np.float64(n_stat - 1) if n_stat > 1 else np.float64(0.0)
            sd = np.sqrt(var)
            prod = np.float64(std_mul) * sd
            thr = mean + prod
            out.update(mean=float(mean), stddev=float(sd), threshold=float(thr))
            with np.errstate(invalid="ignore"):
                mask = stat & (scores.astype(np.float64) <= thr)
    out.update(mask=mask, scores=scores, kept=np.ascontiguousarray(p3[mask]), n_out=int(mask.sum()))
    return out
