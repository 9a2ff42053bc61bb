"""numpy reference of dcreg_p2p_error (include/dcreg.h; calculatePointToPointError, utils.hpp:538-589): brute force, no index.

  - transform(T, pts): the aligned cloud as search.hpp body_to_global computes it - float64, element by element, in the fixed order
    ((R0*x + R1*y) + R2*z) + t, every operation rounded once, then rounded to float32.  No matrix product (a BLAS may fuse or reorder it).
    The forward pass's queries are then bitwise the device's, and so is every float d2 of that pass;
  - p2p_exact(aligned, target, thr): all pairwise distances between the float32 points.  The means are taken from float64 distances; the
    valid count and the squared sum follow the reference's rule on the float d2 that dcreg_knn computes ((dx*dx + dy*dy) + dz*dz, every
    operation rounded to float): a point is valid when (double)sqrtf(d2) < thr, strictly;
  - p2p_exact_rigid(src, T, target): the backward mean in exact arithmetic - float64 distances from each target point to T * p with T * p
    NOT rounded to float.  The backward pass's error bound (include/dcreg.h) is stated against it.
"""
import numpy as np


def transform(T, pts):
    """float32 [n, 3]: T * p as body_to_global rounds it"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(pts, np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty((len(p), 3), np.float32)
    for a in range(3):
        out[:, a] = (((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]).astype(np.float32)
    return out


def transform_exact(T, pts):
    """float64 [n, 3]: T * p, not rounded to float"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(pts, np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def rigid_inverse(T):
    """(R^T, -R^T t) as a 4x4: the inverse of a rigid motion"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def _d2_f32(a, b):
    """[len(a), len(b)] float32: the d2 of dcreg_knn between float32 points"""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    d2 = dx * dx + dy * dy
    return d2 + dz * dz


def nn_dist_f64(q, pts, chunk=256):
    """[len(q)] float64: the distance from every q to its nearest point of pts, all arithmetic in float64"""
    q = np.asarray(q, np.float64)
    pts = np.asarray(pts, np.float64)
    out = np.empty(len(q), np.float64)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - pts[None, :, :]
        out[s:s + chunk] = np.sqrt(np.min(np.einsum("ijk,ijk->ij", d, d), axis=1))
    return out


def nn_d2_f32(q, pts, chunk=256):
    """[len(q)] float32: the smallest float d2 (dcreg_knn's) from every q to the points of pts"""
    q = np.ascontiguousarray(q, np.float32)
    pts = np.ascontiguousarray(pts, np.float32)
    out = np.empty(len(q), np.float32)
    for s in range(0, len(q), chunk):
        out[s:s + chunk] = np.min(_d2_f32(q[s:s + chunk], pts), axis=1)
    return out


def p2p_exact(aligned_f32, target_f32, thr):
    """-> dict: fwd_mean / bwd_mean (float64 distances between the float32 points), fwd_mean_f32 (the mean of (double)sqrtf(d2) over the
    float d2: the terms the reference and the device sum), sum_sq and valid (the reference's rule), rmse, fitness, chamfer"""
    a = np.ascontiguousarray(aligned_f32, np.float32)
    t = np.ascontiguousarray(target_f32, np.float32)
    assert a.dtype == np.float32 and t.dtype == np.float32 and len(a) > 0 and len(t) > 0
    ns, nt = len(a), len(t)
    d2 = nn_d2_f32(a, t)
    fwd = float(np.mean(nn_dist_f64(a, t)))
    bwd = float(np.mean(nn_dist_f64(t, a)))
    dist = np.sqrt(d2).astype(np.float64)              # sqrtf (correctly rounded), widened
    base = dict(fwd_mean=fwd, bwd_mean=bwd, fwd_mean_f32=float(np.sum(dist) / ns), chamfer=(fwd + bwd) / 2.0, ns=ns, nt=nt, d2_f32=d2)
    return p2p_exact_thr(base, thr)


def p2p_exact_thr(base, thr):
    """a result of p2p_exact at another threshold: the means stay, the thresholded sums are taken again"""
    d2 = base["d2_f32"]
    ok = np.sqrt(d2).astype(np.float64) < float(thr)
    sum_sq = float(np.sum(d2[ok].astype(np.float64)))
    valid = int(np.count_nonzero(ok))
    return dict(base, thr=float(thr), sum_sq=sum_sq, valid=valid, rmse=float(np.sqrt(sum_sq / base["ns"])), fitness=valid / base["ns"])


def p2p_exact_rigid(src_f32, T, target_f32):
    """the backward mean in exact arithmetic: float64 distances from each target point to T * p, T * p not rounded to float"""
    return float(np.mean(nn_dist_f64(np.asarray(target_f32, np.float32), transform_exact(T, src_f32))))


def backward_bounds(src_f32, T, target_f32, mean_d):
    """(device bound, reference bound) on |backward mean - p2p_exact_rigid| (include/dcreg.h): sqrt(3) 2^-24 B + 2^-21 mean_d with B the
    largest absolute body-frame coordinate among T^-1 q and the source, and the same with G, the largest absolute map-frame coordinate
    among the target and T p"""
    src = np.asarray(src_f32, np.float32)
    tgt = np.asarray(target_f32, np.float32)
    B = max(float(np.max(np.abs(transform_exact(rigid_inverse(T), tgt)))), float(np.max(np.abs(src.astype(np.float64)))))
    G = max(float(np.max(np.abs(transform_exact(T, src)))), float(np.max(np.abs(tgt.astype(np.float64)))))
    c = np.sqrt(3.0) * 2.0 ** -24
    return c * B + 2.0 ** -21 * mean_d, c * G + 2.0 ** -21 * mean_d
