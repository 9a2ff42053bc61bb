"""numpy reference of the voxel-distribution linearisation with neighbour-voxel correspondences (include/dcreg.h, "voxels_neighbors"): the
rule of tests/voxels_ref.py with S correspondences per source point, literally.  Every operation rounds once in double.

Per source point p (mode, eps, kind, scale as tests/voxels_ref.py linearize):
  - q and v_a = floor((double)q_a / leaf) as there; the stencil is the list of offsets stencil(S): S = 1 the point's own voxel; S = 7 then
    +x -x +y -y +z -z; S = 27 the own voxel first, then the other 26 of the 3^3 block in ascending (dz, dy, dx);
  - correspondence j is the kept voxel at u = v + o_j, the sum formed in double; none when a component of u is not finite (a kept voxel
    lies inside the map's voxel box, so "outside the box" is "none" here without a test of its own);
  - mode 1: m and u = R m are the point's own, formed once; every found voxel of a point without a normal is flag 3;
  - S_ab, Cholesky, W, flag 5, e = (double)q - (double)mu_j, the three rows and - with a kernel on - one factor k_j from the
    correspondence's own squared Mahalanobis distance: per correspondence, from that voxel's record, exactly as voxels_ref;
  - the sums are over all rows of all flag-1 correspondences; n_eff counts the points with a flag-1 correspondence, n_pt the points with
    any correspondence.
The dump has an axis of length S behind the point axis - voxel_idx [n, S], flag [n, S], mean [n, S, 3], cov [n, S, 6], w [n, S, 3, 3],
r [n, S, 3], row [n, S, 3, 8], k [n, S] - except normal_src [n, 3], the point's own (zero for a point without any correspondence); with
S = 1 the axis is left out: the shapes, and every byte, of voxels_ref.linearize.
"""
import numpy as np

import gicp_ref
import robust_ref
import voxels_ref as vr
from normal_icp_ref import transform

SIZES = (1, 7, 27)


def stencil(S):
    """[S, 3] int64: the offsets (dx, dy, dz) in the rule's order"""
    if S == 1:
        return np.zeros((1, 3), np.int64)
    if S == 7:
        return np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)
    if S == 27:
        rest = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
        return np.array([(0, 0, 0)] + rest, np.int64)
    raise ValueError("neighbors: 1, 7 or 27 expected, got %r" % (S,))


def find_voxels(vmap, u):
    """the position of the kept voxel at each row of voxel coordinates u ([n, 3] doubles), -1 for none"""
    table = {tuple(int(x) for x in c): j for j, c in enumerate(vmap["coords"])}
    out = np.full(len(u), -1, np.int32)
    for i in range(len(u)):
        if np.isfinite(u[i]).all() and (np.abs(u[i]) < vr.LIMIT).all():
            out[i] = table.get((int(u[i, 0]), int(u[i, 1]), int(u[i, 2])), -1)
    return out


def linearize(vmap, src, T, mode=0, src_normals=None, eps=1e-3, kind=0, scale=1.0, neighbors=1):
    """-> dict as voxels_ref.linearize, with the axis of the S = neighbors correspondences behind the point axis when S > 1"""
    S = int(neighbors)
    off = stencil(S).astype(np.float64)
    src = np.asarray(src, np.float32)
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    n = len(src)
    c = np.float64(1.0) - np.float64(eps)
    p = src[:, :3].astype(np.float64)
    q = transform(R, t, src)
    with np.errstate(all="ignore"):
        v = vr.voxel_of(q, vmap["leaf"])
        vidx = np.stack([find_voxels(vmap, v + off[j]) for j in range(S)], axis=1)
    hit = vidx >= 0
    found = hit.any(axis=1)
    flag = np.zeros((n, S), np.uint8)
    mean, cov, normal_src = np.zeros((n, S, 3)), np.zeros((n, S, 6)), np.zeros((n, 3))
    w_out, r_out, row, kf = np.zeros((n, S, 3, 3)), np.zeros((n, S, 3)), np.zeros((n, S, 3, 8)), np.ones((n, S))
    has_m = np.ones(n, bool)
    if mode:
        ms = np.asarray(src_normals, np.float32)[:, :3]
        normal_src[found] = ms[found].astype(np.float64)
        has_m = np.isfinite(ms).all(axis=1)
        with np.errstate(all="ignore"):
            scov = vr.source_cov(R, ms.astype(np.float64), c)              # (the point's own: formed once, read by every found voxel)
    for j in range(S):
        h = hit[:, j]
        mean[h, j] = vmap["mean"][vidx[h, j]].astype(np.float64)
        cov[h, j] = vmap["cov"][vidx[h, j]].astype(np.float64)
        flag[h & ~has_m, j] = 3
        sel = np.flatnonzero(h & has_m)
        if not len(sel):
            continue
        Sm = cov[sel, j]
        if mode:
            with np.errstate(all="ignore"):
                Sm = Sm + scov[sel]
        W, ok = vr.whiten(Sm)
        e = q[sel].astype(np.float64) - mean[sel, j]
        with np.errstate(all="ignore"):
            rows, rs = vr.rows_of(R, p[sel], W, e)
        flag[sel, j] = np.where(ok, 1, 5)
        good = sel[ok]
        w_out[good, j], r_out[good, j], row[good, j] = W[ok], rs[ok], rows[ok]
        if kind:
            r = r_out[good, j]
            m2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            k = robust_ref.factor(kind, m2 / (np.float64(scale) * np.float64(scale)))
            kf[good, j] = k
            row[good, j, :, :7] = k[:, None, None] * row[good, j, :, :7]
    out = dict(voxel_idx=vidx, flag=flag, mean=mean, cov=cov, w=w_out, r=r_out, row=row, k=kf)
    if S == 1:
        out = {key: a[:, 0] for key, a in out.items()}
    out["normal_src"] = normal_src
    out.update(gicp_ref.sums_of(row, flag))
    out["n_eff"], out["n_pt"] = int((flag == 1).any(axis=1).sum()), int((flag != 0).any(axis=1).sum())     # points, not correspondences
    return out


def icp(vmap, src, T0, cfg, method="NONE", mode=0, src_normals=None, eps=1e-3, kind=0, scale=1.0, max_iterations=None, neighbors=1):
    """The reference engine at S = neighbors: voxels_ref.icp's loop around this linearisation -> (T, converged, records)"""
    return robust_ref._icp(lambda T: linearize(vmap, src, T, mode, src_normals, eps, kind, scale, neighbors), T0, cfg, method, max_iterations)
