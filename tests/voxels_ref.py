"""numpy reference of the kept voxel map and of the voxel-distribution linearisation (include/dcreg.h, "kept voxel distributions and the
voxel-distribution linearisation"): the two rules, literally.  Every operation rounds once in double.

The map (leaf, epsilon, min_points), its points in index order:
  - v_a = floor((double)p_a / leaf); a voxel's members are its points in ascending index, n their count; n < min_points: not kept (n_small);
  - s_a = the left-to-right sum of (double)p_a; mu_a = s_a / n; d_j = (double)p_j - mu; C_ab = (sum_j d_ja * d_jb) / n left to right for
    xx xy xz yy yz zz;
  - the six-sweep cyclic Jacobi of tests/normals_ref.py -> lambda_0..2, V; lmax = the largest lambda; not kept (n_degenerate) unless
    lmax > 0 and all three lambda are finite; l_k = lambda_k / lmax, epsilon when l_k < epsilon;
  - C'_ab = ((V_a0*l_0)*V_b0 + (V_a1*l_1)*V_b1) + (V_a2*l_2)*V_b2 for a >= b: xx = C'_00, xy = C'_10, xz = C'_20, yy = C'_11, yz = C'_21,
    zz = C'_22; the record is (float)mu, (float)C', n; the kept voxels in ascending (v_z, v_y, v_x) order.
One linearisation (mode = "voxels_source_cov", eps = "gicp_epsilon", c = 1 - eps), per source point p:
  - q as tests/normal_icp_ref.py transforms it (float32); v_a = floor((double)q_a / leaf); flag 0 when no kept voxel has these coordinates;
  - mode 1: m = the point's kept normal, flag 3 when a component is not finite; u = R m summed as tests/gicp_ref.py sums it;
  - S_ab = C'_ab (the record's floats, widened); mode 1: S_ab = C'_ab + (d_ab - c*(u_a*u_b)), d_ab = 1 on the diagonal and 0 off it;
  - Cholesky, W = L^-1, flag 5, the three rows and the sums exactly as tests/gicp_ref.py, with e = (double)q - (double)mu_f;
  - a robust kernel (kind, scale): one k per point as tests/robust_ref.py's third engine, slots 0..6 of the three rows times k.
"""
import math

import numpy as np

import gicp_ref
import normals_ref
import robust_ref
from normal_icp_ref import transform

LIMIT = 2.0 ** 62


def voxel_of(xyz, leaf):
    """[n, 3] float32 -> [n, 3] float64: floor((double)p / leaf)"""
    return np.floor(np.asarray(xyz, np.float32)[:, :3].astype(np.float64) / np.float64(leaf))


def voxel_map(xyz, leaf=1.0, epsilon=1e-3, min_points=6):
    """-> dict coords [V, 3] int64, count [V] int32, mean [V, 3] float32, cov [V, 6] float32 of the kept voxels in (z, y, x) order; the info
    counts n_points, n_voxels, n_small, n_degenerate, n_kept; and the doubles behind the records: mean64, cov64 (C'), cov_raw (C, before
    the eigen-solve), lam, l (clamped)"""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    n = len(xyz)
    v = voxel_of(xyz, leaf)
    assert np.isfinite(v).all() and (np.abs(v) < LIMIT).all()
    vi = v.astype(np.int64)
    order = np.lexsort((np.arange(n), vi[:, 0], vi[:, 1], vi[:, 2]))          # (z, y, x), then the index: a voxel's points ascend
    vs = vi[order]
    head = np.ones(n, bool)
    head[1:] = (vs[1:] != vs[:-1]).any(axis=1)
    start = np.flatnonzero(head)
    count = np.diff(np.append(start, n))
    n_vox = len(start)
    big = count >= min_points
    st, ct, co = start[big], count[big], vs[start[big]]
    p = xyz[order].astype(np.float64)
    m = len(st)
    s = p[st].copy()
    for j in range(1, int(ct.max()) if m else 0):
        sel = ct > j
        s[sel] = s[sel] + p[st[sel] + j]
    mu = s / ct[:, None].astype(np.float64)
    C = np.empty((m, 6))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        d0 = p[st] - mu
        acc = d0[:, a] * d0[:, b]
        for j in range(1, int(ct.max()) if m else 0):
            sel = ct > j
            dj = p[st[sel] + j] - mu[sel]
            acc[sel] = acc[sel] + dj[:, a] * dj[:, b]
        C[:, k] = acc / ct.astype(np.float64)
    lam, V, _ = normals_ref.jacobi(C)
    lmax = lam[:, 0].copy()
    for k in (1, 2):
        lmax = np.where(lam[:, k] > lmax, lam[:, k], lmax)
    ok = (lmax > 0.0) & np.isfinite(lam).all(axis=1)
    with np.errstate(all="ignore"):
        l = lam / lmax[:, None]
    l = np.where(l < np.float64(epsilon), np.float64(epsilon), l)
    Cp = np.empty((m, 6))
    for k, (a, b) in enumerate(((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))):
        Cp[:, k] = ((V[:, a, 0] * l[:, 0]) * V[:, b, 0] + (V[:, a, 1] * l[:, 1]) * V[:, b, 1]) + (V[:, a, 2] * l[:, 2]) * V[:, b, 2]
    return dict(coords=np.ascontiguousarray(co[ok]), count=ct[ok].astype(np.int32), mean=mu[ok].astype(np.float32), cov=Cp[ok].astype(np.float32),
                n_points=n, n_voxels=n_vox, n_small=int((~big).sum()), n_degenerate=int((~ok).sum()), n_kept=int(ok.sum()),
                mean64=mu[ok], cov64=Cp[ok], cov_raw=C[ok], lam=lam[ok], l=l[ok], V=V[ok], leaf=float(leaf))


def find(vmap, q):
    """the position of the kept voxel that holds each float32 point of q, -1 for none"""
    table = {tuple(int(x) for x in c): j for j, c in enumerate(vmap["coords"])}
    with np.errstate(all="ignore"):
        v = voxel_of(q, vmap["leaf"])
    out = np.full(len(q), -1, np.int32)
    for i in range(len(q)):
        if np.isfinite(v[i]).all() and (np.abs(v[i]) < LIMIT).all():
            out[i] = table.get((int(v[i, 0]), int(v[i, 1]), int(v[i, 2])), -1)
    return out


def whiten(S):
    """S [m, 6] (s00 s10 s20 s11 s21 s22) -> (W [m, 3, 3], ok [m]): the third engine's Cholesky factor and W = L^-1, in its order"""
    s00, s10, s20, s11, s21, s22 = (S[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        l00 = np.sqrt(s00)
        l10 = s10 / l00
        l20 = s20 / l00
        d11 = s11 - l10 * l10
        l11 = np.sqrt(d11)
        l21 = (s21 - l20 * l10) / l11
        d22 = (s22 - l20 * l20) - l21 * l21
        l22 = np.sqrt(d22)
        ok = (s00 > 0.0) & (d11 > 0.0) & (d22 > 0.0)
        w00, w11, w22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
        w10 = -(l10 * w00) * w11
        w21 = -(l21 * w11) * w22
        w20 = -(l20 * w00 + l21 * w10) * w22
    zero = np.zeros(len(S))
    W = np.stack([np.stack([w00, zero, zero], axis=1), np.stack([w10, w11, zero], axis=1), np.stack([w20, w21, w22], axis=1)], axis=1)
    return W, ok


def rows_of(R, p, W, e):
    """the three rows [m, 3, 8] and residuals [m, 3] of tests/gicp_ref.py from W, e = q - mu and the source points p (doubles)"""
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    rows, rs = [], []
    for k in range(3):
        ax, ay, az = W[:, k, 0], W[:, k, 1], W[:, k, 2]
        r = (ax * e[:, 0] + ay * e[:, 1]) + az * e[:, 2]
        m0 = (R[0, 0] * ax + R[1, 0] * ay) + R[2, 0] * az
        m1 = (R[0, 1] * ax + R[1, 1] * ay) + R[2, 1] * az
        m2 = (R[0, 2] * ax + R[1, 2] * ay) + R[2, 2] * az
        rows.append(np.stack([py * m2 - pz * m1, pz * m0 - px * m2, px * m1 - py * m0, m0, m1, m2, -r, r], axis=1))
        rs.append(r)
    return np.stack(rows, axis=1), np.stack(rs, axis=1)


def source_cov(R, m, c):
    """the six lower-triangle entries d_ab - c*(u_a*u_b) of the rotated source plane covariance, u = R m"""
    u = [(R[a, 0] * m[:, 0] + R[a, 1] * m[:, 1]) + R[a, 2] * m[:, 2] for a in range(3)]
    return np.stack([(1.0 if a == b else 0.0) - c * (u[a] * u[b]) for a, b in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))], axis=1)


def linearize(vmap, src, T, mode=0, src_normals=None, eps=1e-3, kind=0, scale=1.0):
    """-> dict: voxel_idx [n] int32, flag [n] uint8, mean [n, 3], cov [n, 6], normal_src [n, 3], w [n, 3, 3], r [n, 3], row [n, 3, 8] in
    source order, k [n] (the robust factor, 1 where none), and the sums as tests/gicp_ref.py forms them"""
    src = np.asarray(src, np.float32)
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    n = len(src)
    c = np.float64(1.0) - np.float64(eps)
    p = src[:, :3].astype(np.float64)
    q = transform(R, t, src)
    vidx = find(vmap, q)
    hit = vidx >= 0
    flag = np.zeros(n, np.uint8)
    mean, cov, normal_src = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, 3))
    w_out, r_out, row, kf = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 8)), np.ones(n)
    mean[hit] = vmap["mean"][vidx[hit]].astype(np.float64)
    cov[hit] = vmap["cov"][vidx[hit]].astype(np.float64)
    go = hit.copy()
    if mode:
        ms = np.asarray(src_normals, np.float32)[:, :3]
        normal_src[hit] = ms[hit].astype(np.float64)
        has_m = np.isfinite(ms).all(axis=1)
        flag[hit & ~has_m] = 3
        go = hit & has_m
    sel = np.flatnonzero(go)
    if len(sel):
        S = cov[sel]
        if mode:
            with np.errstate(all="ignore"):
                S = S + source_cov(R, normal_src[sel], c)
        W, ok = whiten(S)
        e = q[sel].astype(np.float64) - mean[sel]
        with np.errstate(all="ignore"):
            rows, rs = rows_of(R, p[sel], W, e)
        flag[sel] = np.where(ok, 1, 5)
        good = sel[ok]
        w_out[good], r_out[good], row[good] = W[ok], rs[ok], rows[ok]
        if kind:
            r = r_out[good]
            m2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            k = robust_ref.factor(kind, m2 / (np.float64(scale) * np.float64(scale)))
            kf[good] = k
            row[good, :, :7] = k[:, None, None] * row[good, :, :7]
    out = dict(voxel_idx=vidx, flag=flag, mean=mean, cov=cov, normal_src=normal_src, w=w_out, r=r_out, row=row, k=kf)
    out.update(gicp_ref.sums_of(row, flag))
    return out


def icp(vmap, src, T0, cfg, method="NONE", mode=0, src_normals=None, eps=1e-3, kind=0, scale=1.0, max_iterations=None):
    """The reference engine: this linearisation + the host solver seam (dcreg_amd.api, no device) + dcreg_boxplus, the loop of
    dcreg_icp_run_voxels -> (T, converged, records) as tests/gicp_ref.py's"""
    return robust_ref._icp(lambda T: linearize(vmap, src, T, mode, src_normals, eps, kind, scale), T0, cfg, method, max_iterations)


def pose_error(T, GT):
    """(translation error in metres, rotation error in degrees) of T against GT"""
    D = np.linalg.inv(np.asarray(GT, np.float64)) @ np.asarray(T, np.float64)
    ang = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))))
    return float(np.linalg.norm(D[:3, 3])), ang
