"""numpy reference of the plane-to-plane (GICP) linearisation (include/dcreg.h, "kept source normals and the plane-to-plane (GICP)
linearisation"): the rule, literally.

eps = the option "gicp_epsilon", c = 1 - eps.  Of the parameters only search_radius (R) is read.  Every operation rounds once in double.
For each source point p (float32, widened to double):
  - transform, nearest point j and radius gate exactly as tests/normal_icp_ref.py: q stored as float32, j the first map point in
    (float32 d2, index) order, flag 0 unless (double)d2 < R*R;
  - n = the kept normal of j, flag 2 when a component is not finite; m = the kept normal of p, flag 3 when a component is not finite;
  - u = R m, component a = (R_a0*mx + R_a1*my) + R_a2*mz;  S_ab = d_ab - c*(n_a*n_b + u_a*u_b), d_ab = 2 on the diagonal and 0 off it;
  - l00 = sqrt(S00); l10 = S10/l00; l20 = S20/l00; l11 = sqrt(S11 - l10*l10); l21 = (S21 - l20*l10)/l11;
    l22 = sqrt((S22 - l20*l20) - l21*l21).  Flag 5 unless each of the three radicands is > 0;
  - w00 = 1/l00; w11 = 1/l11; w22 = 1/l22; w10 = -(l10*w00)*w11; w21 = -(l21*w11)*w22; w20 = -(l20*w00 + l21*w10)*w22; the pseudo-normals
    are the rows of W: a_0 = (w00, 0, 0), a_1 = (w10, w11, 0), a_2 = (w20, w21, w22), zeros multiplied and added like any other value;
  - e = (double)q - (double)t_j; for k = 0, 1, 2: r_k = (a_kx*ex + a_ky*ey) + a_kz*ez; m_k = R^T a_k, component i = (R_0i*a_kx +
    R_1i*a_ky) + R_2i*a_kz; row k = [p x m_k, m_k, -r_k, r_k].  Flag 1;
  - the sums over the three rows of every flag-1 point: H (21, upper triangle row-major), g (6), sum_r2 = sum_b2 = sum r_k^2; n_eff the
    flag-1 POINTS, n_pt the points with flag != 0.
The dump holds -1 / +inf for the nearest point of a flag-0 point, both normals as stored (widened) for every point that passed the radius
gate, and w, r, row for flag 1; 0 everywhere else.
"""
import math

import numpy as np

from normal_icp_ref import nearest, transform


def linearize(map_xyz, map_normals, src, src_normals, T, search_radius, eps=1e-3, nn=None):
    """-> dict: nn_idx [n] int32, nn_d2 [n] float32, flag [n] uint8, normal_map [n, 3], normal_src [n, 3], w [n, 3, 3], r [n, 3],
    row [n, 3, 8] in source order, and the sums H_upper (21), g (6), sum_r2, sum_b2 (math.fsum over the rows), n_eff, n_pt"""
    map_xyz = np.ascontiguousarray(np.asarray(map_xyz, np.float32)[:, :3])
    map_normals = np.asarray(map_normals, np.float32)[:, :3]
    src = np.asarray(src, np.float32)
    src_normals = np.asarray(src_normals, np.float32)[:, :3]
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    n = len(src)
    c = np.float64(1.0) - np.float64(eps)
    p = src[:, :3].astype(np.float64)
    q = transform(R, t, src)
    j, d2 = nn if nn is not None else nearest(map_xyz, q)
    r2 = np.float64(search_radius) * np.float64(search_radius)
    inside = d2.astype(np.float64) < r2
    nn_idx = np.where(inside, j, -1).astype(np.int32)
    nn_d2 = np.where(inside, d2, np.float32(np.inf)).astype(np.float32)
    flag = np.zeros(n, np.uint8)
    normal_map, normal_src = np.zeros((n, 3)), np.zeros((n, 3))
    w_out, r_out, row = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3, 8))
    nj, ms = map_normals[j].astype(np.float64), src_normals.astype(np.float64)
    normal_map[inside], normal_src[inside] = nj[inside], ms[inside]
    has_n, has_m = np.isfinite(map_normals[j]).all(axis=1), np.isfinite(src_normals).all(axis=1)
    flag[inside & ~has_n] = 2
    flag[inside & has_n & ~has_m] = 3
    sel = np.flatnonzero(inside & has_n & has_m)
    if len(sel):
        with np.errstate(all="ignore"):
            nv = [nj[sel, a] for a in range(3)]
            mv = [ms[sel, a] for a in range(3)]
            u = [(R[a, 0] * mv[0] + R[a, 1] * mv[1]) + R[a, 2] * mv[2] for a in range(3)]

            def S(a, b):
                return (2.0 if a == b else 0.0) - c * (nv[a] * nv[b] + u[a] * u[b])
            s00, s10, s11, s20, s21, s22 = S(0, 0), S(1, 0), S(1, 1), S(2, 0), S(2, 1), S(2, 2)
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
            zero = np.zeros(len(sel))
            W = np.stack([np.stack([w00, zero, zero], axis=1), np.stack([w10, w11, zero], axis=1), np.stack([w20, w21, w22], axis=1)], axis=1)
            tj = map_xyz[j[sel]].astype(np.float64)
            e = q[sel].astype(np.float64) - tj
            px, py, pz = p[sel, 0], p[sel, 1], p[sel, 2]
            rows, rs = [], []
            for k in range(3):
                ax, ay, az = W[:, k, 0], W[:, k, 1], W[:, k, 2]
                r = (ax * e[:, 0] + ay * e[:, 1]) + az * e[:, 2]
                m0 = (R[0, 0] * ax + R[1, 0] * ay) + R[2, 0] * az
                m1 = (R[0, 1] * ax + R[1, 1] * ay) + R[2, 1] * az
                m2 = (R[0, 2] * ax + R[1, 2] * ay) + R[2, 2] * az
                rows.append(np.stack([py * m2 - pz * m1, pz * m0 - px * m2, px * m1 - py * m0, m0, m1, m2, -r, r], axis=1))
                rs.append(r)
        flag[sel] = np.where(ok, 1, 5)
        good = sel[ok]
        w_out[good] = W[ok]
        r_out[good] = np.stack(rs, axis=1)[ok]
        row[good] = np.stack(rows, axis=1)[ok]
    out = dict(nn_idx=nn_idx, nn_d2=nn_d2, flag=flag, normal_map=normal_map, normal_src=normal_src, w=w_out, r=r_out, row=row,
               nearest_d2=d2)    # (nearest_d2: ungated, not in the dump)
    out.update(sums_of(row, flag))
    return out


def sums_of(row, flag):
    """the 31 sums over all 3 n rows, each the exactly rounded sum (math.fsum) of its products; the counts are of points"""
    rr = row.reshape(-1, 8)
    H = []
    for a in range(6):
        for b in range(a, 6):
            H.append(math.fsum(rr[:, a] * rr[:, b]))
    g = [math.fsum(rr[:, a] * rr[:, 6]) for a in range(6)]
    return dict(H_upper=np.array(H), g=np.array(g), sum_r2=math.fsum(rr[:, 7] * rr[:, 7]), sum_b2=math.fsum(rr[:, 6] * rr[:, 6]),
                n_eff=int((flag == 1).sum()), n_pt=int((flag != 0).sum()))


def gate_margin(res, search_radius):
    """min |d2 - R^2| over every point's nearest map point: counts compared across two engines' poses rely on it being far from 0"""
    d = np.abs(res["nearest_d2"].astype(np.float64) - search_radius * search_radius)
    return float(d.min()) if len(d) else np.inf


def icp(map_xyz, map_normals, src, src_normals, T0, cfg, method="NONE", eps=1e-3, max_iterations=None):
    """The reference engine: this linearisation + the host solver seam (dcreg_amd.api, no device) + dcreg_boxplus, the loop of
    dcreg_icp_run_gicp.  -> (T, converged, records): one record per completed iteration with n_eff, n_pt, mask, dx, T (after the
    step), H_upper, g and the linearisation"""
    from dcreg_amd import api
    det, hand = api.METHODS[method] if isinstance(method, str) else method
    T = np.asarray(T0, np.float64).reshape(4, 4).copy()
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    recs, converged = [], False
    for it in range(cfg.max_iterations if max_iterations is None else max_iterations):
        Tm = np.eye(4); Tm[:3, :3] = R; Tm[:3, 3] = t
        lin = linearize(map_xyz, map_normals, src, src_normals, Tm, cfg.search_radius, eps)
        if lin["n_eff"] < 10:
            break
        H = api.unpack_hessian(lin["H_upper"])
        an = api.analyze_degeneracy(H, det, hand, cfg)
        dx = api.solve_degenerate_system(H, lin["g"], hand, cfg, an)
        if not np.isfinite(dx).all():
            break
        R, t = api.boxplus(R, t, dx)
        Tn = np.eye(4); Tn[:3, :3] = np.asarray(R).reshape(3, 3); Tn[:3, 3] = t
        R, t = Tn[:3, :3].copy(), Tn[:3, 3].copy()
        recs.append(dict(n_eff=lin["n_eff"], n_pt=lin["n_pt"], mask=list(an.degenerate_mask), dx=np.array(dx), T=Tn, H_upper=lin["H_upper"],
                         g=lin["g"], lin=lin))
        dr = math.sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2])
        dt = math.sqrt(dx[3] * dx[3] + dx[4] * dx[4] + dx[5] * dx[5])
        if dr < cfg.CONVERGENCE_THRESH_ROT and dt < cfg.CONVERGENCE_THRESH_TRANS:
            converged = True
            break
    Tf = np.eye(4); Tf[:3, :3] = R; Tf[:3, 3] = t
    return Tf, converged, recs
