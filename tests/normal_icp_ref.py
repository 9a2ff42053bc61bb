"""numpy reference of the 1-NN point-to-plane linearisation (include/dcreg.h, "kept normals and the 1-NN point-to-plane linearisation"):
the rule, literally.

Of the parameters only search_radius (R), weight_slope, weight_min and use_weight_derivative are read.  Every operation rounds once.  For
each source point p (float32, widened to double):
  - q = R p + t: per coordinate ((R_a0*px + R_a1*py) + R_a2*pz) + t_a in double, stored as float32;
  - candidates are ranked by the total order (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in float32 (what dcreg_knn computes); j is the first
    map point in that order.  Flag 0 (radius gate) unless (double)d2 < R*R; a d2 equal to R*R stays out.  A point that passes counts in n_pt;
  - n = the kept normal of j (float32 {nx, ny, nz}), widened to double.  Flag 2 when a component is not finite: j has no normal;
  - e = (double)q - (double)t_j per coordinate; r = (nx*ex + ny*ey) + nz*ez;
  - s = 1 - weight_slope*|r|, and 0 when that is negative; ds = -weight_slope*(r > 0 ? 1 : -1) when use_weight_derivative and 0 < s < 1,
    else 0.  Flag 4 unless s > weight_min;
  - m = R^T n, component k = (R_0k*nx + R_1k*ny) + R_2k*nz; w = s + r*ds; A = w * [p x m, m]; b = -(s*r) in double.  Flag 1: the row is
    [A0..A5, b, r];
  - the sums: H = sum A A^T (21, upper triangle row-major), g = sum A b (6), sum_r2, sum_b2 = sum b^2 and n_eff over flag 1; n_pt over flag != 0.
The dump holds -1 / +inf for the nearest point of a flag-0 point, r and s for flags 1 and 4, the row for flag 1 and 0 everywhere else; the
normal as stored (widened) for every point that passed the radius gate.
"""
import math

import numpy as np

from normals_ref import d2_f32


def nearest(map_xyz, q, chunk=1024):
    """the first map point of every query in (d2, index) order -> (idx [m] int64, d2 [m] float32)"""
    m = len(q)
    idx = np.zeros(m, np.int64)
    d2 = np.zeros(m, np.float32)
    for s in range(0, m, chunk):
        with np.errstate(over="ignore", invalid="ignore"):
            d = d2_f32(q[s:s + chunk], map_xyz)
        o = np.argmin(d, axis=1)                       # the first occurrence of the minimum: the lowest index among equal d2
        idx[s:s + chunk] = o
        d2[s:s + chunk] = d[np.arange(len(o)), o]
    return idx, d2


def transform(R, t, src):
    """body_to_global: double arithmetic, every operation rounded once, float32 store"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    p = np.asarray(src, np.float32)[:, :3].astype(np.float64)
    q = np.empty((len(p), 3), np.float32)
    for a in range(3):
        q[:, a] = (((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a]).astype(np.float32)
    return q


def linearize(map_xyz, normals, src, T, search_radius, weight_slope=0.9, weight_min=0.1, use_weight_derivative=0, nn=None):
    """nn: nearest(map, transform(T, src)) when the caller has it already (it does not depend on the other parameters).  -> dict: nn_idx [n] int32, nn_d2 [n] float32, flag [n] uint8, normal [n, 3], r [n], s [n], row [n, 8] in source order, and the sums
    H_upper (21), g (6), sum_r2, sum_b2 (math.fsum over the rows: the exactly rounded sums), n_eff, n_pt"""
    map_xyz = np.ascontiguousarray(np.asarray(map_xyz, np.float32)[:, :3])
    normals = np.asarray(normals, np.float32)[:, :3]
    src = np.asarray(src, np.float32)
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    n = len(src)
    p = src[:, :3].astype(np.float64)
    q = transform(R, t, src)
    j, d2 = nn if nn is not None else nearest(map_xyz, q)
    r2 = np.float64(search_radius) * np.float64(search_radius)
    inside = d2.astype(np.float64) < r2
    nn_idx = np.where(inside, j, -1).astype(np.int32)
    nn_d2 = np.where(inside, d2, np.float32(np.inf)).astype(np.float32)
    flag = np.zeros(n, np.uint8)
    normal = np.zeros((n, 3))
    r_out, s_out, row = np.zeros(n), np.zeros(n), np.zeros((n, 8))
    nj = normals[j].astype(np.float64)
    normal[inside] = nj[inside]
    has = np.isfinite(normals[j]).all(axis=1)
    flag[inside & ~has] = 2
    sel = np.flatnonzero(inside & has)
    if len(sel):
        nx, ny, nz = nj[sel, 0], nj[sel, 1], nj[sel, 2]
        tj = map_xyz[j[sel]].astype(np.float64)
        e = q[sel].astype(np.float64) - tj
        r = (nx * e[:, 0] + ny * e[:, 1]) + nz * e[:, 2]
        s = 1.0 - np.float64(weight_slope) * np.abs(r)
        s = np.where(s < 0.0, 0.0, s)
        ds = np.zeros(len(sel))
        if use_weight_derivative:
            ds = np.where((s > 0.0) & (s < 1.0), -np.float64(weight_slope) * np.where(r > 0.0, 1.0, -1.0), 0.0)
        r_out[sel], s_out[sel] = r, s
        eff = s > np.float64(weight_min)
        flag[sel] = np.where(eff, 1, 4)
        m0 = (R[0, 0] * nx + R[1, 0] * ny) + R[2, 0] * nz
        m1 = (R[0, 1] * nx + R[1, 1] * ny) + R[2, 1] * nz
        m2 = (R[0, 2] * nx + R[1, 2] * ny) + R[2, 2] * nz
        w = s + r * ds
        px, py, pz = p[sel, 0], p[sel, 1], p[sel, 2]
        rows = np.stack([w * (py * m2 - pz * m1), w * (pz * m0 - px * m2), w * (px * m1 - py * m0), w * m0, w * m1, w * m2, -(s * r), r], axis=1)
        row[sel[eff]] = rows[eff]
    out = dict(nn_idx=nn_idx, nn_d2=nn_d2, flag=flag, normal=normal, r=r_out, s=s_out, row=row, nearest_d2=d2)    # (nearest_d2: ungated, not in the dump)
    out.update(sums_of(row, flag))
    return out


def sums_of(row, flag):
    """the 31 sums of the rows, each the exactly rounded sum (math.fsum) of its products"""
    H = []
    for a in range(6):
        for b in range(a, 6):
            H.append(math.fsum(row[:, a] * row[:, b]))
    g = [math.fsum(row[:, a] * row[:, 6]) for a in range(6)]
    return dict(H_upper=np.array(H), g=np.array(g), sum_r2=math.fsum(row[:, 7] * row[:, 7]), sum_b2=math.fsum(row[:, 6] * row[:, 6]),
                n_eff=int((flag == 1).sum()), n_pt=int((flag != 0).sum()))


def gate_margins(res, search_radius, weight_min=0.1):
    """how close any point of a linearisation comes to a gate: (min |d2 - R^2| over every point's nearest map point, min |s - weight_min| over
    the points that reached the weight) - counts compared across two engines' poses rely on both being far from 0"""
    d = np.abs(res["nearest_d2"].astype(np.float64) - search_radius * search_radius)
    w = np.abs(res["s"][(res["flag"] == 1) | (res["flag"] == 4)] - weight_min)
    return (float(d.min()) if len(d) else np.inf), (float(w.min()) if len(w) else np.inf)


def icp(map_xyz, normals, src, T0, cfg, method="NONE", max_iterations=None):
    """The reference engine: this linearisation + the host solver seam (dcreg_amd.api, no device) + dcreg_boxplus, the loop of dcreg_icp_run.
    -> (T, converged, records): one record per completed iteration with n_eff, n_pt, mask, dx, T (after the step), H_upper, g and the
    linearisation's gate margins"""
    from dcreg_amd import api
    det, hand = api.METHODS[method] if isinstance(method, str) else method
    T = np.asarray(T0, np.float64).reshape(4, 4).copy()
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    recs, converged = [], False
    for it in range(cfg.max_iterations if max_iterations is None else max_iterations):
        Tm = np.eye(4); Tm[:3, :3] = R; Tm[:3, 3] = t
        lin = linearize(map_xyz, normals, src, Tm, cfg.search_radius, use_weight_derivative=cfg.use_weight_derivative)
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
