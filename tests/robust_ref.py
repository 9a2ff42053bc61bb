"""numpy reference of the robust kernels of the second and third engine (include/dcreg.h, "robust kernels"): the rule, literally, on top of
tests/normal_icp_ref.py and tests/gicp_ref.py.

kind 0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure; c the kernel's scale ("robust_scale" in metres for the second engine,
"gicp_robust_scale" in whitened units for the third); c2 = c * c formed once.  Every operation rounds once in double.
  factor(kind, u2):  Huber: u = sqrt(u2), k = 1 if u <= 1 else sqrt(1 / u);  Cauchy: k = 1 / sqrt(1 + u2);  Geman-McClure: k = 1 / (1 + u2).
Second engine: flags, r, s as without a kernel; for a flag-1 row [A0..A5, b, r]: u2 = (r * r) / c2, k = factor(kind, u2), the row becomes
[k*A0, .., k*A5, k*b, r].  Third engine: m2 = (r_0*r_0 + r_1*r_1) + r_2*r_2 over the point's three residuals, u2 = m2 / c2, one k per point;
slots 0..6 of its three rows are multiplied by k, slot 7 stays r_k.  kind 0 multiplies nothing: the bits of the plain references.
"""
import math

import numpy as np

import gicp_ref
import normal_icp_ref

KINDS = {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3}


def factor(kind, u2):
    """k = sqrt(rho'(r) / r) of the kernel at u2 = (r / c)^2, elementwise"""
    u2 = np.asarray(u2, np.float64)
    if kind == 0:
        return np.ones_like(u2)
    if kind == 1:
        u = np.sqrt(u2)
        with np.errstate(divide="ignore"):
            k = np.sqrt(np.float64(1.0) / u)
        return np.where(u <= 1.0, np.float64(1.0), k)
    if kind == 2:
        return np.float64(1.0) / np.sqrt(np.float64(1.0) + u2)
    if kind == 3:
        return np.float64(1.0) / (np.float64(1.0) + u2)
    raise ValueError("unknown kernel %r" % (kind,))


def point_factors_normals(res, kind, c):
    """k of every flag-1 point of a second-engine linearisation (in the order of np.flatnonzero(flag == 1)), and their u2"""
    c2 = np.float64(c) * np.float64(c)
    r = res["r"][res["flag"] == 1]
    u2 = (r * r) / c2
    return factor(kind, u2), u2


def point_factors_gicp(res, kind, c):
    c2 = np.float64(c) * np.float64(c)
    r = res["r"][res["flag"] == 1]
    m2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    u2 = m2 / c2
    return factor(kind, u2), u2


def linearize_normals(map_xyz, normals, src, T, search_radius, kind=0, c=0.1, weight_slope=0.9, weight_min=0.1, use_weight_derivative=0, nn=None):
    """normal_icp_ref.linearize with the kernel on its flag-1 rows; the sums are those of the scaled rows"""
    out = normal_icp_ref.linearize(map_xyz, normals, src, T, search_radius, weight_slope, weight_min, use_weight_derivative, nn)
    if kind == 0:
        return out
    eff = out["flag"] == 1
    k, _ = point_factors_normals(out, kind, c)
    row = out["row"]
    row[eff, :7] = k[:, None] * row[eff, :7]
    out.update(normal_icp_ref.sums_of(row, out["flag"]))
    return out


def linearize_gicp(map_xyz, map_normals, src, src_normals, T, search_radius, kind=0, c=1.0, eps=1e-3, nn=None):
    """gicp_ref.linearize with the kernel on the three rows of its flag-1 points; the sums are those of the scaled rows"""
    out = gicp_ref.linearize(map_xyz, map_normals, src, src_normals, T, search_radius, eps, nn)
    if kind == 0:
        return out
    eff = out["flag"] == 1
    k, _ = point_factors_gicp(out, kind, c)
    row = out["row"]
    row[eff, :, :7] = k[:, None, None] * row[eff, :, :7]
    out.update(gicp_ref.sums_of(row, out["flag"]))
    return out


def _icp(linearize, T0, cfg, method, max_iterations):
    """the loop of normal_icp_ref.icp / gicp_ref.icp around `linearize(T)`"""
    from dcreg_amd import api
    det, hand = api.METHODS[method] if isinstance(method, str) else method
    T = np.asarray(T0, np.float64).reshape(4, 4).copy()
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    recs, converged = [], False
    for it in range(cfg.max_iterations if max_iterations is None else max_iterations):
        Tm = np.eye(4); Tm[:3, :3] = R; Tm[:3, 3] = t
        lin = linearize(Tm)
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


def icp_normals(map_xyz, normals, src, T0, cfg, kind=0, c=0.1, method="NONE", max_iterations=None):
    """normal_icp_ref.icp with this module's linearisation -> (T, converged, records)"""
    return _icp(lambda T: linearize_normals(map_xyz, normals, src, T, cfg.search_radius, kind, c, use_weight_derivative=cfg.use_weight_derivative),
                T0, cfg, method, max_iterations)


def icp_gicp(map_xyz, map_normals, src, src_normals, T0, cfg, kind=0, c=1.0, method="NONE", eps=1e-3, max_iterations=None):
    """gicp_ref.icp with this module's linearisation -> (T, converged, records)"""
    return _icp(lambda T: linearize_gicp(map_xyz, map_normals, src, src_normals, T, cfg.search_radius, kind, c, eps), T0, cfg, method, max_iterations)
