"""The SO(3) row of the first engine's parity instantiation (dcreg_amd/csrc/device/search.hpp row_of_plane_exact, option
"fast_plane_fit" = 0), written in numpy operation by operation: its dump holds normal, r, s and flag but no row, so the rows that its 31
sums are made of are rebuilt here from the device's OWN dumped normal, r and s, the source points, the pose and the parameters.

Per effective point (flag 1), every operation rounded once in double, no contraction:
  ds = -weight_slope * sign(r) when use_weight_derivative and 0 < s < 1, else 0;
  c = (float)(s * n) per component and ci = (float)(s * r): the float stores;  n' = (double)c / s: the normal recovered by division;
  m = R^T n', component k = (R_0k*n'x + R_1k*n'y) + R_2k*n'z;  w = s + r*ds;
  row = [w * (p x m), w * m, -(double)ci, r],  p x m = (py*m2 - pz*m1, pz*m0 - px*m2, px*m1 - py*m0), p = the float source point widened.
Every other point's row is zero.  The Euler row and the fast instantiation (fast_rcp instead of the division) are not covered.
"""
import numpy as np

import sums_check as sums


def rows_of_dump(src, R, dump, weight_slope, weight_min, use_weight_derivative):
    """src [n, >= 3] float32 in source order, R the pose's rotation (3 x 3), dump = Context.linearize(..., debug=True) -> row [n, 8]"""
    p = np.asarray(src, np.float32)[:, :3].astype(np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    flag = np.asarray(dump["flag"])
    row = np.zeros((len(p), 8))
    sel = np.flatnonzero(flag == 1)
    if len(sel) == 0:
        return row
    nrm = np.asarray(dump["normal"], np.float64)[sel]
    r, s = np.asarray(dump["r"], np.float64)[sel], np.asarray(dump["s"], np.float64)[sel]
    assert np.isfinite(nrm).all() and np.isfinite(r).all() and (s > np.float64(weight_min)).all() and (s <= 1.0).all()
    slope = np.float64(weight_slope)
    ds = np.zeros(len(sel))
    if use_weight_derivative:
        ds = np.where((s > 0.0) & (s < 1.0), -slope * np.where(r > 0.0, 1.0, -1.0), 0.0)
    cx, cy, cz = ((s * nrm[:, a]).astype(np.float32) for a in range(3))
    ci = (s * r).astype(np.float32)
    nx, ny, nz = cx.astype(np.float64) / s, cy.astype(np.float64) / s, cz.astype(np.float64) / s
    m0 = (R[0, 0] * nx + R[1, 0] * ny) + R[2, 0] * nz
    m1 = (R[0, 1] * nx + R[1, 1] * ny) + R[2, 1] * nz
    m2 = (R[0, 2] * nx + R[1, 2] * ny) + R[2, 2] * nz
    w = s + r * ds
    px, py, pz = p[sel, 0], p[sel, 1], p[sel, 2]
    row[sel] = np.stack([w * (py * m2 - pz * m1), w * (pz * m0 - px * m2), w * (px * m1 - py * m0), w * m0, w * m1, w * m2,
                         -(ci.astype(np.float64)), r], axis=1)
    return row


def assert_dump_sums_entrywise(c, src, T, prm, what="", slack=16):
    """One debug launch of dcreg_linearize on the context c (source src, option "fast_plane_fit" = 0) at the pose T: the plain launch gives
    the same 31 sums bit for bit, and every sum lies within the derived bound (tests/sums_check.py) of the exact sum over the rows rebuilt
    from the dump.  The rebuilt row is the device's arithmetic operation by operation; slack = 16 allows a few ulp per factor should a
    compiler reorder a commutative product.  -> (the dump, the largest error / bound)"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    got = c.linearize(T[:3, :3], T[:3, 3], prm, debug=True)
    plain = c.linearize(T[:3, :3], T[:3, 3], prm)
    for k in ("H_upper", "g", "sum_r2", "sum_b2", "n_eff", "n_pt"):
        assert np.array_equal(np.asarray(plain[k]), np.asarray(got[k])), (what, k)
    rows = rows_of_dump(src, T[:3, :3], got, prm.weight_slope, prm.weight_min, prm.use_weight_derivative)
    flag = got["flag"]
    worst = sums.assert_sums_entrywise(got, rows, int((flag == 1).sum()), int((flag != 0).sum()), what, slack)
    return got, worst
