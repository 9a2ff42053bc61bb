"""What the solver-seam edge tests assert of an analysis record and a step, shared by the CPU tests (test_host_solver_edges.py) and the GPU
test of degenerate runs (test_gpu_degenerate_runs.py).

  consistent(rec, cfg, det, hand)   the record agrees with itself: mask and flag are the rule applied - in doubles, bit for bit - to the
                                    record's own spectra and condition numbers, whatever rounding did to a zero eigenvalue
  identity(...)                     the step is its handling's formula evaluated on the record's own mask and eigenvectors
  exact_fields / ratios(...)        the record and the step against the 50-digit reference: masks and counts exactly, the rest as the
                                    ratio of its error to its bound without the constant (decidable cells)

Tolerance (tol_c).  The bound on a step is C * 2^-52 * kappa * |x|, kappa the 50-digit condition number of the system the handling
actually solves (after regularisation, truncation or projection - there also ||H|| over the gap between kept and dropped eigenvalues, the
condition of the projector -, for PCG that of the preconditioned system times that of the blocks whose inverse builds the preconditioner);
on a spectrum C * 2^-52 * ||H|| absolute (Schur spectra: times the condition of the inverted blocks).  C was measured as the largest ratio
of error to that bound of the ORACLE (cyclic Jacobi, its own QR and LU) against the reference over the decidable cells of
solver_scenes.SYSTEMS: MEASURED_C below, per kind of quantity; the library (tred2 / tql2) is held to 8 x that.  Two correct implementations differ by small
multiples; a wrong pivot or a missed sweep by orders of magnitude."""
import types

import numpy as np

import solver_ref as sr
import solver_scenes as sc

# measured: test_host_solver_edges.test_oracle_measures_the_tolerance prints the figures.  The largest ratio overall, C = 196, is a PCG step;
# held to that alone the spectra and the direct steps would go almost unchecked, so each kind is pinned to its own measurement (no more than
# the overall C, each rounded up to the next integer) and the library held to 8 x it
MEASURED_C = {"spectrum": 5.0, "step": 2.0, "step (PCG)": 197.0}       # measured 4.8, 1.16, 196.4
MARGIN = 8.0
U = 2.0 ** -52


def kind(what):
    return what if what.startswith("step") else "spectrum"


def tol_c(what):
    return MARGIN * MEASURED_C[kind(what)]


def ref_config(kappa_target, always_schur, thres_cond=sc.THRES_COND, thres_eig=sc.THRES_EIG, gamma=0.01, pcg_tol=1e-6, pcg_max=10):
    return types.SimpleNamespace(DEGENERACY_THRES_COND=thres_cond, DEGENERACY_THRES_EIG=thres_eig, KAPPA_TARGET=kappa_target,
                                 PCG_TOLERANCE=pcg_tol, PCG_MAX_ITER=pcg_max, STD_REG_GAMMA=gamma, always_compute_schur=always_schur)


_REF = {}


def reference(name, H, g, det, hand, cfg_key):
    """the reference of a cell, computed once per process"""
    key = (name, det, hand, cfg_key)
    if key not in _REF:
        _REF[key] = sr.reference(H, g, det, hand, ref_config(*cfg_key))
    return _REF[key]


def cells():
    for name, family, H, g in sc.SYSTEMS:
        for ck in sc.CONFIGS:
            for det in sr.DETECTIONS:
                for hand in sr.HANDLINGS:
                    yield name, family, H, g, ck, det, hand


def record(an):
    """an analysis record of the library (api.Analysis) or of the oracle (pyoracle.Analysis) under common names"""
    lib = hasattr(an, "isDegenerate")
    f = lambda a, shape=None: np.array(a[:]).reshape(shape) if shape else np.array(a[:])
    r = types.SimpleNamespace(
        deg=int(an.isDegenerate if lib else an.is_degenerate), mask=[int(v) for v in (an.degenerate_mask if lib else an.mask)],
        ev=f(an.eigenvalues_full), V=f(an.eigenvectors_full, (6, 6)), sv=f(an.singular_values),
        schur_rot=f(an.lambda_schur_rot), schur_trans=f(an.lambda_schur_trans), sub_rot=f(an.lambda_sub_rot), sub_trans=f(an.lambda_sub_trans),
        Vr=f(an.schur_V_rot, (3, 3)), Vt=f(an.schur_V_trans, (3, 3)), P=f(an.P_preconditioner, (6, 6)), pcg=int(an.pcg_iterations), lib=lib)
    for k in ("cond_schur_rot", "cond_schur_trans", "cond_diag_rot", "cond_diag_trans", "cond_full", "cond_full_sub_rot", "cond_full_sub_trans"):
        setattr(r, k, float(getattr(an, k)))
    if lib:
        r.Ar, r.At = f(an.aligned_V_rot, (3, 3)), f(an.aligned_V_trans, (3, 3))
        r.ir, r.it = [int(v) for v in an.rot_indices], [int(v) for v in an.trans_indices]
    return r


def _same(a, b):
    """two doubles, bit for bit up to the sign of zero and the payload of NaN"""
    return (np.isnan(a) and np.isnan(b)) or a == b


def _clusters(w, rel=1e-9):
    mx = max(np.max(np.abs(w)), 1e-300)
    groups, cur = [], [0]
    for i in range(1, len(w)):
        if abs(w[i] - w[i - 1]) <= rel * mx:
            cur.append(i)
        else:
            groups.append(cur)
            cur = [i]
    return groups + [cur]


def rule_mask(r, det, thres_cond, thres_eig):
    """the detection's rule in doubles on the record's own numbers -> (flag, mask)"""
    F = np.float64
    mask = [0] * 6
    with np.errstate(all="ignore"):
        if det == "SCHUR_CONDITION_NUMBER":
            if np.isfinite(r.cond_schur_rot) and np.isfinite(r.cond_schur_trans):
                for b, lam in enumerate((r.schur_rot, r.schur_trans)):
                    for i in range(3):
                        mask[3 * b + i] = int(F(np.max(lam)) / F(max(lam[i], 1e-12)) > thres_cond)
                return int(any(mask)), mask
            return 1, [1] * 6
        if det == "FULL_EVD_MIN_EIGENVALUE":
            mask = [int(v < thres_eig) for v in r.ev]
            return int(any(mask)), mask
        if det == "EVD_SUB_CONDITION":
            if r.cond_diag_trans > thres_cond:
                mask[3:] = [1, 1, 1]
            if r.cond_diag_rot > thres_cond:
                mask[:3] = [1, 1, 1]
            return int(any(mask)), mask
        if det == "FULL_SVD_CONDITION":
            deg = int(r.cond_full > thres_cond)
            if deg:
                mask = [int(F(np.max(r.ev)) / F(v) > thres_cond) for v in r.ev]
            return deg, mask
    return 0, mask


def consistent(r, cfg, det, hand, where=""):
    """(b) of the edge tests; cfg: anything with the configuration's names (the library's dcreg_config or ref_config)"""
    F = np.float64
    thc, the = float(cfg.DEGENERACY_THRES_COND), float(cfg.DEGENERACY_THRES_EIG)
    deg, mask = rule_mask(r, det, thc, the)
    assert (r.deg, r.mask) == (deg, mask), (where, "mask is not the rule on the record's own numbers", r.deg, r.mask, deg, mask)
    with np.errstate(all="ignore"):
        # the condition numbers are the rule on the record's own spectra
        assert np.array_equal(r.sv, np.sort(np.abs(r.ev))[::-1]), (where, "singular values")
        assert _same(r.cond_full, F(r.sv[0]) / F(r.sv[5]) if r.sv[5] > 1e-12 else np.inf), (where, "cond_full")
        assert _same(r.cond_full_sub_trans, abs(r.ev[2]) / max(abs(r.ev[0]), 1e-12)), (where, "cond_full_sub_trans")
        assert _same(r.cond_full_sub_rot, abs(r.ev[5]) / max(abs(r.ev[3]), 1e-12)), (where, "cond_full_sub_rot")
        for lam, c, name in ((r.sub_rot, r.cond_diag_rot, "cond_diag_rot"), (r.sub_trans, r.cond_diag_trans, "cond_diag_trans")):
            assert _same(c, np.nan if np.isnan(lam).any() else np.max(lam) / max(np.min(lam), 1e-12)), (where, name)
        for lam, c, name in ((r.schur_rot, r.cond_schur_rot, "cond_schur_rot"), (r.schur_trans, r.cond_schur_trans, "cond_schur_trans")):
            if not np.isnan(lam).any():
                assert _same(c, np.max(lam) / max(np.min(lam), 1e-12)), (where, name)
            else:
                assert np.isnan(c) or c == np.inf, (where, name)
    assert np.all(np.diff(r.ev) >= 0), (where, "eigenvalues ascending")
    eye6, eye3 = np.eye(6), np.eye(3)
    assert np.max(np.abs(r.V.T @ r.V - eye6)) <= 1e-12, (where, "eigenvectors_full orthonormal")
    assert np.max(np.abs(r.Vr.T @ r.Vr - eye3)) <= 1e-12 and np.max(np.abs(r.Vt.T @ r.Vt - eye3)) <= 1e-12, (where, "schur_V orthonormal")
    # the preconditioner: symmetric, block diagonal, spectrum 1 / max(l, l_max / KAPPA_TARGET) per block (identity without Schur spectra)
    assert np.array_equal(r.P[:3, 3:], np.zeros((3, 3))) and np.array_equal(r.P[3:, :3], np.zeros((3, 3))), (where, "P block diagonal")
    assert np.max(np.abs(r.P - r.P.T)) <= 1e-14 * np.max(np.abs(r.P)), (where, "P symmetric")
    for b, lam in enumerate((r.schur_rot, r.schur_trans)):
        Pb = r.P[3 * b:3 * b + 3, 3 * b:3 * b + 3]
        if np.isnan(lam).any():
            assert np.array_equal(Pb, eye3), (where, "P identity without Schur spectra")
        else:
            want = np.sort(1.0 / np.maximum(lam, np.max(lam) / float(cfg.KAPPA_TARGET)))
            got = np.linalg.eigvalsh(0.5 * (Pb + Pb.T))
            assert np.allclose(got, want, rtol=1e-12, atol=0.0), (where, "P spectrum", got, want)
    assert 0 <= r.pcg <= int(cfg.PCG_MAX_ITER), (where, "pcg_iterations")
    if not r.deg or hand != "PRECONDITIONED_CG":
        assert r.pcg == 0, (where, "pcg_iterations without PCG")
    if r.lib:
        for A, Vs, idx, lam, name in ((r.Ar, r.Vr, r.ir, r.schur_rot, "rot"), (r.At, r.Vt, r.it, r.schur_trans, "trans")):
            assert np.max(np.abs(A.T @ A - eye3)) <= 1e-12, (where, "aligned_V orthonormal", name)
            assert sorted(idx) == [0, 1, 2], (where, "indices are a permutation", name, idx)
            if np.isnan(lam).any():
                continue
            for grp in _clusters(lam):
                cols = [j for j in range(3) if idx[j] in grp]
                if len(grp) == 1:
                    j, k = cols[0], grp[0]
                    assert min(np.max(np.abs(A[:, j] - Vs[:, k])), np.max(np.abs(A[:, j] + Vs[:, k]))) <= 1e-12, (where, "aligned column", name, j)
                    assert A[j, j] >= -1e-12, (where, "aligned sign", name, j)
                else:       # a repeated eigenvalue: the eigenspace, never the vectors
                    assert np.max(np.abs(A[:, cols] @ A[:, cols].T - Vs[:, grp] @ Vs[:, grp].T)) <= 1e-12, (where, "aligned eigenspace", name)


def _pcg_double(A, b, P, max_iter, tol):
    x, r = np.zeros(6), b.copy()
    bn = np.linalg.norm(b)
    if bn == 0.0:
        return x
    z = P @ r
    p, rz = z.copy(), r @ z
    for _ in range(max_iter):
        Ap = A @ p
        pAp = p @ Ap
        if not pAp > 0.0:
            break
        alpha = rz / pAp
        x, r = x + alpha * p, r - alpha * Ap
        if np.linalg.norm(r) <= tol * bn:
            break
        z = P @ r
        rz, beta = r @ z, (r @ z) / rz
        p = z + beta * p
    return x


def identity(r, H, g, hand, cfg, x, x_qr, x_qr_reg, where=""):
    """(d): the step is the handling's formula on the record's own mask and eigenvectors.  x_qr = the same implementation's plain step
    (NONE_HAND) on H, x_qr_reg on H + STD_REG_GAMMA I"""
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    with np.errstate(all="ignore"):
        if hand in ("NONE_HAND", "ADAPTIVE_REGULARIZATION") or (hand == "PRECONDITIONED_CG" and not r.deg):
            assert same(x, x_qr), (where, "the plain step")
        elif hand == "STANDARD_REGULARIZATION":
            assert same(x, x_qr_reg if r.deg else x_qr), (where, "the regularised step")
        elif hand == "PRECONDITIONED_CG":
            want = _pcg_double(H, g, r.P, int(cfg.PCG_MAX_ITER), float(cfg.PCG_TOLERANCE))
            assert np.all(np.abs(x - want) <= 1e-6 * max(np.max(np.abs(want)), 1e-300)) or same(x, want), (where, "PCG on the record's P", x, want)
        elif hand == "SOLUTION_REMAPPING":
            want = x_qr
            if r.deg and np.all(np.isfinite(r.ev)):
                keep = [i for i in range(6) if not r.mask[i]]
                want = r.V[:, keep] @ (r.V[:, keep].T @ x_qr) if keep else np.zeros(6)
            if np.all(np.isfinite(want)):
                size = np.max(np.abs(x_qr)) if np.all(np.isfinite(x_qr)) else 0.0
                assert np.all(np.abs(x - want) <= 1e-12 * max(size, 1e-300)), (where, "projection of the plain step", x, want)
            else:
                assert not np.all(np.isfinite(x)), (where, "projection of a non-finite plain step")
        elif hand == "TRUNCATED_SVD":
            order = sorted(range(6), key=lambda i: -abs(r.ev[i]))
            want, size = np.zeros(6), 0.0
            for i in range(6):
                if r.mask[i] or not r.sv[i] > 1e-9:
                    continue
                e = order[i]
                term = r.V[:, e] * (r.V[:, e] @ g) / r.ev[e]
                want, size = want + term, size + np.max(np.abs(term))
            assert np.all(np.abs(x - want) <= 1e-12 * max(size, 1e-300)), (where, "truncated SVD on the record's own spectrum", x, want)


def _iv_cond(a, b, da, db, inf_rule):
    """the interval of a / max(b, 1e-12) (or of cond_full's a / b, infinite unless b > 1e-12) when a and b are known to +-da, +-db"""
    if inf_rule:
        lo = np.inf if b + db <= 1e-12 else (a - da) / (b + db)
        hi = np.inf if b - db <= 1e-12 else (a + da) / (b - db)
    else:
        lo, hi = (a - da) / max(b + db, 1e-12), (a + da) / max(b - db, 1e-12)
    return lo * (1 - 8 * U), hi * (1 + 8 * U)


def ratios(r, x, ref):
    """the errors of a record and its step against the reference, each over its bound WITHOUT the constant C -> [(what, ratio)];
    non-finite values must match as such (asserted here)"""
    out = []
    nH = float(ref.normH)
    bs = U * nH
    fv = lambda v: np.array([float(t) for t in v])

    def spectrum(got, want, structural, what, scale=1.0):
        want = fv(want)
        if structural is not None:      # (which of several zeros is the structural one is not a matter of order)
            assert int(np.sum(got == 0.0)) >= sum(structural), (what, "a structural zero is an exact zero", got)
        err = float(np.max(np.abs(got - want)))
        out.append((what, err / (bs * scale) if bs > 0 else (np.inf if err > 0 else 0.0)))

    spectrum(r.ev, ref.ev, ref.structural, "eigenvalues_full")
    spectrum(r.sv, ref.sv, None, "singular_values")
    kb = float(ref.kappa_blocks)
    if ref.schur_ran:
        spectrum(r.sub_rot, ref.sub_rot, ref.sub_rot_structural, "lambda_sub_rot")
        spectrum(r.sub_trans, ref.sub_trans, ref.sub_trans_structural, "lambda_sub_trans")
    else:
        assert np.isnan(r.sub_rot).all() and np.isnan(r.sub_trans).all() and np.isnan(r.cond_diag_rot) and np.isnan(r.cond_diag_trans)
    if ref.schur_ok:
        spectrum(r.schur_rot, ref.schur_rot, None, "lambda_schur_rot", kb)
        spectrum(r.schur_trans, ref.schur_trans, None, "lambda_schur_trans", kb)
        Pw = np.array([[float(ref.P[i, j]) for j in range(6)] for i in range(6)])
        out.append(("P_preconditioner", float(np.max(np.abs(r.P - Pw))) / (U * kb * float(ref.kappa_P) * np.max(np.abs(Pw)))))
    else:
        assert np.isnan(r.schur_rot).all() and np.isnan(r.schur_trans).all()
        want = np.inf if ref.schur_ran else np.nan
        assert _same(r.cond_schur_rot, want) and _same(r.cond_schur_trans, want), ("cond_schur", r.cond_schur_rot, want)
        assert np.array_equal(r.P, np.eye(6))
    # condition numbers: inside the interval the bound on their spectra leaves (C enters through `ratio`: the smallest C that admits it)
    def cond(got, a, b, b_structural, inf_rule, what, scale=1.0, mixed=False):
        a, b = float(a), float(b)
        b_structural = b_structural and b == 0.0 and not mixed      # beside a zero of rounding noise the order of the zeros is arbitrary
        for c in (0.0, 1.0, 4.0, 16.0, 64.0, 256.0, 1024.0, 4096.0):
            lo, hi = _iv_cond(a, b, c * bs * scale, 0.0 if b_structural else c * bs * scale, inf_rule)
            if lo <= got <= hi:
                out.append((what, c))
                return
        out.append((what, np.inf))

    ev, st = fv(ref.ev), ref.structural
    mixed = any(ref.tiny)
    cond(r.cond_full, ref.sv[0], ref.sv[5], st[ref.order[5]], True, "cond_full", mixed=mixed)
    cond(r.cond_full_sub_trans, abs(ev[2]), abs(ev[0]), st[0], False, "cond_full_sub_trans", mixed=mixed)
    cond(r.cond_full_sub_rot, abs(ev[5]), abs(ev[3]), st[3], False, "cond_full_sub_rot", mixed=mixed)
    if ref.schur_ran:
        for lam, s, got, what in ((ref.sub_rot, ref.sub_rot_structural, r.cond_diag_rot, "cond_diag_rot"), (ref.sub_trans, ref.sub_trans_structural, r.cond_diag_trans, "cond_diag_trans")):
            lam = fv(lam)
            cond(got, lam[2], lam[0], s[0], False, what, mixed=True)      # (the blocks: a structural zero is given the spectrum's noise too)
    if ref.schur_ok:
        cond(r.cond_schur_rot, fv(ref.schur_rot)[2], fv(ref.schur_rot)[0], False, False, "cond_schur_rot", kb)
        cond(r.cond_schur_trans, fv(ref.schur_trans)[2], fv(ref.schur_trans)[0], False, False, "cond_schur_trans", kb)
    # the step
    if x is not None:
        want = fv(ref.x)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(x), np.isnan(want)) and np.array_equal(x[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), ("non-finite step", x, want)
        if fin.all():
            bound = U * float(ref.kappa) * np.max(np.abs(want))
            err = float(np.max(np.abs(x - want)))
            out.append(("step (PCG)" if ref.pcg_iterations else "step", err / bound if bound > 0 else (np.inf if err > 0 else 0.0)))
    return out


def exact_fields(r, ref, where=""):
    assert r.mask == ref.mask and r.deg == int(ref.is_degenerate), (where, "mask", r.deg, r.mask, ref.is_degenerate, ref.mask)
    assert r.pcg == ref.pcg_iterations, (where, "pcg_iterations", r.pcg, ref.pcg_iterations)
