"""A plain high-precision reference of the solver seam (include/dcreg.h "solver seam", csrc/host/solver.cpp), in 50-digit arithmetic.

Written from the rule, not from the C++: what each detection masks, what each handling solves, and which decisions of the rule a
double-precision implementation can be held to.  Nothing here knows tred2 / tql2 or Jacobi: eigen-decompositions come from mpmath.

The rule, for a double H (6 x 6, symmetrised), g, a detection, a handling and a configuration:

  spectra      eigenvalues of H ascending; singular values = |eigenvalues| descending; eigenvalues of the diagonal blocks Hrr, Htt and - when
               both are invertible by full-pivot LU (every pivot above eps * 3 * |largest pivot|) - of the Schur complements
               S_R = Hrr - Hrt Htt^-1 Htr and S_t = Htt - Htr Hrr^-1 Hrt.  The block part runs for the SCHUR detection, the PCG handling, or
               with always_compute_schur; otherwise its numbers read NaN.
  conditions   cond_full = s_max / s_min (infinite unless s_min > 1e-12), cond_full_sub_trans = |l_2| / max(|l_0|, 1e-12),
               cond_full_sub_rot = |l_5| / max(|l_3|, 1e-12), cond_diag_* and cond_schur_* = l_max / max(l_min, 1e-12) of their block
               (cond_schur_* infinite when a block is not invertible).
  mask         SCHUR: bit i of a block where l_max / max(l_i, 1e-12) > DEGENERACY_THRES_COND, every bit when the Schur numbers are
               infinite; FULL_EVD: l_i < DEGENERACY_THRES_EIG; EVD_SUB: a whole block whose cond_diag exceeds the threshold (NaN - the block
               part did not run - exceeds nothing); FULL_SVD: if cond_full exceeds the threshold, l_max / l_i > threshold (no floor, IEEE
               division: a zero eigenvalue gives +inf); NONE: nothing.
  step         NONE, ADAPTIVE_REGULARIZATION (no case) : the column-pivoted QR solution of H x = g
               STANDARD_REGULARIZATION                 : of (H + STD_REG_GAMMA I) x = g when degenerate
               PRECONDITIONED_CG                       : PCG on H x = g with P = blockdiag(V diag(1 / max(l, l_max / KAPPA_TARGET)) V^T) of the
                                                         Schur spectra (identity when they do not exist) when degenerate, else the QR solution
               SOLUTION_REMAPPING                      : the QR solution projected onto the unmasked eigenvectors when degenerate (0 if none)
               TRUNCATED_SVD                           : sum over sigma (descending, index i) with mask[i] == 0 and sigma_i > 1e-9 of
                                                         v_i (v_i . g) / lambda_i - mask[i] belongs to the i-th SMALLEST eigenvalue, the quirk
                                                         the goldens pin
  The QR solution of a rank-deficient matrix (a remaining column below eps * |largest column| in norm) is the basic solution on the pivot
  columns.

decidable(cell): what a double implementation can be held to.
  A comparison against a threshold is decidable when it clears the threshold by more than 1e-6 relative in 50-digit arithmetic - or when H
  is diagonal: then every eigenvalue is an entry of H, and the reference compares the same correctly rounded quotient the doubles give.
  An eigenvalue with |l| <= 1e-9 l_max may be neither divided by nor compared in sign, with one exception that the corridor (rank 5, the
  FULL_SVD mask divides by its zero eigenvalue) needs: a STRUCTURAL zero.  Row and column i of the matrix are exactly zero; then e_i is the
  eigenvector, and every floating-point elimination, Householder reflection or rotation leaves that row and column exactly zero, so that
  the eigenvalue is +0.0 in double too, the LU meets a pivot that is exactly 0 and the QR a column of norm exactly 0.  The two thresholds
  at rounding level (LU pivot against eps * 3 * max pivot, QR column norm against eps * max norm) are decidable from below only through
  such structural zeros: any other exactly singular block leaves a pivot of rounding noise against a threshold of rounding size.
  A comparison of an eigenvalue with an absolute threshold (DEGENERACY_THRES_EIG, 1e-9, 1e-12) must also clear it by the rounding
  noise of a spectrum, NOISE * 2^-52 * ||H||.
  Where the mask splits a cluster of (relatively 1e-6) equal eigenvalues, the remapping and the truncated SVD depend on the basis chosen
  inside the eigenspace: undecidable.
"""
import mpmath as mp
import numpy as np

DPS = 50                     # set around every computation here (mp.workdps), never as the process-wide precision
M = mp.mpf
EPS = M(2) ** -52
CLEAR = M(10) ** -6          # every comparison clears its threshold by this, relative
TINY = M(10) ** -9           # an eigenvalue below TINY * l_max is not divided by or compared in sign
NOISE = M(10) ** 4           # rounding noise of a spectrum: NOISE * 2^-52 * ||H||
EXACT0 = M(10) ** -35        # below this relative size a 50-digit eigenvalue of an integer matrix is an exact zero

DETECTIONS = ["NONE_DETE", "SCHUR_CONDITION_NUMBER", "FULL_EVD_MIN_EIGENVALUE", "EVD_SUB_CONDITION", "FULL_SVD_CONDITION"]
HANDLINGS = ["NONE_HAND", "STANDARD_REGULARIZATION", "ADAPTIVE_REGULARIZATION", "PRECONDITIONED_CG", "SOLUTION_REMAPPING", "TRUNCATED_SVD"]

INF, NAN = M("inf"), M("nan")
FLOOR, SV_MIN = M(1e-12), M(1e-9)      # the rule's two absolute floors, as the doubles the library compares with


def _mat(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[M(float(v)) for v in row] for row in a])


def _sym(A):
    n = A.rows
    return mp.matrix([[(A[i, j] + A[j, i]) / 2 for j in range(n)] for i in range(n)])


def sym_eig(A):
    """eigenvalues ascending, eigenvectors as columns, and which eigenvalues are structural zeros (row and column exactly zero: the
    eigenvector is that axis and the eigenvalue an exact 0)"""
    n = A.rows
    zero = [i for i in range(n) if all(A[i, j] == 0 for j in range(n))]
    live = [i for i in range(n) if i not in zero]
    pairs = [(M(0), [M(1) if k == i else M(0) for k in range(n)], True) for i in zero]
    if live:
        B = mp.matrix([[A[i, j] for j in live] for i in live])
        if all(B[i, j] == 0 for i in range(len(live)) for j in range(len(live)) if i != j):
            E, Q = [B[i, i] for i in range(len(live))], mp.eye(len(live))      # diagonal: the entries themselves, exactly
        else:
            E, Q = mp.eigsy(B)
        for c in range(len(live)):
            v = [M(0)] * n
            for r, i in enumerate(live):
                v[i] = Q[r, c]
            pairs.append((E[c], v, False))
    pairs.sort(key=lambda p: p[0])
    w = [p[0] for p in pairs]
    V = mp.matrix(n, n)
    for c, p in enumerate(pairs):
        for r in range(n):
            V[r, c] = p[1][r]
    return w, V, [p[2] for p in pairs]


class Undecided(list):
    """the reasons a cell is undecidable, as strings"""

    def clear(self, value, threshold, what, exact=False):
        """value against threshold: decidable when it clears by CLEAR relative (or the operands are exact: diagonal H)"""
        if exact:
            return
        if not (abs(value - threshold) > CLEAR * abs(threshold)):
            self.append("%s: %s against %s" % (what, mp.nstr(value, 17), mp.nstr(threshold, 17)))


def _lu_invertible(B, und, what):
    """FullPivLU::isInvertible of a 3 x 3 block: every pivot above eps * 3 * |largest pivot|.  -> True / False"""
    n = B.rows
    A = B.copy()
    structural = [i for i in range(n) if all(B[i, j] == 0 for j in range(n)) and all(B[j, i] == 0 for j in range(n))]
    piv = []
    for k in range(n):
        best, pr, pc = M(-1), k, k
        for i in range(k, n):
            for j in range(k, n):
                if abs(A[i, j]) > best:
                    best, pr, pc = abs(A[i, j]), i, j
        if best == 0:
            # the rest is exactly zero: decided when every zero pivot is a structural one (zero row and column of the block itself)
            if n - k > len(structural):
                und.append("%s: LU pivot %d is zero in exact arithmetic only" % (what, k))
            return False
        for j in range(n):
            A[k, j], A[pr, j] = A[pr, j], A[k, j]
        for i in range(n):
            A[i, k], A[i, pc] = A[i, pc], A[i, k]
        piv.append(A[k, k])
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            for j in range(k, n):
                A[i, j] -= f * A[k, j]
    thr = EPS * n * max(abs(p) for p in piv)
    ok = True
    for k, p in enumerate(piv):
        if abs(p) > thr * (1 + CLEAR):
            continue
        ok = ok and abs(p) > thr
        und.append("%s: LU pivot %d = %s against a threshold of rounding size %s" % (what, k, mp.nstr(p, 5), mp.nstr(thr, 5)))
    return ok


def _kappa_sym(w):
    """condition number of a symmetric matrix from its eigenvalues, over those that are not exact zeros"""
    a = [abs(x) for x in w]
    mx = max(a) if a else M(0)
    nz = [x for x in a if x > EXACT0 * mx]
    return max(nz) / min(nz) if nz else M(1)


def qr_solve(A, b, und, what):
    """the column-pivoted QR solution of the symmetric A x = b -> (x, kappa of what was solved)"""
    n = A.rows
    norms = [mp.sqrt(sum(A[i, j] ** 2 for i in range(n))) for j in range(n)]
    mx = max(norms)
    if mx == 0:          # threshold 0: no column is below it, the back substitution divides 0 by 0
        return [NAN] * n, M(1)
    zero = [j for j in range(n) if norms[j] == 0]
    live = [j for j in range(n) if j not in zero]
    # rank of the live part by the rule, remaining column norms taken exactly (Gram-Schmidt with column pivoting)
    cols = {j: [A[i, j] for i in range(n)] for j in live}
    thr2 = (mx * EPS) ** 2 / n
    rank, k = len(live), 0
    rest = list(live)
    while rest:
        nr = {j: mp.sqrt(sum(v * v for v in cols[j])) for j in rest}
        j0 = max(rest, key=lambda j: nr[j])
        lim = thr2 * (n - k)
        if not (nr[j0] ** 2 > lim * (1 + CLEAR) ** 2):
            und.append("%s: QR column norm %s against a threshold of rounding size %s" % (what, mp.nstr(nr[j0], 5), mp.nstr(mp.sqrt(lim), 5)))
            rank = k
            break
        q = [v / nr[j0] for v in cols[j0]]
        rest.remove(j0)
        for j in rest:
            d = sum(q[i] * cols[j][i] for i in range(n))
            cols[j] = [cols[j][i] - d * q[i] for i in range(n)]
        k += 1
    x = [M(0)] * n
    if rank < len(live):
        return x, M(1)           # undecidable (recorded above): no step to compare
    B = mp.matrix([[A[i, j] for j in live] for i in live])
    # (least squares over the live columns: the zero rows of the symmetric A drop out of it)
    y = mp.lu_solve(B, mp.matrix([b[i] for i in live]))
    for r, j in enumerate(live):
        x[j] = y[r]
    w, _, _ = sym_eig(B)
    return x, _kappa_sym(w)


def pcg(A, b, P, max_iter, tol, und, kappa):
    """preconditioned conjugate gradients, the iteration itself in 50 digits with its three stop rules -> (x, iterations)"""
    n = 6
    x = [M(0)] * n
    r = list(b)
    bn = mp.sqrt(sum(v * v for v in b))
    if bn == 0:
        return x, 0
    mv = lambda Mx, v: [sum(Mx[i, j] * v[j] for j in range(n)) for i in range(n)]
    dot = lambda u, v: sum(a * c for a, c in zip(u, v))
    An = max(abs(A[i, j]) for i in range(n) for j in range(n)) * n
    z = mv(P, r)
    p = list(z)
    rz = dot(r, z)
    iters = 0
    for k in range(max_iter):
        Ap = mv(A, p)
        pAp = dot(p, Ap)
        if not (abs(pAp) > CLEAR * An * dot(p, p)):
            und.append("PCG: p.Ap = %s against 0 at iteration %d" % (mp.nstr(pAp, 5), k))
        if not pAp > 0:
            break
        alpha = rz / pAp
        x = [x[i] + alpha * p[i] for i in range(n)]
        r = [r[i] - alpha * Ap[i] for i in range(n)]
        iters = k + 1
        rn = mp.sqrt(dot(r, r))
        if not (abs(rn - tol * bn) > CLEAR * tol * bn + NOISE * EPS * kappa * bn):
            und.append("PCG: |r| = %s against tol |b| = %s at iteration %d" % (mp.nstr(rn, 5), mp.nstr(tol * bn, 5), k))
        if rn <= tol * bn:
            break
        z = mv(P, r)
        rz_new = dot(r, z)
        beta = rz_new / rz
        rz = rz_new
        p = [z[i] + beta * p[i] for i in range(n)]
    return x, iters


class Ref:
    pass


def _cond_floor(w):
    return max(w) / max(min(w), FLOOR)


def _ieee_div(a, b):
    if b == 0:
        return NAN if a == 0 else (INF if a > 0 else -INF)
    return a / b


def _clusters(w):
    """groups of indices whose eigenvalues agree to CLEAR relative to the largest"""
    mx = max(abs(x) for x in w)
    groups, cur = [], [0]
    for i in range(1, len(w)):
        if abs(w[i] - w[i - 1]) <= CLEAR * mx:
            cur.append(i)
        else:
            groups.append(cur)
            cur = [i]
    groups.append(cur)
    return groups


def reference(H, g, detection, handling, cfg):
    with mp.workdps(DPS):
        return _reference(H, g, detection, handling, cfg)


def _reference(H, g, detection, handling, cfg):
    """cfg: anything with DEGENERACY_THRES_COND, DEGENERACY_THRES_EIG, KAPPA_TARGET, PCG_TOLERANCE, PCG_MAX_ITER, STD_REG_GAMMA,
    always_compute_schur.  H and g finite.  -> Ref: spectra, conditions, mask, step, preconditioner and the list `undecided`"""
    r = Ref()
    und = r.undecided = Undecided()
    Hd = np.asarray(H, dtype=np.float64).reshape(6, 6)
    A = _sym(_mat(Hd))
    gv = [M(float(v)) for v in np.asarray(g, dtype=np.float64).reshape(6)]
    thc, the = M(float(cfg.DEGENERACY_THRES_COND)), M(float(cfg.DEGENERACY_THRES_EIG))
    diagonal = all(A[i, j] == 0 for i in range(6) for j in range(6) if i != j)
    r.diagonal = diagonal

    # ---- spectra
    w, V, sz = sym_eig(A)
    r.ev, r.V, r.structural = w, V, sz
    lmax = max(abs(x) for x in w)
    r.normH = lmax
    r.noise = NOISE * EPS * lmax
    tiny = [(not sz[i]) and abs(w[i]) <= TINY * lmax for i in range(6)]      # not to be divided by or compared in sign
    r.tiny = tiny
    r.sv = sorted((abs(x) for x in w), reverse=True)
    r.order = sorted(range(6), key=lambda i: -abs(w[i]))      # sigma index -> eigen index
    r.cond_full = r.sv[0] / r.sv[5] if r.sv[5] > FLOOR else INF
    r.cond_full_sub_trans = abs(w[2]) / max(abs(w[0]), FLOOR)
    r.cond_full_sub_rot = abs(w[5]) / max(abs(w[3]), FLOOR)

    r.schur_ran = detection == "SCHUR_CONDITION_NUMBER" or handling == "PRECONDITIONED_CG" or bool(cfg.always_compute_schur)
    r.cond_diag_rot = r.cond_diag_trans = r.cond_schur_rot = r.cond_schur_trans = NAN
    r.sub_rot = r.sub_trans = r.schur_rot = r.schur_trans = None
    r.schur_ok = False
    r.P = mp.eye(6)
    r.kappa_blocks = r.kappa_P = M(1)
    lu_und = Undecided()
    if r.schur_ran:
        blk = lambda r0, c0: mp.matrix([[A[r0 + i, c0 + j] for j in range(3)] for i in range(3)])
        Hrr, Htt, Hrt, Htr = blk(0, 0), blk(3, 3), blk(0, 3), blk(3, 0)
        r.sub_rot, _, r.sub_rot_structural = sym_eig(Hrr)
        r.sub_trans, _, r.sub_trans_structural = sym_eig(Htt)
        r.cond_diag_rot, r.cond_diag_trans = _cond_floor(r.sub_rot), _cond_floor(r.sub_trans)
        okT, okR = _lu_invertible(Htt, lu_und, "Htt"), _lu_invertible(Hrr, lu_und, "Hrr")
        r.schur_ok = okT and okR
        if not r.schur_ok:
            r.cond_schur_rot = r.cond_schur_trans = INF
        else:
            SR = _sym(Hrr - Hrt * mp.inverse(Htt) * Htr)
            ST = _sym(Htt - Htr * mp.inverse(Hrr) * Hrt)
            # (a zero row of a Schur complement is the result of a cancellation: never a structural zero of the doubles)
            r.schur_rot, r.Vr, _ = sym_eig(SR)
            r.schur_trans, r.Vt, _ = sym_eig(ST)
            r.schur_rot_structural = r.schur_trans_structural = [False] * 3
            r.cond_schur_rot, r.cond_schur_trans = _cond_floor(r.schur_rot), _cond_floor(r.schur_trans)
            r.kappa_blocks = max(_kappa_sym(r.sub_rot), _kappa_sym(r.sub_trans))
            kt = M(float(cfg.KAPPA_TARGET))
            for b, (lam, Vb) in enumerate(((r.schur_rot, r.Vr), (r.schur_trans, r.Vt))):
                fl = max(lam) / kt
                r.kappa_P = max(r.kappa_P, lmax / max(min(lam), fl))       # 1 / max(l, fl) is Lipschitz with 1 / max(l_min, fl)^2
                for i in range(3):
                    for j in range(3):
                        r.P[3 * b + i, 3 * b + j] = sum(Vb[i, k] * Vb[j, k] / max(lam[k], fl) for k in range(3))
    r.lu_undecided = lu_und

    # ---- mask
    mask = [0] * 6
    deg = False
    if detection == "SCHUR_CONDITION_NUMBER":
        und.extend(lu_und)
        if r.schur_ok:
            for b, lam in enumerate((r.schur_rot, r.schur_trans)):
                st = r.schur_rot_structural if b == 0 else r.schur_trans_structural
                for i in range(3):
                    if not st[i] and abs(lam[i]) <= TINY * max(abs(x) for x in lam):
                        und.append("SCHUR: divides by the eigenvalue %s of a Schur complement" % mp.nstr(lam[i], 5))
                    q = max(lam) / max(lam[i], FLOOR)
                    und.clear(q, thc, "SCHUR bit %d" % (3 * b + i), exact=diagonal and M(float(q)) == q)
                    mask[3 * b + i] = int(q > thc)
            deg = any(mask)
        else:
            mask, deg = [1] * 6, True
    elif detection == "FULL_EVD_MIN_EIGENVALUE":
        for i in range(6):
            und.clear(w[i], the, "FULL_EVD bit %d" % i, exact=diagonal)
            if not diagonal and not sz[i] and not abs(w[i] - the) > r.noise:
                und.append("FULL_EVD bit %d: within the rounding noise of the spectrum" % i)
            mask[i] = int(w[i] < the)
        deg = any(mask)
    elif detection == "EVD_SUB_CONDITION":
        if r.schur_ran:
            for name, c, lam, st in (("rot", r.cond_diag_rot, r.sub_rot, r.sub_rot_structural), ("trans", r.cond_diag_trans, r.sub_trans, r.sub_trans_structural)):
                lo = min(range(3), key=lambda i: lam[i])
                if not st[lo] and abs(lam[lo]) <= TINY * max(abs(x) for x in lam):
                    und.append("EVD_SUB: divides by the eigenvalue %s of H%s" % (mp.nstr(lam[lo], 5), name))
                und.clear(c, thc, "EVD_SUB " + name, exact=diagonal and M(float(c)) == c)
            if r.cond_diag_trans > thc:
                mask[3:] = [1, 1, 1]
            if r.cond_diag_rot > thc:
                mask[:3] = [1, 1, 1]
        deg = any(mask)
    elif detection == "FULL_SVD_CONDITION":
        if tiny[r.order[5]]:
            # the smallest singular value: cond_full is huge or infinite either way, but only if the noise keeps it large
            if not (r.sv[0] / (r.sv[5] + r.noise) > thc * (1 + CLEAR)):
                und.append("FULL_SVD: cond_full within rounding noise of the threshold")
        else:
            und.clear(r.cond_full, thc, "FULL_SVD cond_full", exact=diagonal and (r.cond_full == INF or M(float(r.cond_full)) == r.cond_full))
            if not diagonal and not sz[r.order[5]] and not abs(r.sv[5] - FLOOR) > r.noise:
                und.append("FULL_SVD: the smallest singular value is within rounding noise of 1e-12")
        deg = r.cond_full > thc
        if deg:
            mx = max(w)
            for i in range(6):
                if tiny[i]:
                    und.append("FULL_SVD bit %d: the sign of the eigenvalue %s decides it" % (i, mp.nstr(w[i], 5)))
                q = _ieee_div(mx, w[i])
                if mp.isnan(q):
                    mask[i] = 0
                    continue
                if not mp.isinf(q):
                    und.clear(q, thc, "FULL_SVD bit %d" % i, exact=diagonal and M(float(q)) == q)
                mask[i] = int(q > thc)
    r.mask, r.is_degenerate = mask, bool(deg)

    # ---- step
    r.pcg_iterations = 0
    r.kappa = M(1)
    r.gap = None
    amp = M(1)
    if handling == "PRECONDITIONED_CG":
        und.extend(x for x in lu_und if x not in und)
    if handling == "STANDARD_REGULARIZATION":
        B = A.copy()
        if deg:
            for i in range(6):
                B[i, i] += M(float(cfg.STD_REG_GAMMA))
        r.x, r.kappa = qr_solve(B, gv, und, "QR of H + gamma I")
    elif handling == "PRECONDITIONED_CG" and deg:
        # kappa of the preconditioned system P^1/2 H P^1/2 (similar to P H), over what is not an exact zero
        wp, Vp, _ = sym_eig(_sym(r.P))
        Ph = Vp * mp.diag([mp.sqrt(abs(x)) for x in wp]) * Vp.T      # (|.|: an indefinite H can give a P that is not positive)
        wk, _, _ = sym_eig(_sym(Ph * A * Ph))
        r.kappa = _kappa_sym(wk) * r.kappa_blocks      # (the preconditioner carries the error of the inverted blocks)
        r.x, r.pcg_iterations = pcg(A, gv, r.P, int(cfg.PCG_MAX_ITER), M(float(cfg.PCG_TOLERANCE)), und, r.kappa)
    elif handling == "SOLUTION_REMAPPING":
        x, r.kappa = qr_solve(A, gv, und, "QR of H")
        if deg:
            keep = [i for i in range(6) if not mask[i]]
            r.gap = _split(w, keep, und, "SOLUTION_REMAPPING")
            y = [M(0)] * 6
            for i in keep:
                d = sum(V[k, i] * x[k] for k in range(6))
                y = [y[k] + V[k, i] * d for k in range(6)]
            # the projection's error is relative to the plain step it projects, not to what is left of it
            ny = mp.sqrt(sum(v * v for v in y))
            if ny > 0 and not any(mp.isnan(v) for v in x):
                amp = max(M(1), mp.sqrt(sum(v * v for v in x)) / ny)
                r.kappa *= amp
            x = y
        r.x = x
    elif handling == "TRUNCATED_SVD":
        keep = []
        for i in range(6):
            e = r.order[i]
            if mask[i]:
                continue
            if not sz[e]:
                und.clear(r.sv[i], SV_MIN, "TRUNCATED_SVD sigma %d" % i, exact=diagonal)
                if not diagonal and not abs(r.sv[i] - SV_MIN) > r.noise:
                    und.append("TRUNCATED_SVD sigma %d: within rounding noise of 1e-9" % i)
            if not r.sv[i] > SV_MIN:
                continue
            if tiny[e]:
                und.append("TRUNCATED_SVD: divides by the eigenvalue %s" % mp.nstr(w[e], 5))
            keep.append(e)
        # |lambda| ties between eigenvalues of opposite sign would make the sigma order itself arbitrary
        for i in range(5):
            a, b = r.order[i], r.order[i + 1]
            if (mask[i] != mask[i + 1]) and abs(r.sv[i] - r.sv[i + 1]) <= CLEAR * r.sv[0] and not _same_cluster(w, a, b):
                und.append("TRUNCATED_SVD: sigma %d and %d tie between different eigenvalues" % (i, i + 1))
        r.gap = _split(w, keep, und, "TRUNCATED_SVD")
        y = [M(0)] * 6
        for e in keep:
            d = sum(V[k, e] * gv[k] for k in range(6))
            y = [y[k] + V[k, e] * d / w[e] for k in range(6)]      # sign(l) v (sign(l) v . g) / |l|
        r.x = y
        if keep:
            s = [abs(w[e]) for e in keep]
            r.kappa = max(s) / min(s)
            # v.g is taken of the whole of g, of which the kept directions may hold little: its error is relative to |g|
            ny = mp.sqrt(sum(v * v for v in y))
            if ny > 0:
                amp = max(M(1), mp.sqrt(sum(v * v for v in gv)) / (min(s) * ny))
                r.kappa = max(r.kappa, amp)
    else:       # NONE_HAND, ADAPTIVE_REGULARIZATION, PCG when not degenerate
        r.x, r.kappa = qr_solve(A, gv, und, "QR of H")
    if r.gap is not None:
        r.kappa = max(r.kappa, amp * lmax / r.gap)
    return r


def _same_cluster(w, a, b):
    return abs(w[a] - w[b]) <= CLEAR * max(abs(x) for x in w)


def _split(w, keep, und, what):
    """the kept eigen-indices must be whole clusters of equal eigenvalues -> the smallest gap between a kept and a dropped eigenvalue"""
    gap = None
    for grp in _clusters(w):
        k = [i in keep for i in grp]
        if any(k) and not all(k):
            und.append("%s: the mask splits the eigenvalues %s" % (what, ", ".join(mp.nstr(w[i], 8) for i in grp)))
    for i in range(6):
        for j in range(6):
            if (i in keep) != (j in keep):
                d = abs(w[i] - w[j])
                gap = d if gap is None or d < gap else gap
    if gap is not None and gap == 0:
        gap = None
    return gap


def decidable(ref):
    return not ref.undecided
