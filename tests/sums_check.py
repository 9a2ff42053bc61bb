"""An entry-wise check of the 31 sums of a linearisation against its rows, with a bound that is derived and not measured.  numpy and
math.fsum only, no device.

rows [m, 8] = [A0..A5, b, r] (dcreg_amd/csrc/device/search.hpp row_of_plane; three rows per point for the third engine).  The 29
floating-point slots are, in this order: the 21 entries of H = sum A A^T (upper triangle, row-major), the 6 of g = sum A b,
sum_r2 = sum r r and sum_b2 = sum b b.  The other two of the 31 are counts and are compared exactly.

The bound.  A slot is a sum of m products.  However they are added - left to right, pairwise, as a tree of wave, block and chunk sums,
each product rounded on its own or fused into the addition - every term passes through at most m roundings (one for its product, at most
m - 1 additions; a fused multiply-add saves one), each of relative size at most u = 2^-53.  So (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 4.2 and lemma 3.1)
        |computed - exact| <= gamma_m * sum |a_i b_i|,    gamma_n = n u / (1 - n u).
Two more roundings are allowed for the yardstick itself (exact_sums rounds the exact sum and the exact sum of the absolute values once
each), hence n = m + 2.  `slack` adds to n: it is for rows that the caller recomputed and that may differ from the device's by a few ulp
per factor.  A slot whose terms are all zero has the bound 0: it must come out exactly 0.  The comparison itself is carried out in
rational arithmetic, so the bound needs no margin.
"""
import math
from fractions import Fraction

import numpy as np

N_SLOTS = 29
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)] + [(a, 6) for a in range(6)] + [(7, 7), (6, 6)]
NAMES = ["H[%d,%d]" % p for p in PAIRS[:21]] + ["g[%d]" % a for a in range(6)] + ["sum_r2", "sum_b2"]
U = Fraction(1, 2 ** 53)
_SPLIT = 134217729.0        # 2^27 + 1 (Veltkamp)


def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product from Veltkamp's split: plain multiplies and adds, no fused
    operation needed).  Holds while nothing overflows and the error term does not underflow: asserted by the caller's range check."""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_sums(rows):
    """rows [m, 8] -> (exact [29], absum [29]): per slot the exactly rounded sum of its m products (the products themselves exact, not
    rounded) and the exactly rounded sum of their absolute values"""
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 8)
    assert np.isfinite(rows).all()
    rows = rows[np.any(rows != 0.0, axis=1)]            # (a row of zeros adds exactly nothing to either sum)
    mag = np.abs(rows[rows != 0.0])
    assert len(mag) == 0 or (mag.max() < 2.0 ** 480 and mag.min() > 2.0 ** -480), "two_product's range"
    exact, absum = np.zeros(N_SLOTS), np.zeros(N_SLOTS)
    for k, (a, b) in enumerate(PAIRS):
        p, e = two_product(rows[:, a], rows[:, b])
        exact[k] = math.fsum(np.concatenate([p, e]))
        absum[k] = math.fsum(np.concatenate([np.abs(p), np.where(p < 0.0, -e, e)]))
    return exact, absum


def slots_of(got):
    """the 29 floating-point slots of a result dict (H_upper, g, sum_r2, sum_b2) in the order of PAIRS"""
    return np.concatenate([np.asarray(got["H_upper"], np.float64).reshape(21), np.asarray(got["g"], np.float64).reshape(6),
                           [np.float64(got["sum_r2"]), np.float64(got["sum_b2"])]])


def gamma(n):
    nu = n * U
    assert nu < 1
    return nu / (1 - nu)


def assert_sums_entrywise(got, rows, n_eff, n_pt, what="", slack=0):
    """got: a result dict (H_upper, g, sum_r2, sum_b2, n_eff, n_pt); rows [m, 8] or [n, 3, 8]: the rows its sums were made of.  The
    counts exactly; every slot within gamma_(m + 2 + slack) * sum |terms| of the exact sum of its products.  -> the largest
    |error| / bound over the slots with a nonzero bound (for reports; 0.0 where there is none)"""
    rows = np.asarray(rows, np.float64).reshape(-1, 8)
    assert (got["n_eff"], got["n_pt"]) == (n_eff, n_pt), (what, got["n_eff"], n_eff, got["n_pt"], n_pt)
    g = gamma(len(rows) + 2 + slack)
    exact, absum = exact_sums(rows)
    have = slots_of(got)
    worst = 0.0
    for k in range(N_SLOTS):
        assert np.isfinite(have[k]), (what, NAMES[k], have[k])
        err = abs(Fraction(float(have[k])) - Fraction(float(exact[k])))
        bound = g * Fraction(float(absum[k]))
        assert err <= bound, (what, NAMES[k], "got %r, exact %r, error %.3e, bound %.3e" % (have[k], exact[k], float(err), float(bound)))
        if bound > 0:
            worst = max(worst, float(err / bound))
    return worst
