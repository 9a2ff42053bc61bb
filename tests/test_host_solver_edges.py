"""CPU tests of the degeneracy solver (csrc/host/solver.cpp, linalg.hpp) through the C-ABI on singular, repeated, threshold, scaled and
improper systems (solver_scenes.py), against the 50-digit reference (solver_ref.py) and the oracle.

A cell is (system, detection, handling, configuration): 40 finite systems x 5 x 6 x 4.  Every cell's record must agree with itself and its
step with its handling's formula (solver_checks.consistent / identity); every DECIDABLE cell (solver_ref: every comparison of the rule
clears its threshold in 50 digits) must equal the reference - masks, flags and PCG iteration counts exactly, spectra, condition numbers
and steps to solver_checks.tol_c * 2^-52 * kappa.  On an exactly rank-deficient H that is not singular along coordinate axes (a tilted
plane, a rank-1 matrix) the library and the oracle may legitimately differ in a mask bit and then in the first digit of a step - the
sign of a 1e-15 eigenvalue decides the reference's own FULL_SVD rule -; there only self-consistency and the identities are asserted.

Measured (test_oracle_measures_the_tolerance prints it): the oracle's largest error-to-bound ratio over the decidable cells is C = 196, a
PCG step.  Per kind of quantity it is 4.8 (spectra, condition numbers, the preconditioner), 1.16 (steps by QR, remapping, truncated SVD)
and 196.4 (PCG steps); each kind is pinned to its own figure rounded up to an integer - 5, 2, 197 - and the library held to
8 x that: 40, 16, 1576.  The library's own largest ratios are 4, 2.5 and 5.2.

Non-finite input: before the fix in solveDegenerateSystem, of the 360 calls of test_a_non_finite_system_gives_a_non_finite_step's systems
45 with TRUNCATED_SVD and 26 with PRECONDITIONED_CG returned x = [0, 0, 0, 0, 0, 0]; after it none returns a finite x."""
import numpy as np
import pytest

import solver_checks as ck
import solver_ref as sr
import solver_scenes as sc
from dcreg_amd import api
from oracle import pyoracle as po


def _cfgs(key):
    k, s = key
    return api.default_config(KAPPA_TARGET=k, always_compute_schur=s), po.default_config(kappa_target=k, always_compute_schur=s)


def _lib(H, g, det, hand, cfg):
    an = api.analyze_degeneracy(H, det, hand, cfg)
    x = api.solve_degenerate_system(H, g, hand, cfg, an)
    return an, x


def _orc(H, g, det, hand, ocfg):
    an = po.analyze(H, det, hand, ocfg)
    x = po.solve(H, g, hand, ocfg, an)
    return an, x


@pytest.fixture(scope="module")
def runs():
    """every cell through the library and the oracle, once: {cell key: (family, H, g, cfg, (record, x, plain x, plain x of H + gamma I)
    of the library, the same of the oracle)}"""
    out = {}
    for name, family, H, g, key, det, hand in ck.cells():
        cfg, ocfg = _cfgs(key)
        Hg = H + cfg.STD_REG_GAMMA * np.eye(6)
        an, x = _lib(H, g, det, hand, cfg)
        lib = (ck.record(an), x, api.solve_degenerate_system(H, g, "NONE_HAND", cfg, an), api.solve_degenerate_system(Hg, g, "NONE_HAND", cfg, an))
        oan, ox = _orc(H, g, det, hand, ocfg)
        orc = (ck.record(oan), ox, po.solve(H, g, "NONE_HAND", ocfg, oan), po.solve(Hg, g, "NONE_HAND", ocfg, oan))
        out[(name, key, det, hand)] = (family, H, g, cfg, lib, orc)
    return out


def _ref(cell, H, g):
    name, key, det, hand = cell
    return ck.reference(name, H, g, det, hand, key)


def test_every_record_is_self_consistent(runs):
    """(b) the mask and the flag are the rule on the record's own spectra, bit for bit, whatever rounding did to a zero eigenvalue; bases
    orthonormal, indices permutations, aligned columns +- the chosen Schur eigenvectors, the preconditioner's spectrum; library and oracle"""
    for cell, (family, H, g, cfg, lib, orc) in runs.items():
        ck.consistent(lib[0], cfg, cell[2], cell[3], ("library",) + cell)
        ck.consistent(orc[0], cfg, cell[2], cell[3], ("oracle",) + cell)


def test_every_step_is_its_handlings_formula_on_the_record(runs):
    """(d), asserted of every cell: the step is the handling's identity on the record's own mask and eigenvectors, and finite outside the
    improper family"""
    for cell, (family, H, g, cfg, lib, orc) in runs.items():
        for who, (r, x, xq, xr) in (("library", lib), ("oracle", orc)):
            ck.identity(r, H, g, cell[3], cfg, x, xq, xr, (who,) + cell)
            # decidable or not: QR on a pivot of rounding noise gives a huge step, never a non-finite one
            assert family == "improper" or np.all(np.isfinite(x)), (who, cell, x)


def _decidable(runs):
    for cell, v in runs.items():
        ref = _ref(cell, v[1], v[2])
        if not ref.undecided:
            yield cell, v, ref


def test_oracle_measures_the_tolerance(runs):
    """C of the tolerance: the oracle against the reference over the decidable cells.  Pinned as solver_checks.MEASURED_C"""
    worst = {}
    for cell, (family, H, g, cfg, lib, orc), ref in _decidable(runs):
        ck.exact_fields(orc[0], ref, ("oracle",) + cell)
        for what, q in ck.ratios(orc[0], orc[1], ref):
            if q > worst.get(what, (-1.0, None))[0]:
                worst[what] = (q, cell)
    for what, (q, cell) in sorted(worst.items()):
        print("oracle / reference  %-22s %10.3g  %s" % (what, q, cell))
    print("measured C = %.3g overall" % max(q for q, _ in worst.values()))
    for k, pinned in ck.MEASURED_C.items():
        c = max(q for what, (q, _) in worst.items() if ck.kind(what) == k)
        print("measured C (%s) = %.3g, pinned %.3g, the library is held to %.3g" % (k, c, pinned, ck.MARGIN * pinned))
        assert c <= pinned, (k, c, pinned)


def test_library_equals_the_reference_on_decidable_cells(runs):
    """(c) masks, flags and PCG iteration counts exactly; spectra, condition numbers, the preconditioner and the step of all six handlings
    to tol_c * 2^-52 * kappa; infinities and NaNs as such"""
    worst = {}
    n = 0
    for cell, (family, H, g, cfg, lib, orc), ref in _decidable(runs):
        n += 1
        ck.exact_fields(lib[0], ref, ("library",) + cell)
        for what, q in ck.ratios(lib[0], lib[1], ref):
            if q > worst.get(what, (-1.0, None))[0]:
                worst[what] = (q, cell)
            assert q <= ck.tol_c(what), (cell, what, q, ck.tol_c(what))
    for what, (q, cell) in sorted(worst.items()):
        print("library / reference %-22s %10.3g  %s" % (what, q, cell))
    assert n >= 0.75 * len(runs)


def test_library_and_oracle_agree_on_decidable_cells(runs):
    """masks exactly, the step to the tolerance of test_host_solver.py"""
    for cell, (family, H, g, cfg, lib, orc), ref in _decidable(runs):
        assert (lib[0].deg, lib[0].mask) == (orc[0].deg, orc[0].mask), cell
        x, ox = lib[1], orc[1]
        assert np.array_equal(np.isnan(x), np.isnan(ox)), (cell, x, ox)
        if np.all(np.isfinite(ox)):
            assert np.allclose(x, ox, rtol=1e-8, atol=1e-12 * max(1.0, np.max(np.abs(ox)))), (cell, x, ox)


def test_two_part_analysis_is_byte_identical_on_every_system():
    """(e) analyzeStep + analyzeFinish (the pipelined loop's analysis) against the one-pass record: every system, the non-finite ones
    included, all 30 detection / handling pairs, all four configurations"""
    owed_singular = 0
    for name, family, H, g in sc.SYSTEMS + sc.NONFINITE:
        for key in sc.CONFIGS:
            cfg, _ = _cfgs(key)
            for det in sr.DETECTIONS:
                for hand in sr.HANDLINGS:
                    one = api.analyze_degeneracy(H, det, hand, cfg)
                    two, owed = api.analyze_degeneracy_two_part(H, det, hand, cfg)
                    assert bytes(one) == bytes(two), (name, det, hand, key, owed)
                    if family in ("plane", "plane_tilted", "corridor", "sphere", "cylinder", "line", "rank_one") or name == "zero":
                        owed_singular += owed != 0
    assert owed_singular > 0


@pytest.mark.parametrize("hand", sr.HANDLINGS)
def test_a_non_finite_system_gives_a_non_finite_step(hand):
    """(f) H or g with one NaN, +Inf or -Inf entry: every call returns (the eigen-solver's 60-sweep cap ends it) and the step carries a
    non-finite entry with every handling, so that the loop's check aborts with status 2 and never reads a finite 0 as convergence"""
    for name, family, H, g in sc.NONFINITE:
        for key in sc.CONFIGS:
            cfg, ocfg = _cfgs(key)
            for det in sr.DETECTIONS:
                an, x = _lib(H, g, det, hand, cfg)
                print("library %-12s %-24s %-24s x = %s" % (name, det, hand, x))
                assert not np.all(np.isfinite(x)), ("library", name, det, hand, key, x)
                oan, ox = _orc(H, g, det, hand, ocfg)
                assert not np.all(np.isfinite(ox)), ("oracle", name, det, hand, key, ox)
