"""Host replay of the third engine's per-point functions (dcreg_amd/csrc/device/gicp.hpp through tests/emul_glin.py) against the numpy
reference of tests/gicp_ref.py: flags, nearest index, d2 bits, both normals, the nine entries of W, the residuals and all three rows
BITWISE - on the lot, on ties, duplicates, queries outside the grid and the planted flags, and along a walk with the warm words carried
or filled with garbage, where warm and cold must agree bit for bit."""
import numpy as np
import pytest

import emul_glin as eg
import gicp_ref as gref
import gicp_scenes as gs
import normal_icp_scenes as sc

CASES = {"lattice": gs.lattice_case, "duplicates": gs.duplicate_case, "outside": gs.outside_case, "planted": gs.plant_case}


@pytest.mark.parametrize("normals", [("n5", "m5"), ("nb", "mb")])
@pytest.mark.parametrize("radius", [0.5, 0.1])
def test_the_lot_is_bitwise_the_reference(normals, radius):
    L = gs.lot()
    nm, ns = normals
    m, s = eg.Map(L["tgt"], L[nm], radius), eg.Source(L["src"], L[ns])
    for pose in ("INIT", "MID"):
        for eps in (1e-3, 1e-2):
            want = gref.linearize(L["tgt"], L[nm], L["src"], L[ns], L[pose], radius, eps)
            got = eg.linearize(m, s, L[pose], radius, eps, warm=False)
            gs.assert_dump_bitwise(got, want, (pose, eps))
            sc.assert_sums_close(got, want, (pose, eps))
    assert (want["flag"] == 0).any() == (radius == 0.1) and (want["flag"] == 2).any() == (nm == "nb") and (want["flag"] == 3).any() == (ns == "mb")


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("cell", [0.0, 0.11, 0.7])
def test_ties_duplicates_flags_and_queries_outside_the_grid(name, cell):
    """in the cells the build would choose and in cells much smaller and larger than the radius: the grid decides how fast, never which"""
    C = CASES[name]()
    m, s = eg.Map(C["tgt"], C["normals"], C["radius"], cell=cell), eg.Source(C["src"], C["src_normals"])
    want = gref.linearize(C["tgt"], C["normals"], C["src"], C["src_normals"], C["T"], C["radius"], gs.EPS)
    for warm in (False, True, True):
        got = eg.linearize(m, s, C["T"], C["radius"], gs.EPS, warm=warm)
        gs.assert_dump_bitwise(got, want, (name, cell, warm))
        sc.assert_sums_close(got, want, (name, cell, warm))
    if name == "planted":
        assert list(want["flag"]) == gs.PLANT_FLAGS
    if name == "lattice":                      # every query ties eight corners: the lowest index wins
        assert np.all(want["nn_d2"] == np.float32(3 * 0.125 ** 2)) and (want["flag"] == 1).all()
    if name == "outside":
        assert (want["flag"] == 0).sum() > 50 and (want["flag"] == 1).sum() > 50


def test_a_walk_with_the_warm_words_carried_is_bitwise_cold():
    L = gs.lot()
    m = eg.Map(L["tgt"], L["nb"], 0.5)
    warm_src, cold_src = eg.Source(L["src"], L["mb"]), eg.Source(L["src"], L["mb"])
    for step, T in enumerate(sc.walk()):
        want = gref.linearize(L["tgt"], L["nb"], L["src"], L["mb"], T, 0.5, gs.EPS)
        w = eg.linearize(m, warm_src, T, 0.5, gs.EPS, warm=True)
        c = eg.linearize(m, cold_src, T, 0.5, gs.EPS, warm=False)
        assert w["warm_used"] == (step > 0) and not c["warm_used"]
        gs.assert_dump_bitwise(w, want, step)
        gs.assert_dump_bitwise(c, want, step)
        sc.assert_sums_bitwise(w, c, step)             # (the replay adds in processing order either way)
        assert w["evals"] <= c["evals"] + len(L["src"])      # never worse than cold by more than the one extra look per point


def test_garbage_warm_words_change_nothing():
    """the words are positions of real map points or anything at all: a word beyond the map is ignored, a valid one only bounds"""
    L = gs.lot()
    m, s = eg.Map(L["tgt"], L["n5"], 0.5), eg.Source(L["src"], L["m5"])
    for step, T in enumerate(sc.walk()):
        want = gref.linearize(L["tgt"], L["n5"], L["src"], L["m5"], T, 0.5, gs.EPS)
        s.warm = np.random.default_rng(3 + step).integers(0, 2 ** 32, s.n, dtype=np.uint64).astype(np.uint32)
        s.warm[::2] %= np.uint32(len(L["tgt"]))                        # half of them valid positions of unrelated points
        gs.assert_dump_bitwise(eg.linearize(m, s, T, 0.5, gs.EPS, warm=True), want, step)
