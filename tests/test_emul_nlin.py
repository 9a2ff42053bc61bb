"""Host replay of the second engine's per-point function (dcreg_amd/csrc/device/normal_icp.hpp through tests/emul_nlin.py) against the numpy
reference of tests/normal_icp_ref.py: flags, nearest index, d2 bits, residual, weight and rows BITWISE - on the lot, on ties, duplicates
and queries outside the grid, and along a walk with the warm words carried, where warm and cold must agree bit for bit."""
import numpy as np
import pytest

import emul_nlin as en
import normal_icp_ref as ref
import normal_icp_scenes as sc

CASES = {"lattice": sc.lattice_case, "duplicates": sc.duplicate_case, "outside": sc.outside_case, "gates": sc.gate_case}


def reference(C, T, radius, wd, slope=0.9):
    return ref.linearize(C["tgt"], C["normals"], C["src"], T, radius, weight_slope=slope, use_weight_derivative=wd)


@pytest.mark.parametrize("normals", ["n5", "nb"])
@pytest.mark.parametrize("radius", [0.5, 0.1])
def test_the_lot_is_bitwise_the_reference(normals, radius):
    L = sc.lot()
    m, s = en.Map(L["tgt"], L[normals], radius), en.Source(L["src"])
    for pose in ("INIT", "MID"):
        for wd in (0, 1):
            want = ref.linearize(L["tgt"], L[normals], L["src"], L[pose], radius, use_weight_derivative=wd)
            got = en.linearize(m, s, L[pose], radius, wd=wd, warm=False)
            sc.assert_dump_bitwise(got, want, (pose, wd))
            sc.assert_sums_close(got, want, (pose, wd))
    assert (want["flag"] == 0).any() == (radius == 0.1) and (want["flag"] == 2).any() == (normals == "nb")


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("cell", [0.0, 0.11, 0.7])
def test_ties_duplicates_gates_and_queries_outside_the_grid(name, cell):
    """in the cells the build would choose and in cells much smaller and larger than the radius: the grid decides how fast, never which"""
    C = CASES[name]()
    slopes = sc.GATE_SLOPES if name == "gates" else (0.9,)
    m, s = en.Map(C["tgt"], C["normals"], C["radius"], cell=cell), en.Source(C["src"])
    for slope in slopes:
        want = reference(C, C["T"], C["radius"], 1, slope)
        for warm in (False, True, True):
            got = en.linearize(m, s, C["T"], C["radius"], wd=1, warm=warm, w_slope=slope)
            sc.assert_dump_bitwise(got, want, (name, cell, slope, warm))
            sc.assert_sums_close(got, want, (name, cell, slope, warm))
    if name == "gates":
        assert list(want["flag"]) == sc.GATE_FLAGS
    if name == "lattice":                      # every query ties eight corners: the lowest index wins
        assert np.all(want["nn_d2"] == np.float32(3 * 0.125 ** 2)) and (want["flag"] != 0).all()
    if name == "outside":
        assert (want["flag"] == 0).sum() > 50 and (want["flag"] != 0).sum() > 50


def test_a_walk_with_the_warm_words_carried_is_bitwise_cold_and_cheaper():
    L = sc.lot()
    m = en.Map(L["tgt"], L["nb"], 0.5)
    warm_src, cold_src = en.Source(L["src"]), en.Source(L["src"])
    for step, T in enumerate(sc.walk()):
        want = ref.linearize(L["tgt"], L["nb"], L["src"], T, 0.5, use_weight_derivative=1)
        w = en.linearize(m, warm_src, T, 0.5, wd=1, warm=True)
        c = en.linearize(m, cold_src, T, 0.5, wd=1, warm=False)
        assert w["warm_used"] == (step > 0) and not c["warm_used"]
        sc.assert_dump_bitwise(w, want, step)
        sc.assert_dump_bitwise(c, want, step)
        sc.assert_sums_bitwise(w, c, step)             # (the replay adds in processing order either way)
        if step == 1:                                  # a small step: the old neighbour bounds the search tightly
            assert w["evals"] < 0.6 * c["evals"], (w["evals"], c["evals"])
        assert w["evals"] <= c["evals"] + len(L["src"])      # never worse than cold by more than the one extra look per point


def test_warm_words_of_another_radius_and_garbage_words_change_nothing():
    """the words are positions of real map points or anything at all: a word beyond the map is ignored, a valid one only bounds"""
    L = sc.lot()
    m, s = en.Map(L["tgt"], L["n5"], 0.5), en.Source(L["src"])
    want = ref.linearize(L["tgt"], L["n5"], L["src"], L["MID"], 0.1)
    en.linearize(m, s, L["INIT"], 0.5, warm=True)                      # words of the large radius ...
    sc.assert_dump_bitwise(en.linearize(m, s, L["MID"], 0.1, warm=True), want, "radius")      # ... bound a search of the small one
    s.warm = np.random.default_rng(3).integers(0, 2 ** 32, s.n, dtype=np.uint64).astype(np.uint32)
    s.warm[::2] %= np.uint32(len(L["tgt"]))                            # half of them valid positions of unrelated points
    sc.assert_dump_bitwise(en.linearize(m, s, L["MID"], 0.1, warm=True), want, "garbage")
