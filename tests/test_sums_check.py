"""tests/sums_check.py on the CPU: the entry-wise check accepts what any correct summation gives and rejects what the norm-wise
comparison (normal_icp_scenes.assert_sums_close: max |a - b| / max |b| over all of H at once) lets through.  The rows are the
reference's (tests/normal_icp_ref.py) on the lot; computed once per module, never modified."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import normal_icp_ref as ref
import normal_icp_scenes as sc
import sums_check as sums

N = 4099


@functools.lru_cache(maxsize=None)
def lot_rows():
    """the reference linearisation of sized_source(4099) on the lot, halfway between the start and the truth, weight derivative on"""
    L = sc.lot()
    want = ref.linearize(L["tgt"], L["nb"], sc.sized_source(N), L["MID"], sc.RADIUS, use_weight_derivative=1)
    assert want["n_eff"] > 1000 and (want["flag"] == 2).any()
    sc.frozen(want["row"])
    return want


FAR = np.array([3.0e4, -2.0e4, 500.0])


@functools.lru_cache(maxsize=None)
def far_rows():
    """the same frame with its points moved 3e4 m from the sensor's origin and the pose moved back by as much: the rotation columns of
    the rows carry a lever arm of 3.6e4 m, the translation columns are of size 1"""
    L = sc.lot()
    src = (sc.sized_source(N).astype(np.float64) + FAR).astype(np.float32)
    T = np.array(L["MID"])
    T[:3, 3] = T[:3, 3] - T[:3, :3] @ FAR
    want = ref.linearize(L["tgt"], L["nb"], src, T, sc.RADIUS, use_weight_derivative=1)
    assert want["n_eff"] > 1000
    sc.frozen(want["row"])
    return want


def as_result(slots, want):
    slots = np.asarray(slots, np.float64)
    return dict(H_upper=slots[:21].copy(), g=slots[21:27].copy(), sum_r2=float(slots[27]), sum_b2=float(slots[28]), n_eff=want["n_eff"],
                n_pt=want["n_pt"])


def products(rows):
    """[m, 29]: the rounded products of every slot"""
    return np.stack([rows[:, a] * rows[:, b] for a, b in sums.PAIRS], axis=1)


def check(got, want, slack=0):
    return sums.assert_sums_entrywise(got, want["row"], want["n_eff"], want["n_pt"], "test", slack)


def rejected(got, want):
    """-> the slot named by the failing assertion"""
    with pytest.raises(AssertionError) as e:
        check(got, want)
    return e.value.args[0][1]


def test_exact_sums_are_the_rational_sums_rounded_once():
    rows = lot_rows()["row"]
    rows = rows[np.any(rows != 0.0, axis=1)][:100]
    exact, absum = sums.exact_sums(rows)
    for k, (a, b) in enumerate(sums.PAIRS):
        terms = [Fraction(float(x)) * Fraction(float(y)) for x, y in zip(rows[:, a], rows[:, b])]
        assert exact[k] == float(sum(terms)) and absum[k] == float(sum(abs(t) for t in terms)), sums.NAMES[k]
        p, e = sums.two_product(rows[:, a], rows[:, b])
        assert all(Fraction(float(x)) + Fraction(float(y)) == t for x, y, t in zip(p, e, terms)), sums.NAMES[k]
    assert float(sums.gamma(4)) == 4.0 * 2.0 ** -53 / (1.0 - 4.0 * 2.0 ** -53)


@pytest.mark.parametrize("scene", ["lot", "far"])
def test_every_correct_summation_is_accepted(scene):
    want = lot_rows() if scene == "lot" else far_rows()
    rows = want["row"]
    P = products(rows)
    exact, _ = sums.exact_sums(rows)
    order = np.random.default_rng(5).permutation(len(rows))
    left_to_right = np.cumsum(P[order], axis=0)[-1]            # (a running sum: one term after the other)
    forms = {"exact": exact, "the reference's fsum of rounded products": sums.slots_of(want), "left to right, random order": left_to_right,
             "numpy pairwise": np.array([np.sum(np.ascontiguousarray(P[:, k])) for k in range(sums.N_SLOTS)])}
    for name, slots in forms.items():
        worst = check(as_result(slots, want), want)
        print("%s, %s: the largest error is %.3g of its bound" % (scene, name, worst))
        assert worst < 1.0
    assert check(as_result(exact, want), want) < 1e-3          # (one rounding against a bound of thousands)
    # a result without any effective point: every slot exactly zero, and nothing else is accepted
    none = dict(row=np.zeros((7, 8)), n_eff=0, n_pt=3)
    check(as_result(np.zeros(sums.N_SLOTS), none), none)
    assert rejected(as_result(np.full(sums.N_SLOTS, 5e-324), none), none) == "H[0,0]"
    # the counts are exact
    for key in ("n_eff", "n_pt"):
        wrong = as_result(exact, want)
        wrong[key] += 1
        with pytest.raises(AssertionError):
            check(wrong, want)


def test_a_row_left_out_is_rejected():
    want = lot_rows()
    rows = want["row"]
    eff = np.flatnonzero(want["flag"] == 1)
    for leave in (eff[0], eff[len(eff) // 2], eff[-1]):
        part, _ = sums.exact_sums(np.delete(rows, leave, axis=0))
        assert rejected(as_result(part, want), want) in sums.NAMES
    # ... and so is a row counted twice
    twice, _ = sums.exact_sums(np.concatenate([rows, rows[eff[:1]]]))
    assert rejected(as_result(twice, want), want) in sums.NAMES


def test_one_slot_off_by_1e_9_of_its_own_value_is_rejected():
    """In every slot whose bound is below 1e-9 of the slot's value - the bound is gamma * sum |terms|, 4.6e-13 of the value where the
    terms do not cancel (the diagonal of H, sum_r2, sum_b2) - and that is all of them on this scene."""
    want = lot_rows()
    exact, absum = sums.exact_sums(want["row"])
    bound = float(sums.gamma(len(want["row"]) + 2)) * absum
    caught = 0
    for k in range(sums.N_SLOTS):
        for factor in (1.0 + 1e-9, 1.0 - 1e-9):
            wrong = exact.copy()
            wrong[k] *= factor
            if 1e-9 * abs(exact[k]) > 2.0 * bound[k]:
                assert rejected(as_result(wrong, want), want) == sums.NAMES[k]
                caught += 1
    squares = [k for k, (a, b) in enumerate(sums.PAIRS) if a == b]
    assert all(1e-9 * abs(exact[k]) > 2.0 * bound[k] for k in squares) and len(squares) == 8
    print("slots in which 1e-9 is caught: %d of %d" % (caught // 2, sums.N_SLOTS))
    assert caught == 2 * sums.N_SLOTS


def test_a_wrong_translation_block_far_from_the_origin_passes_the_norm_wise_check_and_fails_this_one():
    """The reason this file exists: 3e4 m from the origin the translation block of H is 1e-9 of max |H|, so a comparison relative to
    max |H| at 1e-9 cannot see it at all."""
    want = far_rows()
    exact, _ = sums.exact_sums(want["row"])
    H = exact[:21]
    block = [k for k, (a, b) in enumerate(sums.PAIRS[:21]) if a >= 3]
    assert len(block) == 6 and max(abs(H[k]) for k in block) < 1e-8 * np.abs(H).max()
    wrong = exact.copy()
    wrong[block] *= 1.0 + 1e-6
    got = as_result(wrong, want)
    sc.assert_sums_close(got, want, "far")                      # accepted: relative to max |H| the block is not there
    assert rejected(got, want) == "H[3,3]"
    check(as_result(exact, want), want)
    # the same error on the lot itself, its points around the sensor, is rejected as well
    near = lot_rows()
    ex, _ = sums.exact_sums(near["row"])
    wr = ex.copy()
    wr[block] *= 1.0 + 1e-6
    assert rejected(as_result(wr, near), near) == "H[3,3]"


@pytest.mark.parametrize("n", [257, 32769])
def test_the_exact_scene_keeps_its_premises_and_its_sums_do_not_depend_on_the_order(n):
    """tests/exact_sums_scene.py asserts its own premises while it builds (the transform exact, every flag 1, rows * 2^9 integers, the sum
    of the absolute integer products below 2^53); here also: a float64 sum in a seeded random order and numpy's own give math.fsum's bits"""
    import exact_sums_scene as ex
    for rotation in ex.ROTATIONS:
        for wd in (0, 1):
            S = ex.scene(n, rotation, wd)
            want = S["want"]
            assert S["worst_log2"] < 45.0
            P = products(want["row"])
            fs = sums.slots_of(want)
            order = np.random.default_rng(n + wd).permutation(n)
            acc = np.cumsum(P[order], axis=0)[-1]               # (a running sum: one term after the other)
            assert np.array_equal(acc, fs) and np.array_equal(P.sum(axis=0), fs), (n, rotation, wd)
            if (rotation, wd) == ("rz90", 1):
                exact, _ = sums.exact_sums(want["row"])
                assert np.array_equal(exact, fs)
                assert check(as_result(fs, want), want) == 0.0
