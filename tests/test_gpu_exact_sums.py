"""The second engine (dcreg_linearize_normals and its batched form) on the scene of tests/exact_sums_scene.py, whose sums are exact in
double in any order of addition: the device's 31 sums must equal math.fsum's bit for bit, at every size and through every level of the
reduction - wave Gram matrices, block rows, chunk sums, the result row.  One wrong, missing or doubled term anywhere shows as a
difference; no tolerance is involved."""
import numpy as np
import pytest

import exact_sums_scene as ex
import normal_icp_scenes as sc
from dcreg_amd import api

pytestmark = pytest.mark.gpu


def lin_params(wd):
    p = api.default_lin_params(ex.RADIUS, wd)
    p.weight_slope, p.weight_min = ex.SLOPE, ex.W_MIN
    return p


def context(src=None):
    tgt, nrm = ex.lattice_map()
    c = api.Context(0)
    c.set_target(tgt, ex.RADIUS)
    if src is not None:
        c.set_source(src)
    c.set_target_normals(np.ascontiguousarray(nrm))
    return c


def assert_exact(got, want, what):
    assert (got["n_eff"], got["n_pt"]) == (want["n_eff"], want["n_pt"]), (what, got["n_eff"], got["n_pt"])
    for k in ("H_upper", "g", "sum_r2", "sum_b2"):
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert np.array_equal(a, b), (what, k, a, b)            # (equal values: bit for bit but for the sign of a zero)


@pytest.mark.parametrize("n", ex.SIZES)
def test_single_launches_give_fsum_bit_for_bit(n):
    for rotation in ex.ROTATIONS:
        S = ex.scene(n, rotation, 0)
        c = context(S["src"])
        try:
            for wd in (0, 1):
                S = ex.scene(n, rotation, wd)
                got = c.linearize_normals(S["T"], lin_params(wd))
                assert_exact(got, S["want"], (n, rotation, wd))
                assert_exact(c.linearize_normals(S["T"], lin_params(wd)), S["want"], (n, rotation, wd, "warm"))
            if n == 4099:
                dump = c.linearize_normals(S["T"], lin_params(1), debug=True)
                sc.assert_dump_bitwise(dump, S["want"], (n, rotation))
                assert_exact(dump, S["want"], (n, rotation, "dump"))
        finally:
            c.close()


@pytest.mark.parametrize("wd", [0, 1])
def test_a_batched_launch_gives_fsum_bit_for_bit(wd):
    """three frames of 16 385 points, one per rotation, in one launch"""
    n = 16385
    scenes = [ex.scene(n, rotation, wd) for rotation in ex.ROTATIONS]
    c = context()
    try:
        c.frames_load([S["src"] for S in scenes])
        c.normals_reserve_slots(3)
        for ids in ([0, 1, 2], None, [2, 0, 1]):
            got = c.normals_batch([S["T"] for S in scenes], ids, [0, 1, 2], lin_params(wd))
            for k, (g, S) in enumerate(zip(got, scenes)):
                assert_exact(g, S["want"], (wd, k, ids))
    finally:
        c.close()
