"""Host replay of the verification call's per-point function (dcreg_amd/csrc/device/verify.hpp through tests/emul_verify.py) against the
numpy reference of tests/verify_ref.py: inlier flags, nearest index, d2 bits and integer terms BITWISE - on the lot's poses, on the
lattice whose distances sit on the gate, for queries many cells outside the grid and for an inlier distance larger than the map."""
import numpy as np
import pytest

import emul_verify as ev
import normal_icp_scenes as sc
import verify_ref as vr
from test_normals_reference import lattice


def assert_bitwise(got, map_xyz, cloud, Ts, d, what=""):
    for k, T in enumerate(np.asarray(Ts, np.float64).reshape(-1, 4, 4)):
        want = vr.score_pose(map_xyz, cloud, T, d)
        assert np.array_equal(got["inl"][k], want["mask"]), (what, k)
        assert np.array_equal(got["nn"][k], want["nn"]), (what, k)
        inl = want["mask"] == 1
        assert np.array_equal(got["d2"][k][inl].view(np.uint32), want["d2"][inl].view(np.uint32)), (what, k)
        assert np.isinf(got["d2"][k][~inl]).all() and not got["e"][k][~inl].any(), (what, k)
        assert (got["count"][k], got["cost"][k]) == (want["count"], want["cost"]), (what, k, got["count"][k], got["cost"][k], want["count"], want["cost"])


@pytest.mark.parametrize("d", [0.1, 0.3, 0.5])
@pytest.mark.parametrize("cell", [0.0, 0.11, 0.7])
def test_the_lot_poses_are_bitwise_the_reference(d, cell):
    """in the cells the build would choose and in cells much smaller and larger than the distance: the grid decides how fast, never which"""
    L = sc.lot()
    Ts = vr.lot_poses()
    m = ev.Map(L["tgt"], 0.5, cell=cell)
    assert_bitwise(ev.verify(m, L["src"], Ts, d), L["tgt"], L["src"], Ts, d, (d, cell))


@pytest.mark.parametrize("cell", [0.0, 0.1, 0.6])
def test_the_lattice_edge_the_gate_is_strict(cell):
    lat = lattice((8, 8, 8), 0.25)
    T = np.eye(4)
    T[0, 3] = 0.125
    m = ev.Map(lat, 0.25, cell=cell)
    at = ev.verify(m, lat, [T], 0.125)
    assert at["count"] == [0] and at["cost"] == [0]
    up = ev.verify(m, lat, [T], np.nextafter(0.125, 1.0))
    assert up["count"] == [512] and up["cost"] == [512 * ((1 << 20) - 1)] and (up["nn"][0] == np.arange(512)).all()
    for d in (0.125, np.nextafter(0.125, 1.0), np.nextafter(0.125, 0.0), 0.2):
        assert_bitwise(ev.verify(m, lat, [T, np.eye(4)], d), lat, lat, [T, np.eye(4)], d, (cell, d))


def test_queries_far_outside_the_grid_and_a_distance_larger_than_the_map():
    L = sc.lot()
    m = ev.Map(L["tgt"], 0.5)
    far = [sc.offset(L["GT"], dx=x) for x in (30.0, -2000.0, 4.0e6)] + [sc.offset(L["GT"], dz=-1.0e5)]
    got = ev.verify(m, L["src"], far, 0.5)
    assert got["count"] == [0, 0, 0, 0] and got["evals"] == 0             # nothing within reach: no candidate is even looked at
    assert_bitwise(got, L["tgt"], L["src"], far, 0.5, "far")
    # every map point lies inside the distance: the walk sweeps the whole grid, whatever the pose
    for d in (40.0, 1.0e4):
        Ts = [L["GT"], far[0], sc.offset(L["GT"], dx=-35.0, yaw=1.0)]
        got = ev.verify(m, L["src"][::7], Ts, d)
        assert_bitwise(got, L["tgt"], L["src"][::7], Ts, d, d)
        assert got["count"][0] == len(L["src"][::7])
