"""Host replay of the fourth engine's per-point functions (dcreg_amd/csrc/device/voxel_icp.hpp through tests/emul_vlin.py) against the
numpy reference of tests/voxels_ref.py: voxel, flag, record, source normal, the nine entries of W, the residuals and all three rows
BITWISE - on the lot, the planted map and the lattice, in both modes and with the robust kernels - and flag 5 from a hand-made record."""
import numpy as np
import pytest

import emul_vlin as ev
import normal_icp_scenes as sc
import voxels_ref as vr
import voxels_scenes as vs


def _replay(S, T, mode=0, normals=None, **kw):
    m = S["vmap"]
    return ev.linearize(ev.records(m), m["coords"], vs.box_of(S["tgt"]), vs.LEAF, S["src"], T, mode, normals, **kw)


@pytest.mark.parametrize("mode", [0, 1])
def test_the_lot_is_bitwise_the_reference(mode):
    L = vs.lot()
    for pose in ("INIT", "MID", "GT"):
        for nrm in ("m5", "mb"):
            want = vr.linearize(L["vmap"], L["src"], L[pose], mode, L[nrm], vs.GICP_EPS)
            got = _replay(L, L[pose], mode, L[nrm], eps=vs.GICP_EPS)
            vs.assert_dump_bitwise(got, want, (pose, nrm))
            sc.assert_sums_close(got, want, (pose, nrm))
    assert (want["flag"] == 0).any() and (want["flag"] == 1).any() and (want["flag"] == 3).any() == (mode == 1)


@pytest.mark.parametrize("name", ["planted", "lattice"])
@pytest.mark.parametrize("mode", [0, 1])
def test_planted_voxels_and_the_table_under_load(name, mode):
    S = vs.MAPS[name]()
    want = vr.linearize(S["vmap"], S["src"], S["T"], mode, S["src_normals"], vs.GICP_EPS)
    got = _replay(S, S["T"], mode, S["src_normals"], eps=vs.GICP_EPS)
    vs.assert_dump_bitwise(got, want, (name, mode))
    sc.assert_sums_close(got, want, (name, mode))
    if name == "planted":
        assert got["flag"].tolist() == S["flags%d" % mode]
    else:
        assert (got["flag"] == 0).sum() > 100 and (got["flag"] == 1).sum() > 500


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_the_robust_kernels_are_bitwise_the_reference(kind):
    L = vs.lot()
    for mode in (0, 1):
        want = vr.linearize(L["vmap"], L["src"], L["INIT"], mode, L["m5"], vs.GICP_EPS, kind, 0.7)
        got = _replay(L, L["INIT"], mode, L["m5"], eps=vs.GICP_EPS, kind=kind, scale=0.7)
        vs.assert_dump_bitwise(got, want, (kind, mode))


def test_a_record_that_is_not_positive_definite_is_flag_5():
    rec = np.zeros((2, 12), np.float32)
    rec[0, :3], rec[0, 3:9] = (0.5, 0.5, 0.5), (1, 2, 0, 1, 0, 1)          # s11 - l10^2 = 1 - 4 < 0
    rec[1, :3], rec[1, 3:9] = (1.5, 0.5, 0.5), (1, 0, 0, 1, 0, 1)
    coords = np.array([[0, 0, 0], [1, 0, 0]], np.int64)
    src = np.array([[0.25, 0.5, 0.75], [1.25, 0.5, 0.75], [2.5, 0.5, 0.5]], np.float32)
    got = ev.linearize(rec, coords, (np.array([0, 0, 0]), np.array([2, 0, 0])), 1.0, src, np.eye(4))
    assert got["flag"].tolist() == [5, 1, 0] and got["voxel_idx"].tolist() == [0, 1, -1]
    assert not got["w"][0].any() and not got["row"][0].any() and got["cov"][0].tolist() == [1, 2, 0, 1, 0, 1]
    assert (got["n_eff"], got["n_pt"]) == (1, 2)
    want = vr.linearize(dict(coords=coords, mean=rec[:, :3], cov=rec[:, 3:9], leaf=1.0), src, np.eye(4))
    vs.assert_dump_bitwise(got, want)
