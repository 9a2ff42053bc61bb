"""Host replay of the fourth engine's per-correspondence functions (dcreg_amd/csrc/device/voxel_icp.hpp vlin_offset, vmap_find_voxel,
vlin_normal, vlin_corr through tests/emul_vlin_stencil.py) against the numpy reference of tests/voxels_stencil_ref.py: voxel, flag, record,
W, the residuals and all three rows of EVERY correspondence bitwise, the point's source normal and the counts - at S = 7 and 27, in both
modes, with a robust kernel off and on, on the lot, the planted scene and the lattice; and at S = 1 the replay of emul_vlin."""
import numpy as np
import pytest

import emul_vlin as ev
import emul_vlin_stencil as es
import normal_icp_scenes as sc
import voxels_scenes as vs
import voxels_stencil_ref as sr
import voxels_stencil_scenes as ss


def _replay(S, T, mode, normals, neighbors, **kw):
    m = S["vmap"]
    return es.linearize(es.records(m), m["coords"], vs.box_of(S["tgt"]), vs.LEAF, S["src"], T, mode, normals, neighbors=neighbors, **kw)


@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("neighbors", [7, 27])
@pytest.mark.parametrize("name", ["lot", "planted7", "lattice"])
def test_every_correspondence_is_bitwise_the_reference(name, neighbors, mode, kind):
    S = ss.SCENES[name]()
    T, nrm = ss.pose_of(S), ss.normals_of(S)
    want = sr.linearize(S["vmap"], S["src"], T, mode, nrm, vs.GICP_EPS, kind, 0.7, neighbors)
    got = _replay(S, T, mode, nrm, neighbors, eps=vs.GICP_EPS, kind=kind, scale=0.7)
    ss.assert_dump_bitwise(got, want, (name, neighbors, mode, kind))
    assert (got["n_eff"], got["n_pt"]) == (want["n_eff"], want["n_pt"])
    sc.assert_sums_close(got, want, (name, neighbors, mode, kind))
    per_point = (want["flag"] == 1).sum(axis=1)
    assert (per_point >= 2).any() and (want["flag"][:, 1:] == 1).any()              # neighbours contribute rows
    if kind:
        assert (want["k"][want["flag"] == 1] < 1.0).any()


def test_one_voxel_per_point_is_the_replay_of_vlin_point():
    for name in ("planted7", "lattice"):
        S = ss.SCENES[name]()
        m = S["vmap"]
        for mode in (0, 1):
            want = ev.linearize(ev.records(m), m["coords"], vs.box_of(S["tgt"]), vs.LEAF, S["src"], S["T"], mode, S["src_normals"], kind=2, scale=0.7)
            got = _replay(S, S["T"], mode, S["src_normals"], 1, kind=2, scale=0.7)
            for k in vs.DUMP_KEYS:
                a = got[k] if k == "normal_src" else got[k][:, 0]
                assert sc.same_bits(a, want[k]), (name, mode, k)
            sc.assert_sums_bitwise(got, want, (name, mode))


def test_a_pose_that_is_not_finite_finds_nothing():
    S = ss.planted7()
    T = np.eye(4)
    T[0, 3] = np.inf
    got = _replay(S, T, 0, None, 7)
    assert not got["flag"].any() and (got["voxel_idx"] == -1).all() and (got["n_eff"], got["n_pt"]) == (0, 0)
