"""The numpy reference of the neighbour-voxel correspondences (tests/voxels_stencil_ref.py) against tests/voxels_ref.py at S = 1, and what
the scenes of tests/voxels_stencil_scenes.py hold - asserted here, on the reference alone, so that the replay's and the device's tests on
the same scenes cannot pass vacuously.  No device."""
import numpy as np
import pytest

import voxels_ref as vr
import voxels_scenes as vs
import voxels_stencil_ref as sr
import voxels_stencil_scenes as ss

# the flags of planted7 at S = 7, mode 0 (own, +x, -x, +y, -y, +z, -z); mode 1 differs in the last five points only
FLAGS7 = [[1, 1, 1, 0, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0],
          [1, 1, 1, 0, 0, 0, 1], [1, 0, 1, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0],
          [1, 0, 0, 0, 0, 1, 0], [1, 1, 1, 0, 0, 0, 1], [1, 1, 1, 0, 0, 0, 1], [1, 1, 1, 0, 0, 0, 1], [1, 1, 1, 0, 0, 0, 1], [1, 1, 1, 0, 0, 0, 1]]
FLAGS7_MODE1_TAIL = [[3, 3, 3, 0, 0, 0, 3], [5, 5, 5, 0, 0, 0, 5], [1, 5, 1, 0, 0, 0, 1], [5, 5, 1, 0, 0, 0, 5], [5, 1, 5, 0, 0, 0, 1]]


def test_the_stencils_are_the_rules_lists():
    assert sr.stencil(1).tolist() == [[0, 0, 0]]
    assert sr.stencil(7).tolist() == [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    s = sr.stencil(27)
    assert s[0].tolist() == [0, 0, 0] and len({tuple(o) for o in s.tolist()}) == 27 and np.abs(s).max() == 1
    key = (s[1:, 2] * 9 + s[1:, 1] * 3 + s[1:, 0]).tolist()
    assert key == sorted(key) and s[1].tolist() == [-1, -1, -1] and s[26].tolist() == [1, 1, 1] and s[13].tolist() == [-1, 0, 0] and s[14].tolist() == [1, 0, 0]
    for bad in (0, 2, 8, 26):
        with pytest.raises(ValueError):
            sr.stencil(bad)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["lot", "planted", "lattice"])
def test_one_voxel_per_point_is_voxels_ref_bit_for_bit(name, mode):
    S = vs.MAPS[name]()
    T, nrm = ss.pose_of(S), ss.normals_of(S)
    for kind in (0, 2):
        want = vr.linearize(S["vmap"], S["src"], T, mode, nrm, vs.GICP_EPS, kind, 0.7)
        got = sr.linearize(S["vmap"], S["src"], T, mode, nrm, vs.GICP_EPS, kind, 0.7, neighbors=1)
        assert sorted(got) == sorted(want)
        for k in want:
            a, b = np.asarray(got[k]), np.asarray(want[k])
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, mode, kind, k)


def test_the_planted_scene_holds_every_kind_of_correspondence():
    P = ss.planted7()
    assert len(P["src"]) == 18                                             # one wave: the lanes of the asserts below are its lanes
    r0 = sr.linearize(P["vmap"], P["src"], P["T"], 0, P["src_normals"], neighbors=7)
    r1 = sr.linearize(P["vmap"], P["src"], P["T"], 1, P["src_normals"], neighbors=7)
    f0, f1 = r0["flag"], r1["flag"]
    assert f0.tolist() == FLAGS7 and f1.tolist() == FLAGS7[:13] + FLAGS7_MODE1_TAIL
    assert (r0["n_eff"], r0["n_pt"], r1["n_eff"], r1["n_pt"]) == (14, 14, 12, 14)
    # a point whose own voxel is not kept (the small voxel) but a face neighbour is
    assert f0[2].tolist() == [0, 0, 1, 0, 0, 0, 0] and r0["voxel_idx"][2, 0] == -1 and r0["voxel_idx"][2, 2] >= 0
    # points with two or more effective correspondences
    assert ((f0 == 1).sum(axis=1) >= 2).sum() == 11 and (f0[0] == 1).sum() == 4
    # not positive definite beside effective, in one point (mode 1: the three over-long normals)
    assert all((f1[i] == 5).any() and (f1[i] == 1).any() for i in (15, 16, 17))
    # a point without a normal: every found correspondence is flag 3, the others 0
    assert np.array_equal(f1[13] == 3, f0[13] == 1) and not (f1[13] == 1).any() and r1["normal_src"][13].tolist()[1:] == [0.0, 1.0]
    assert not r1["normal_src"][9].any() and not r0["normal_src"].any()  # (no correspondence: no normal is read; mode 0: none at all)
    # the map's voxel box and the points at its low and high edge on every axis: their stencils leave the box
    lo, hi = vs.box_of(P["tgt"])
    assert lo.tolist() == [-1, 0, -1] and hi.tolist() == [6, 2, 0]
    v = vr.voxel_of(P["src"], vs.LEAF).astype(np.int64)
    own = f0[:, 0] == 1
    for a in range(3):
        assert (own & (v[:, a] == lo[a])).any() and (own & (v[:, a] == hi[a])).any(), a
    # within the wave: nobody has a +y or -y neighbour, exactly one lane has a +z neighbour
    assert (r0["voxel_idx"][:, 3] < 0).all() and (r0["voxel_idx"][:, 4] < 0).all() and (r0["voxel_idx"][:, 5] >= 0).sum() == 1
    # S = 27 holds S = 7: the face neighbours are entries 13 14 11 16 5 22 of the block's order
    r27 = sr.linearize(P["vmap"], P["src"], P["T"], 1, P["src_normals"], neighbors=27)
    at = [0, 14, 13, 16, 11, 22, 5]
    for k in ("voxel_idx", "flag", "w", "row"):
        assert np.array_equal(r27[k][:, at], r1[k], equal_nan=True), k
    assert (r27["flag"][12, [21, 22, 23]] == 1).all()                      # an edge and a corner neighbour: -x+z, +z, +x+z
    assert (r27["n_eff"], r27["n_pt"]) == (12, 14)


def test_the_lattice_holds_points_with_all_27_correspondences_effective():
    L = vs.lattice()
    r = sr.linearize(L["vmap"], L["src"], L["T"], 0, L["src_normals"], neighbors=27)
    assert (r["flag"] == 1).all(axis=1).sum() == 481 and (r["n_eff"], r["n_pt"]) == (994, 994)
    one = vr.linearize(L["vmap"], L["src"], L["T"])
    assert r["n_pt"] > one["n_pt"]                                         # points just outside the lattice have neighbours only
    edge = (r["flag"][:, 0] == 0) & (r["flag"] == 1).any(axis=1)
    assert edge.sum() == r["n_pt"] - one["n_pt"]


def test_the_sums_count_points_and_hold_every_effective_row():
    L = vs.lot()
    one = vr.linearize(L["vmap"], L["src"], L["INIT"], 1, L["mb"])
    for S in (7, 27):
        r = sr.linearize(L["vmap"], L["src"], L["INIT"], 1, L["mb"], neighbors=S)
        for k in vs.DUMP_KEYS:
            a = r[k] if k == "normal_src" else r[k][:, 0]
            if k == "normal_src":                                          # (a point that has a neighbour only now shows its normal)
                hit = one["voxel_idx"] >= 0
                assert np.array_equal(a[hit], one[k][hit], equal_nan=True)
            else:
                assert np.array_equal(a, one[k], equal_nan=True), (S, k)
        assert r["n_eff"] >= one["n_eff"] and r["n_pt"] >= one["n_pt"] and r["n_pt"] <= len(L["src"])
        eff = r["flag"] == 1
        assert eff.sum() > r["n_eff"] and not r["row"][~eff].any()
        assert r["sum_r2"] == pytest.approx((r["r"][eff] ** 2).sum(), rel=1e-12)
