"""The numpy reference of dcreg_p2p_error (p2p_ref.py) against the oracle on every scene of test_gpu_p2p_error.py, and the conditions each
scene must meet to exercise its edge (no GPU).  The GPU tests compare the device with this reference; here the reference itself is
pinned, and a scene that quietly stops being asymmetric, tied or ragged fails here."""
import numpy as np
import pytest

import p2p_ref as pr
import p2p_scenes as ps


@pytest.mark.parametrize("name", ps.scene_names())
def test_reference_matches_oracle(name):
    """valid and fitness exactly, rmse to 1e-12; the forward mean: the float terms to 1e-12, the float64 distances within 2^-21 of the mean
    (float d2 arithmetic and sqrtf); the backward mean: the oracle rounds T p to float in the map frame, within the map-frame bound of
    include/dcreg.h of the exact mean"""
    s, ref, orc = ps.scene(name), ps.reference(name), ps.oracle(name)
    for thr in s["thrs"]:
        r = ref["thr"][thr]
        ormse, ofit, ochamfer, ovalid = orc["thr"][thr]
        assert r["valid"] == ovalid and r["fitness"] == ofit, thr
        assert np.isclose(r["rmse"], ormse, rtol=1e-12, atol=0.0), thr
        if ovalid == 0:
            assert r["rmse"] == 0.0 and r["fitness"] == 0.0
        assert np.isclose(ochamfer, (orc["fwd_mean"] + orc["bwd_mean"]) / 2.0, rtol=1e-12, atol=0.0)      # the oracle's own two halves
    r = ref["thr"][s["thrs"][0]]
    assert np.isclose(r["fwd_mean_f32"], orc["fwd_mean"], rtol=1e-12, atol=0.0)
    assert abs(r["fwd_mean"] - orc["fwd_mean"]) <= 2.0 ** -21 * r["fwd_mean"]
    assert abs(orc["bwd_mean"] - ref["exact_bwd"]) <= ref["bound_ref"]
    assert abs(r["bwd_mean"] - ref["exact_bwd"]) <= ref["bound_ref"]           # float64 distances to the float-rounded T p: the same bound


def test_transform_rounds_as_the_device_does():
    """element-wise float64 in the order ((R0 x + R1 y) + R2 z) + t, one rounding to float32: a hand-computed point, and exactness at the
    exactly representable pose"""
    T = ps.POSES["large"]
    p = np.array([[1.5, -2.25, 3.125]], np.float32)
    want = [np.float32(((T[a, 0] * 1.5 + T[a, 1] * -2.25) + T[a, 2] * 3.125) + T[a, 3]) for a in range(3)]
    got = pr.transform(T, p)
    assert got.dtype == np.float32 and np.array_equal(got[0], np.array(want, np.float32))
    s = ps.scene("ties")
    assert np.array_equal(pr.transform(s["T"], s["src"]).astype(np.float64), pr.transform_exact(s["T"], s["src"]))


def test_poses_are_rigid_and_as_the_scenes_need_them():
    for name, T in ps.POSES.items():
        R = T[:3, :3]
        assert np.max(np.abs(R.T @ R - np.eye(3))) < 1e-15 and np.linalg.det(R) > 0, name
        assert np.allclose(pr.rigid_inverse(T) @ T, np.eye(4), atol=1e-12)
    assert np.array_equal(ps.POSES["identity"], np.eye(4))
    assert 0 < np.max(np.abs(ps.POSES["near"] - np.eye(4))) < 0.05
    L = ps.POSES["large"]
    assert np.isclose(np.arccos((np.trace(L[:3, :3]) - 1) / 2), 2.5) and np.array_equal(L[:3, 3], [120.0, -340.0, 15.0])
    assert np.allclose(L[:3, :3] @ (np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)), np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))


@pytest.mark.parametrize("pose", list(ps.POSES))
def test_asymmetric_pair_is_asymmetric(pose):
    """ns != nt, the forward and backward means differ by more than a factor of two in both arrangements (a swapped normalisation or a swapped
    pass moves the Chamfer distance far outside tolerance), and the threshold splits the source"""
    for swapped in (False, True):
        s = ps.scene("asym_%s%s" % (pose, "_swapped" if swapped else ""))
        r = ps.reference(s["name"])["thr"][s["thrs"][0]]
        assert (r["ns"], r["nt"]) == ((3000, 700) if swapped else (700, 3000))
        hi, lo = max(r["fwd_mean"], r["bwd_mean"]), min(r["fwd_mean"], r["bwd_mean"])
        assert lo > 0 and hi > 2.0 * lo
        assert (r["fwd_mean"] > r["bwd_mean"]) == swapped
        assert 0 < r["valid"] < r["ns"]
        # dividing the backward sum by ns where nt belongs moves the Chamfer distance by far more than the tolerance
        ref = ps.reference(s["name"])
        assert abs(r["bwd_mean"] * r["nt"] / r["ns"] - r["bwd_mean"]) / 2.0 > 1e3 * (ref["bound_dev"] + ref["bound_ref"])


def test_large_motion_scene_is_far_from_the_map_frame_and_overlaps_the_map():
    s = ps.scene("asym_large")
    r = ps.reference("asym_large")["thr"][s["thrs"][0]]
    assert np.min(np.linalg.norm(s["src"].astype(np.float64), axis=1)) > 300.0          # the body frame: hundreds of metres away
    assert np.max(np.abs(s["tgt"])) < 45.0 and r["fwd_mean"] < 1.0                        # the aligned cloud lies on the map
    # a wrong inverse pose (no transpose, or no minus sign) moves the backward queries by metres
    T = s["T"]
    for Pi_R, Pi_t in ((T[:3, :3], -(T[:3, :3].T @ T[:3, 3])), (T[:3, :3].T, T[:3, :3].T @ T[:3, 3])):
        q = s["tgt"][:200].astype(np.float64) @ Pi_R.T + Pi_t
        wrong = np.mean(pr.nn_dist_f64(q, s["src"].astype(np.float64)))
        assert abs(wrong - r["bwd_mean"]) > 1.0


def test_tie_scene_has_exact_ties():
    """at the exactly representable pose every aligned point is a lattice point plus a dyadic offset: the float d2 are exact, points sit at
    exactly the tie distances, and the count changes between a tie threshold and its float64 neighbour above"""
    s, ref = ps.scene("ties"), ps.reference("ties")
    ns = len(s["src"])
    d2 = ref["thr"][s["thrs"][0]]["d2_f32"]
    want = np.concatenate([np.full(30 + 3 * k, float(np.dot(o, o))) for k, o in enumerate(ps.TIE_OFFSETS)])
    assert np.array_equal(d2.astype(np.float64), want)
    for tie in (ps.TIE_DISTANCE, ps.TIE_DISTANCE_2):
        assert np.float32(tie) == tie and np.count_nonzero(d2 == np.float32(tie * tie)) >= 30
        up, down = float(np.nextafter(tie, np.inf)), float(np.nextafter(tie, -np.inf))
        at = ref["thr"][tie]["valid"]
        assert 0 < at < ns
        assert ref["thr"][up]["valid"] == at + np.count_nonzero(d2 == np.float32(tie * tie))     # the tied points are excluded at the tie
        if tie == ps.TIE_DISTANCE:
            assert ref["thr"][down]["valid"] == at
    for none in (0.0, -1.0):
        assert ref["thr"][none]["valid"] == 0 and ref["thr"][none]["rmse"] == 0.0 and ref["thr"][none]["fitness"] == 0.0
    assert ref["thr"][float("inf")]["valid"] == ns
    assert set(ps.TIE_THRESHOLDS) == set(s["thrs"]) and len(s["thrs"]) == 8


def test_reduction_shapes_cover_the_ragged_sizes():
    ns = sorted(a for a, _ in ps.REDUCTION_SHAPES)
    nt = sorted(b for _, b in ps.REDUCTION_SHAPES)
    assert ns == nt == sorted(ps.REDUCTION_SIZES) == [1, 2, 4, 63, 64, 65, 255, 256, 257, 513]
    for must in ((1, 513), (513, 1), (256, 256)):
        assert must in ps.REDUCTION_SHAPES
    for a, b in ps.REDUCTION_SHAPES:
        s = ps.scene("reduce_%d_%d" % (a, b))
        assert (len(s["src"]), len(s["tgt"])) == (a, b)
        assert s["src"].min() >= 0 and s["src"].max() <= 2 and s["tgt"].min() >= 0 and s["tgt"].max() <= 2
    # the threshold splits at least the larger sources
    r = ps.reference("reduce_513_1")["thr"][0.3]
    assert 0 < r["valid"] < 513


@pytest.mark.parametrize("pose", ["near", "large"])
def test_degenerate_sources_are_degenerate(pose):
    ext = {w: np.ptp(ps.scene("degenerate_%s_%s" % (w, pose))["src"], axis=0) for w in ps.DEGENERATE}
    assert np.array_equal(ext["identical"], [0, 0, 0]) and len(ps.scene("degenerate_identical_%s" % pose)["src"]) == 300
    assert ext["collinear"][0] > 20 and np.array_equal(ext["collinear"][1:], [0, 0])
    assert ext["coplanar"][0] > 20 and ext["coplanar"][1] > 20 and ext["coplanar"][2] == 0
    single = ps.scene("degenerate_single_%s" % pose)["src"]
    assert single.shape == (1, 3) and np.linalg.norm(single[0]) > (300.0 if pose == "large" else 30.0)
    for w in ps.DEGENERATE:
        assert len(ps.scene("degenerate_%s_%s" % (w, pose))["tgt"]) == 3000
