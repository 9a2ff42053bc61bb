"""dcreg_p2p_error (metrics.hip) off the symmetric case (run with -m gpu on an MI355X): the device against the brute-force numpy reference
(p2p_ref.py, pinned against the oracle by test_p2p_reference.py) and the oracle itself, on the scenes of p2p_scenes.py.

Tolerances (include/dcreg.h states them; none is measured):
  - forward: the queries and every float d2 are bitwise the reference's - valid and fitness are equal, rmse agrees to 1e-12 (a double sum
    of identical terms in another order), and so does the forward mean, which the call returns only inside chamfer (the "forward term");
  - backward: |device - exact| <= sqrt(3) 2^-24 B + 2^-21 mean, |oracle - exact| <= sqrt(3) 2^-24 G + 2^-21 mean (B, G: the largest
    absolute body-frame / map-frame coordinate, computed from each scene): the device's backward mean, 2 chamfer - forward mean, is
    asserted against the exact mean with the first bound and against the oracle's with the sum; chamfer against the oracle's with half
    the sum, plus the forward term."""
import numpy as np
import pytest

import helpers as h
import p2p_scenes as ps
from dcreg_amd import api
from test_gpu_device_seam import DevCloud, strided

pytestmark = pytest.mark.gpu

LIN_KEYS = ("H_upper", "g", "sum_r2", "sum_b2", "n_eff", "n_pt", "flag", "nn_idx", "nn_d2", "normal", "r", "s")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def assert_p2p(got, ref, orc, thr, what=""):
    rmse, fit, chamfer, valid = got
    r = ref["thr"][thr]
    ormse, ofit, ochamfer, ovalid = orc["thr"][thr]
    fwd = r["fwd_mean_f32"]
    fwd_term = 1e-12 * fwd
    bwd = 2.0 * chamfer - fwd
    both = ref["bound_dev"] + ref["bound_ref"]
    print("%s thr=%r: valid %d/%d rmse %.17g (ref %.17g) chamfer %.17g (oracle %.17g)  backward %.17g: - exact %.3e (bound %.3e), - oracle %.3e "
          "(bound %.3e)" % (what, thr, valid, r["valid"], rmse, r["rmse"], chamfer, ochamfer, bwd, bwd - ref["exact_bwd"], ref["bound_dev"],
                            bwd - orc["bwd_mean"], both))
    assert valid == r["valid"] == ovalid, what
    assert fit == r["fitness"] == ofit, what
    assert np.isclose(rmse, r["rmse"], rtol=1e-12, atol=0.0) and np.isclose(rmse, ormse, rtol=1e-12, atol=0.0), what
    if r["valid"] == 0:
        assert rmse == 0.0 and fit == 0.0, what
    assert abs(bwd - ref["exact_bwd"]) <= ref["bound_dev"] + fwd_term, what
    assert abs(bwd - orc["bwd_mean"]) <= both + fwd_term, what
    assert abs(chamfer - ochamfer) <= both / 2.0 + fwd_term, what


def twice(c, T, thr):
    """the call, twice: the header promises determinism"""
    a, b = c.p2p_error(T, thr), c.p2p_error(T, thr)
    assert a == b, (a, b)
    return a


def _kind(k):
    return [s["name"] for s in ps.all_scenes() if s["kind"] == k]


def _run_scene(ctx, name):
    s, ref, orc = ps.scene(name), ps.reference(name), ps.oracle(name)
    ctx.set_target(s["tgt"], 1.0)
    ctx.set_source(s["src"])
    for thr in s["thrs"]:
        assert_p2p(twice(ctx, s["T"], thr), ref, orc, thr, name)


@pytest.mark.parametrize("name", _kind("asym"))
def test_asymmetric_pair_at_every_pose(ctx, name):
    """ns != nt and forward and backward means a factor of more than two apart (test_p2p_reference.py), at the identity, a near-identity pose,
    an exactly representable one and a large motion whose body frame lies hundreds of metres from the map frame - and with the roles and
    sizes swapped: a normalisation by the wrong cloud, swapped passes or a wrong inverse pose are off by far more than the bounds"""
    _run_scene(ctx, name)


def test_threshold_ties(ctx):
    """distances exactly at the threshold are excluded (the comparison is strict); the float64 neighbours of the threshold, 0, a negative
    threshold (nothing valid: rmse = fitness = 0) and +inf (everything valid)"""
    _run_scene(ctx, "ties")
    s = ps.scene("ties")
    tie, up = ps.TIE_THRESHOLDS[0], ps.TIE_THRESHOLDS[1]
    assert ctx.p2p_error(s["T"], tie)[3] < ctx.p2p_error(s["T"], up)[3]
    assert ctx.p2p_error(s["T"], 0.0)[:2] == (0.0, 0.0) and ctx.p2p_error(s["T"], -1.0)[:2] == (0.0, 0.0)
    assert ctx.p2p_error(s["T"], float("inf"))[3] == len(s["src"])


@pytest.mark.parametrize("name", _kind("reduce"))
def test_reduction_shapes(ctx, name):
    """sizes that leave a ragged last wave or block, a single block, a single point on either side (kBlock is 256, a wave is 64)"""
    _run_scene(ctx, name)


@pytest.mark.parametrize("name", _kind("degenerate"))
def test_degenerate_sources_for_the_auxiliary_grid(ctx, name):
    """the grid of the backward pass over a source of extent 0 on all axes, on two, on one, and over a single point far from the body origin,
    near the map frame and hundreds of metres from it"""
    _run_scene(ctx, name)


def _state_sources():
    tgt = ps.surface_target()
    T = ps.POSES["near"]
    mk = lambda n, n_off, seed, side: ps.to_body(T, ps.half_cover(tgt, n, n_off, seed, side))     # noqa: E731
    return tgt, T, dict(a=mk(500, 20, 31, 1.0), b=mk(650, 30, 32, -1.0), c=mk(300, 10, 33, 1.0), d=mk(1200, 0, 34, -1.0), e=mk(420, 15, 35, 1.0))


def test_state_follows_the_clouds():
    """one context, every call against the reference: the auxiliary grid reused over three poses, rebuilt after every way of setting a source
    (the sources alternate between the two halves of the map: a stale grid is metres off), the shared neighbour buffers grown by a larger
    dcreg_knn in between, and the map changed by dcreg_target_insert and dcreg_target_crop"""
    tgt, T, src = _state_sources()
    thr = 0.05
    c = api.Context(0)
    dev = None
    try:
        def check(s, t, pose, what):
            got = twice(c, pose, thr)
            assert_p2p(got, ps.reference_of(s, t, pose, (thr,)), ps.oracle_of(s, t, pose, (thr,)), thr, what)
            return got
        c.set_target(tgt, 1.0)
        c.set_source(src["a"])
        for k, pose in enumerate((T, np.eye(4), h.pose6d_matrix(-0.2, 0.1, 0.05, 0.0, h.deg2rad(0.3), h.deg2rad(-1.0)) @ T)):
            check(src["a"], tgt, pose, "three poses, pose %d" % k)
        c.set_source(src["b"])
        check(src["b"], tgt, T, "set_source")
        dev = DevCloud(strided(src["c"], 4))
        c.set_source_device(dev.ptr, len(src["c"]), 4)
        check(src["c"], tgt, T, "set_source_device")
        info = c.set_source_voxel(src["d"], 2.0)
        vox = c.voxel_downsample([src["d"]], 2.0)[0][0]
        assert 0 < info["n_out"] == len(vox) < len(src["d"])
        check(vox, tgt, T, "set_source_voxel")
        rec = np.zeros((len(src["e"]), 4), np.float32)
        rec[:, :3] = src["e"]
        rec[:, 3] = np.linspace(0.0, 0.1, len(rec), dtype=np.float32)
        field, still = api.time_field(3), api.sweep_motion(np.eye(3), np.zeros(3), (0.0, float(np.float32(0.1))), 0.5)
        c.set_source_deskew(rec, field, still)
        swept = c.deskew([rec], field, [still])[0][0]                   # (the source is bitwise set_source of this: include/dcreg.h)
        assert np.array_equal(swept, src["e"])
        before = check(src["e"], tgt, T, "set_source_deskew (identity motion)")
        # a k-NN call with more queries than max(ns, nt): the neighbour buffers the two passes share grow
        q = np.random.default_rng(36).uniform(-45, 45, (5000, 3)).astype(np.float32)
        c.knn(q, k=5, max_radius=0.0)
        assert check(src["e"], tgt, T, "after a larger dcreg_knn") == before
        # the map changes under the same source
        extra = ps.to_body(T, ps.half_cover(tgt, 200, 0, 37, -1.0))
        up = c.insert(extra, T, 0.0)
        assert up["n_added"] == 200
        check(src["e"], c.target_points(), T, "after dcreg_target_insert")
        up = c.crop([-45.0, -45.0, -5.0], [45.0, 10.0, 30.0])
        cropped = c.target_points()
        assert up["n_removed"] > 500 and len(cropped) == 3200 - up["n_removed"]
        check(src["e"], cropped, T, "after dcreg_target_crop")
    finally:
        if dev is not None:
            dev.free()
        c.close()


@pytest.mark.parametrize("roi_index", [0, 2])
def test_no_side_effects_on_the_hot_path(roi_index):
    """a walk of four poses on two contexts with the same clouds, a plain and a debug linearisation at each, dcreg_p2p_error and dcreg_knn
    interleaved on one of the contexts: bitwise the same sums and debug arrays.  With the window index forced ("roi_index" 2) the metrics
    switch to the whole map and the next plain linearisation is back on the window"""
    tgt = h.scene_cylinder(4000, seed=41, radius=10.0, height=6.0, noise=0.01)
    rng = np.random.default_rng(42)
    half = np.flatnonzero(tgt[:, 0] > 2.0)
    T0 = ps.POSES["near"]
    src = ps.to_body(T0, tgt[rng.choice(half, 800, replace=False)] + rng.normal(0, 0.01, (800, 3)).astype(np.float32))
    q = rng.uniform(-12, 12, (100, 3)).astype(np.float32)
    prm = api.default_lin_params(1.0, 0)
    plain, busy = api.Context(0), api.Context(0)
    try:
        for c in (plain, busy):
            c.set_option("roi_index", roi_index)
            c.set_option("roi_margin", 1.0)                 # (the source covers x > 2 of a map 20 m across: the window leaves part of it out)
            c.set_target(tgt, 1.0)
            c.set_source(src)
        want = None
        for k, (dx, dy, dz, yaw) in enumerate(((0, 0, 0, 0), (0.02, -0.01, 0.0, 0.001), (0.05, 0.03, -0.01, 0.003), (0.02, -0.01, 0.0, 0.001))):
            T = T0 @ h.pose6d_matrix(dx, dy, dz, 0.0, 0.0, yaw)
            # the sums of a plain launch (on the window, where one is forced), then - after the metrics - the debug arrays (a debug launch
            # always runs on the whole map: include/dcreg.h)
            a, b = plain.linearize(T[:3, :3], T[:3, 3], prm), busy.linearize(T[:3, :3], T[:3, 3], prm)
            assert a["n_eff"] > 100
            same_lin(a, b, LIN_KEYS[:6], k)
            if roi_index == 2:
                assert busy.roi_info()["active"] and 0 < busy.roi_info()["points"] < len(tgt)
            got = busy.p2p_error(T, 0.3)
            if roi_index == 2:
                assert not busy.roi_info()["active"]
            if k == 0:
                want = got
                assert_p2p(got, ps.reference_of(src, tgt, T, (0.3,)), ps.oracle_of(src, tgt, T, (0.3,)), 0.3, "walk, roi_index %d" % roi_index)
            busy.knn(q, k=5, max_radius=0.0)
            a = plain.linearize(T[:3, :3], T[:3, 3], prm, debug=True)
            b = busy.linearize(T[:3, :3], T[:3, 3], prm, debug=True)
            same_lin(a, b, LIN_KEYS, k)
            busy.knn(q, k=1, max_radius=2.0)
        T = T0
        assert busy.p2p_error(T, 0.3) == want == plain.p2p_error(T, 0.3)
    finally:
        plain.close()
        busy.close()


def same_lin(a, b, keys, what):
    for key in keys:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key)


def _bad_rotations(T):
    scaled, mirrored, sheared = T.copy(), T.copy(), T.copy()
    scaled[:3, :3] *= 1.01
    mirrored[:3, :3] = np.diag([1.0, 1.0, -1.0]) @ T[:3, :3]
    sheared[0, 1] += 0.01
    return dict(scaled=scaled, mirrored=mirrored, sheared=sheared)


def test_refusals():
    """a pose with a non-finite entry in its top three rows, or whose rotation block is not a rotation, is refused with DCREG_E_INVALID on the
    host; no source or no target is DCREG_E_STATE; after every refusal a valid call returns what a fresh context returns.  The bottom row
    is ignored."""
    s = ps.scene("asym_near")
    T, thr = s["T"], s["thrs"][0]
    fresh, c, empty = api.Context(0), api.Context(0), api.Context(0)
    try:
        fresh.set_target(s["tgt"], 1.0)
        fresh.set_source(s["src"])
        want = fresh.p2p_error(T, thr)
        assert_p2p(want, ps.reference("asym_near"), ps.oracle("asym_near"), thr, "fresh")
        # no clouds
        with pytest.raises(api.DcregError, match=r"\(-4\)"):
            empty.p2p_error(T, thr)
        empty.set_target(s["tgt"], 1.0)
        with pytest.raises(api.DcregError, match=r"\(-4\)"):
            empty.p2p_error(T, thr)
        empty.set_source(s["src"])
        assert empty.p2p_error(T, thr) == want
        only_source = api.Context(0)
        try:
            only_source.set_source(s["src"])
            with pytest.raises(api.DcregError, match=r"\(-4\)"):
                only_source.p2p_error(T, thr)
            only_source.set_target(s["tgt"], 1.0)
            assert only_source.p2p_error(T, thr) == want
        finally:
            only_source.close()
        # poses
        c.set_target(s["tgt"], 1.0)
        c.set_source(s["src"])
        assert c.p2p_error(T, thr) == want
        bad = []
        for k in range(12):
            for v in (np.nan, np.inf, -np.inf):
                B = T.copy().reshape(16)
                B[k] = v
                bad.append(("entry %d = %r" % (k, v), B, "non-finite"))
        bad += [(name, B.reshape(16), "not a rotation") for name, B in _bad_rotations(T).items()]
        for name, B, msg in bad:
            with pytest.raises(api.DcregError, match=r"\(-1\).*" + msg):
                c.p2p_error(B, thr)
            assert c.p2p_error(T, thr) == want, name
        # the bottom row is not looked at
        for v in (np.nan, np.inf, 7.0):
            B = T.copy()
            B[3, :] = v
            assert c.p2p_error(B, thr) == want
        # the edge of the rule: a rotation block off by 1e-9 is a rotation
        B = T.copy()
        B[0, 1] += 1e-9
        c.p2p_error(B, thr)
        assert c.p2p_error(T, thr) == want
    finally:
        for x in (fresh, c, empty):
            x.close()
