"""Kept normals that follow the map (option "normals_follow", dcreg_target_normals_get, dcreg_target_normals_follow_info).  The yardstick
for bits is a FRESH context given set_target(c.target_points()) + keep_target_normals(p): that path is pinned to the numpy reference by
tests/test_gpu_normals.py, and one case here is compared with the reference of the updated cloud directly.  Every comparison is bitwise;
nothing has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import normal_icp_scenes as sc
import normals_ref as nr
from dcreg_amd import api
from test_gpu_normals import OPTS_WINDOW
from test_gpu_visibility import pose, shell
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
I4 = np.eye(4)
P5 = dict(k=5)
PARAM_SETS = {"k5": P5, "k5-radius": dict(k=5, search_radius=RADIUS), "k12": dict(k=12), "no-orient": dict(k=5, viewpoint=None),
              "viewpoint": dict(k=5, viewpoint=(-110.0, -395.0, 6.0))}


def ctx(tgt, src, p, opts=(), follow=1):
    c = api.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_option("normals_follow", follow)
    c.set_target(tgt, RADIUS)
    if src is not None:
        c.set_source(src)
    if p is not None:
        c.keep_target_normals(p)
    return c


def oracle(c, p, opts=(), src=None):
    """a fresh context with the same options that holds c's map and the normals keep_target_normals gives it"""
    return ctx(c.target_points(), src, p, opts, follow=0)


def assert_same_normals(got, want, what=""):
    assert got[0].shape == want[0].shape and sc.same_bits(got[0], want[0]) and sc.same_bits(got[1], want[1]), what


def assert_follows(c, p, opts=(), what="", n_added=None):
    """the kept normals are bitwise the oracle's, and the info adds up -> info"""
    assert c.target_normals_kept() == 1, what
    o = oracle(c, p, opts)
    try:
        assert_same_normals(c.kept_target_normals(), o.kept_target_normals(), what)
    finally:
        o.close()
    info = c.normals_follow_info()
    n = len(c.target_points())
    assert info["followed"] in (1, 2) and info["n_target"] == n and info["n_refit"] + info["n_carried"] == n, (what, info)
    if n_added is not None:
        assert info["n_refit"] >= n_added, (what, info)
    return info


def patch(centre, n, seed, size=1.0):
    """n points on a size x size square around centre, 1 cm of height noise"""
    rng = np.random.default_rng(7700 + seed)
    return (np.asarray(centre, np.float64) + np.c_[rng.uniform(-0.5 * size, 0.5 * size, (n, 2)), rng.normal(0.0, 0.01, n)]).astype(np.float32)


def lot_middle():
    """the map point of the lot nearest to the middle of its box"""
    tgt = sc.lot()["tgt"]
    mid = 0.5 * (tgt.min(axis=0).astype(np.float64) + tgt.max(axis=0))
    return tgt[np.argmin(((tgt - mid) ** 2).sum(axis=1))]


def crop_box(tgt):
    return tgt.min(axis=0) + np.float32([3, 3, -1]), tgt.max(axis=0) - np.float32([3, 3, -1])


# ---- 1. an insert
@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_an_insert_refits_what_changed_and_carries_the_rest(name):
    L = sc.lot()
    p = api.normal_params(**PARAM_SETS[name])
    c = ctx(L["tgt"], L["src"], p)
    try:
        if name == "k5-radius":
            assert sc.same_bits(c.kept_target_normals()[0], L["nb"]) and sc.same_bits(c.kept_target_normals()[1], L["curb"])
        u = c.insert_source(L["GT"], 0.05)
        assert u["n_added"] == 53 and u["n_target"] == 4053
        info = assert_follows(c, p, what=name, n_added=53)
        print("%s: %s" % (name, info))
        if name == "k5":                                   # ... and the numpy reference of the updated cloud itself
            want = nr.normals_reference(c.target_points(), k=5)
            assert_same_normals(c.kept_target_normals(), (want["normals"], want["curvature"]), "reference")
    finally:
        c.close()


# ---- 2. a crop
def test_a_crop_renumbers_the_carried_normals():
    L = sc.lot()
    p = api.normal_params(**P5)
    c = ctx(L["tgt"], None, p)
    try:
        u = c.crop(*crop_box(L["tgt"]))
        assert u["n_target"] == 2304 and u["n_removed"] == 1696
        info = assert_follows(c, p, what="crop")
        print(info)
    finally:
        c.close()


# ---- 3. the filters
def test_remove_outliers_is_followed():
    L = sc.lot()
    p = api.normal_params(**P5)
    c = ctx(L["tgt"], None, p)
    try:
        r = c.remove_outliers(api.outlier_params("radius", radius=0.3, min_neighbors=3))
        assert 0 < r["n_out"] < 4000 and len(c.target_points()) == r["n_out"]
        print(assert_follows(c, p, what="remove_outliers"))
    finally:
        c.close()


def test_remove_dynamic_is_followed():
    L = sc.lot()
    p = api.normal_params(**P5)
    centre = 0.5 * (L["tgt"].min(axis=0).astype(np.float64) + L["tgt"].max(axis=0))
    store = [shell(4000, 40 + k, r_lo=10.0, r_hi=30.0, el=0.6) for k in range(3)]           # three sensors above the lot that see beyond it
    members = []
    for k in range(3):
        T = pose(k)
        T[:3, 3] += centre + [0.0, 0.0, 1.5]
        members.append((k, T))
    c = ctx(L["tgt"], None, p)
    try:
        c.keyframes_reset()
        assert c.keyframes_add(store) == 0
        r = c.remove_dynamic(members, api.visibility_params(rows=16, cols=64))
        assert 0 < r["n_flagged"] and 0 < r["n_out"] < 4000 and len(c.target_points()) == r["n_out"]
        print(assert_follows(c, p, what="remove_dynamic"))
    finally:
        c.close()


# ---- 4. a sequence on one context
def run_sequence(c, p, opts, merged):
    L = sc.lot()
    tgt = L["tgt"]
    u = c.insert_source(L["GT"], 0.05)                                     # into the current grid
    assert u["n_added"] == 53 and (merged is None or u["rebuilt"] == (0 if merged else 1))
    assert_follows(c, p, opts, "merged insert", 53)
    far = patch([tgt[:, 0].max() + 30.0, tgt[:, 1].mean(), tgt[:, 2].mean()], 60, 1)
    u = c.insert(far, I4)                                                  # outside the grid's box: the grid is derived again
    assert u["n_added"] == 60 and u["rebuilt"] == 1
    assert_follows(c, p, opts, "insert outside the box", 60)
    u = c.crop(*crop_box(tgt))
    assert 0 < u["n_removed"] and u["n_target"] < 4113
    assert_follows(c, p, opts, "crop")
    u = c.insert(sc.sized_source(257), L["GT"])
    assert u["n_added"] == 257
    assert_follows(c, p, opts, "insert after the crop", 257)


@pytest.mark.parametrize("map_update", [1, 0])
def test_a_sequence_of_updates_is_the_oracle_after_every_step(map_update):
    L = sc.lot()
    p = api.normal_params(**P5)
    opts = [("map_update", map_update)]
    c = ctx(L["tgt"], L["src"], p, opts)
    try:
        run_sequence(c, p, opts, merged=bool(map_update))
    finally:
        c.close()


def test_the_sequence_with_the_window_index_active():
    L = sc.lot()
    p = api.normal_params(k=5, search_radius=RADIUS)
    c = ctx(L["tgt"], L["src"], p, OPTS_WINDOW)
    try:
        c.linearize_normals(L["INIT"], api.default_lin_params(RADIUS, 1))
        assert c.roi_info()["active"]
        run_sequence(c, p, OPTS_WINDOW, merged=None)               # (a capped table: either path may serve)
        c.linearize_normals(L["INIT"], api.default_lin_params(RADIUS, 1))
        assert c.roi_info()["active"]                                      # ... and once more from behind a window
        u = c.insert(patch(lot_middle(), 40, 2), I4)
        assert u["n_added"] == 40
        assert_follows(c, p, OPTS_WINDOW, "insert behind a window", 40)
    finally:
        c.close()


# ---- 5. the boundaries of the dirty list
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_inserts_across_wave_and_block_boundaries(n):
    L = sc.lot()
    p = api.normal_params(**P5)
    c = ctx(L["tgt"], None, p)
    try:
        u = c.insert(patch(lot_middle(), n, 3), I4)
        assert u["n_added"] == n
        print(assert_follows(c, p, what=n, n_added=n))
    finally:
        c.close()


# ---- 6. ties
def test_duplicates_of_a_point_and_a_crop_beside_them():
    L = sc.lot()
    p = api.normal_params(**P5)
    P = lot_middle()
    c = ctx(L["tgt"], None, p)
    try:
        u = c.insert(np.repeat(P[None], 8, axis=0), I4, 0.0)
        assert u["n_added"] == 8
        assert_follows(c, p, what="duplicates", n_added=8)
        lo, hi = L["tgt"].min(axis=0) - 1.0, L["tgt"].max(axis=0) + 1.0
        hi[0] = P[0] + np.float32(0.3)                                     # everything 0.3 m beyond the point in x goes
        u = c.crop(lo, hi)
        assert 0 < u["n_removed"] < 4008
        assert_follows(c, p, what="crop beside the duplicates")
    finally:
        c.close()


def test_a_point_at_exactly_the_kth_distance_changes_no_set():
    m = sc.lattice_case()["tgt"]                                           # spacing 0.25, exact in float; x = 0 is a face of it
    p = api.normal_params(**P5)
    q = int(np.flatnonzero((m[:, 0] == 0.0) & (m[:, 1] == 0.5) & (m[:, 2] == 0.5))[0])
    d2 = nr.d2_f32(m[q][None], m)[0]
    assert np.sort(d2)[4] == np.float32(0.0625)                            # its 5th neighbour (itself first) is a lattice step away
    new = (m[q] - np.float32([0.25, 0.0, 0.0]))[None]                      # ... and so is the new point: it loses the tie on the index
    assert nr.d2_f32(m[q][None], new)[0, 0] == np.float32(0.0625)
    c = ctx(m, None, p)
    try:
        before = c.kept_target_normals()
        u = c.insert(new, I4)
        assert u["n_added"] == 1
        assert_follows(c, p, what="tie", n_added=1)
        after = c.kept_target_normals()
        assert sc.same_bits(after[0][q], before[0][q]) and sc.same_bits(after[1][q], before[1][q])
    finally:
        c.close()


# ---- 7. locality
def test_two_far_patches_refit_their_surroundings_only():
    rng = np.random.default_rng(77)
    gx, gy = np.meshgrid(np.arange(101) * 0.2, np.arange(101) * 0.2, indexing="ij")
    plane = np.c_[400.0 + gx.ravel() + rng.uniform(-0.05, 0.05, gx.size), gy.ravel() + rng.uniform(-0.05, 0.05, gx.size),
                  rng.normal(0.0, 0.01, gx.size)].astype(np.float32)
    p = api.normal_params(**P5)
    c = ctx(plane, None, p)
    try:
        two = np.concatenate([patch([400.5, 0.5, 0.0], 100, 4), patch([419.5, 19.5, 0.0], 100, 5)])      # their box is the whole map
        u = c.insert(two, I4)
        assert u["n_added"] == 200 and u["n_target"] == 10401
        info = assert_follows(c, p, what="locality", n_added=200)
        print(info)
        assert info["followed"] == 1 and info["n_refit"] <= info["n_target"] // 10, info
    finally:
        c.close()


# ---- 8. the engines
def values(o):
    if isinstance(o, C.Structure):
        return tuple(values(getattr(o, f[0])) for f in o._fields_)
    if isinstance(o, C.Array):
        return tuple(values(x) for x in o)
    return np.float64(o).tobytes() if isinstance(o, float) else o


def timeless(res, logs):
    res.time_ms = 0.0
    for g in logs:
        g.iter_time_ms = 0.0
    return values(res), [values(g) for g in logs]


def test_the_engines_on_followed_normals_are_the_oracles():
    L = sc.lot()
    p = api.normal_params(**P5)
    cfg = cfg_pk01()
    prm = api.default_lin_params(RADIUS, 1)
    c = ctx(L["tgt"], L["src"], p)
    try:
        c.insert_source(L["GT"], 0.05)
        assert c.normals_follow_info()["followed"] in (1, 2)
        o = oracle(c, p, src=L["src"])
        try:
            got, want = c.linearize_normals(L["INIT"], prm, debug=True), o.linearize_normals(L["INIT"], prm, debug=True)
            sc.assert_dump_bitwise(got, want)
            sc.assert_sums_bitwise(got, want)
            assert timeless(*c.icp_run_normals(L["INIT"], "Ours", cfg)) == timeless(*o.icp_run_normals(L["INIT"], "Ours", cfg))
            frames, T0s = [L["src"]] * 4, np.stack([L["INIT"]] * 4)
            a, b = c.register_frames_normals(frames, T0s, "Ours", cfg), o.register_frames_normals(frames, T0s, "Ours", cfg)
            assert len(a) == len(b) == 4
            for ra, rb in zip(a, b):
                assert ra.iterations > 1 and timeless(ra, [])[0] == timeless(rb, [])[0]
        finally:
            o.close()
    finally:
        c.close()


# ---- 9. what does not follow
def test_what_drops_the_normals_still_drops_them():
    L = sc.lot()
    p = api.normal_params(**P5)
    c = ctx(L["tgt"], L["src"], p, follow=0)
    try:
        c.insert_source(L["GT"], 0.05)                                     # the option at 0: as before
        info = c.normals_follow_info()
        assert c.target_normals_kept() == 0 and info["followed"] == 0 and info["n_target"] == 4053
        with pytest.raises(api.DcregError) as e:
            c.kept_target_normals()
        assert "(%d)" % api.E_STATE in str(e.value)
        c.set_option("normals_follow", 1)                                  # given normals have no rule to refit with
        c.set_target_normals(np.tile(np.float32([0, 0, 1]), (4053, 1)))
        c.insert(patch(lot_middle(), 10, 6), I4)
        assert c.target_normals_kept() == 0 and c.normals_follow_info()["followed"] == 0
        c.keep_target_normals(p)                                           # a new map
        c.set_target(L["tgt"], RADIUS)
        assert c.target_normals_kept() == 0 and c.normals_follow_info()["followed"] == 0
        c.keep_target_normals(p)                                           # the option is read at the time of the update
        c.set_option("normals_follow", 0)
        c.insert(patch(lot_middle(), 10, 6), I4)
        assert c.target_normals_kept() == 0
        assert c._L.dcreg_target_normals_follow_info(c._h, None) == api.E_INVALID
    finally:
        c.close()


def test_updates_that_change_nothing_and_refused_updates_leave_every_bit():
    L = sc.lot()
    p = api.normal_params(**P5)
    c = ctx(L["tgt"], L["src"], p)
    try:
        c.insert(patch(lot_middle(), 30, 7), I4)
        base, info = c.kept_target_normals(), c.normals_follow_info()
        assert info["followed"] in (1, 2)

        def untouched(what):
            assert c.target_normals_kept() == 1 and c.normals_follow_info() == info, what
            assert_same_normals(c.kept_target_normals(), base, what)
        assert c.insert_source(L["GT"], 100.0)["n_added"] == 0             # everything thinned away
        untouched("thinned insert")
        assert c.crop(L["tgt"].min(axis=0) - 50.0, L["tgt"].max(axis=0) + 50.0)["n_removed"] == 0
        untouched("a crop around everything")
        bad = np.eye(4)
        bad[0, 3] = np.nan
        R, t = api._pose_rt(bad, "insert_source")                          # (straight to the library: it refuses)
        assert c._L.dcreg_target_insert_source(c._h, api._dp(R), api._dp(t), 0.0, None) == api.E_INVALID
        untouched("a non-finite pose")
        with pytest.raises(api.DcregError):
            c.crop([1e6, 1e6, 1e6], [2e6, 2e6, 2e6])                       # keeps nothing
        untouched("a crop that keeps nothing")
        small = np.zeros((4, 4), np.float32)                               # the capacity protocol of the getter
        assert c._L.dcreg_target_normals_get(c._h, small.ctypes.data, 4) == api.E_INVALID
        assert c._L.dcreg_target_normals_get(c._h, None, 1 << 20) == api.E_INVALID
        untouched("refused reads")
    finally:
        c.close()
