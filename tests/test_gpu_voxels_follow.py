"""The kept voxel map that follows the map (option "voxels_follow", dcreg_target_voxels_follow_info).  Two yardsticks, both bitwise: a
FRESH context given set_target(c.target_points()) + keep_target_voxels(params) - that path is pinned to the numpy reference by
tests/test_gpu_voxels.py - and voxels_ref.voxel_map of the updated cloud directly.  The info's counts are derived in numpy from the
changed points' voxels.  Nothing has a tolerance."""
import numpy as np
import pytest

import normal_icp_scenes as sc
import voxels_ref as vr
import voxels_scenes as vs
from dcreg_amd import api
from test_gpu_normals import OPTS_WINDOW
from test_gpu_normals_follow import crop_box, patch, timeless
from test_gpu_visibility import pose, shell
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
I4 = np.eye(4)
PARAMS = (vs.LEAF, vs.EPS, vs.MIN_POINTS)
INFO_KEYS = ("n_points", "n_voxels", "n_small", "n_degenerate", "n_kept")
ZERO = dict(n_target=0, n_touched=0, n_refit=0, n_carried=0, n_kept=0, followed=0)
BIG = 1.0e6
INCREMENTAL = [("voxels_follow_full_share", 1.0)]       # a small map is past the default share at once: the incremental path is what these tests are about


def ctx(tgt, src=None, params=PARAMS, opts=(), follow=1, src_normals=None):
    c = api.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_option("voxels_follow", follow)
    c.set_target(tgt, RADIUS)
    if src is not None:
        c.set_source(src)
    if src_normals is not None:
        c.set_source_normals(np.ascontiguousarray(src_normals, np.float32))
    if params is not None:
        c.keep_target_voxels(api.voxel_map_params(*params))
    return c


def fresh(c, params=PARAMS, src=None, src_normals=None):
    """a fresh context that holds c's map and what keep_target_voxels gives it"""
    return ctx(c.target_points(), src, params, follow=0, src_normals=src_normals)


def voxel_set(xyz, leaf):
    return set(map(tuple, vr.voxel_of(xyz, leaf).astype(np.int64)))


def expected_info(old, new, changed, params=PARAMS):
    """the info of an incremental follow from the map before, the map after and the points that came or went"""
    touched = voxel_set(changed, params[0])
    kept_before = set(map(tuple, vr.voxel_map(old, *params)["coords"]))
    return dict(n_target=len(new), n_touched=len(touched), n_refit=len(touched & voxel_set(new, params[0])), n_carried=len(kept_before - touched),
                n_kept=vr.voxel_map(new, *params)["n_kept"], followed=1)


def assert_follows(c, params=PARAMS, what="", followed=(1, 2), want=None):
    """the member is bitwise the fresh context's and the reference's; -> info"""
    pts = c.target_points()
    ref = vr.voxel_map(pts, *params)
    assert c.target_voxels_kept() == ref["n_kept"] > 0, what
    got = c.kept_target_voxels()
    vs.assert_map_bitwise(got, ref, (what, "reference"))
    o = fresh(c, params)
    try:
        assert o.target_voxels_kept() == c.target_voxels_kept(), what
        vs.assert_map_bitwise(got, o.kept_target_voxels(), (what, "fresh context"))
    finally:
        o.close()
    info = c.voxels_follow_info()
    assert info["followed"] in followed and info["n_target"] == len(pts) and info["n_kept"] == ref["n_kept"], (what, info)
    if info["followed"] == 1:
        assert info["n_refit"] <= info["n_touched"] and 0 <= info["n_kept"] - info["n_carried"] <= info["n_refit"], (what, info)
    if want is not None:
        assert info == want, (what, info, want)
    return info


def crop_changed(old, new, lo, hi):
    """the points a crop removed (the survivors keep their order)"""
    inside = ((old.astype(np.float64) >= np.asarray(lo, np.float64)) & (old.astype(np.float64) <= np.asarray(hi, np.float64))).all(axis=1)
    assert old[inside].tobytes() == new.tobytes()
    return old[~inside]


def in_voxel(rng, v, n):
    return (np.asarray(v, np.float64) + rng.uniform(0.1, 0.9, (n, 3))).astype(np.float32)


# ---- 1. the lot: an insert, then a crop
def test_an_insert_and_a_crop_of_the_lot_refit_the_touched_voxels_and_carry_the_rest():
    L = vs.lot()
    c = ctx(L["tgt"], L["src"])
    try:
        vs.assert_map_bitwise(c.kept_target_voxels(), L["vmap"])
        assert c.voxels_follow_info() == ZERO                              # no update yet
        u = c.insert_source(L["GT"], 0.05)
        assert u["n_added"] == 53 and u["n_target"] == 4053
        new = c.target_points()
        info = assert_follows(c, what="insert", want=expected_info(L["tgt"], new, new[4000:]))
        print("insert:", info)
        lo, hi = crop_box(L["tgt"])
        assert c.crop(lo, hi)["n_removed"] > 0                             # ... and a crop of the map the insert left
        after = c.target_points()
        info = assert_follows(c, what="crop after the insert", want=expected_info(new, after, crop_changed(new, after, lo, hi)))
        print("crop after the insert:", info)
    finally:
        c.close()
    c = ctx(L["tgt"])                                                      # the crop the normals' follow pins, of the lot itself
    try:
        u = c.crop(lo, hi)
        assert u["n_target"] == 2304 and u["n_removed"] == 1696
        after = c.target_points()
        info = assert_follows(c, what="crop", want=expected_info(L["tgt"], after, crop_changed(L["tgt"], after, lo, hi)))
        print("crop:", info)
    finally:
        c.close()


# ---- 2. one voxel of every kind
def planted_additions():
    rng = np.random.default_rng(2025)
    return np.concatenate([in_voxel(rng, (2, 0, 0), 1),                    # the small voxel becomes kept
                           in_voxel(rng, (4, 0, 0), 3),                    # the degenerate voxel becomes kept
                           in_voxel(rng, (-3, 0, 0), 6),                   # a new kept voxel below the minimum: every carried key is rewritten
                           in_voxel(rng, (0, 0, 0), 2),                    # a kept record changes
                           in_voxel(rng, (8, 0, 0), 3)])                   # a new small voxel


def test_planted_one_insert_changes_a_voxel_of_every_kind():
    P = vs.planted()
    assert (P["vmap"]["n_voxels"], P["vmap"]["n_kept"]) == (8, 6)
    add = planted_additions()
    want = vr.voxel_map(np.concatenate([P["tgt"], add]), *PARAMS)
    assert [want[k] for k in INFO_KEYS[1:]] == [10, 1, 0, 9]
    c = ctx(P["tgt"], opts=INCREMENTAL)
    try:
        assert c.insert(add, I4, 0.0)["n_added"] == len(add)
        assert c.kept_target_voxels()["coords"][:, 0].min() == -3
        info = assert_follows(c, what="planted insert", want=expected_info(P["tgt"], c.target_points(), add))
        assert (info["n_touched"], info["n_refit"], info["n_carried"], info["n_kept"]) == (5, 5, 5, 9)
    finally:
        c.close()


def planted_crops():
    P = vs.planted()
    tgt = P["tgt"]
    v = vr.voxel_of(tgt, 1.0)
    y_top = tgt[(v == (0, 2, 0)).all(axis=1), 1].max()                    # 2.6729884: the voxel with exactly min_points loses it
    assert y_top == np.float32(2.6729884)
    return {"z": ([-BIG, -BIG, 0.0], [BIG] * 3, 5, 0), "x": ([0.0, -BIG, -BIG], [BIG] * 3, 5, 0),
            "y": ([-BIG] * 3, [BIG, float(np.nextafter(y_top, np.float32(-np.inf))), BIG], 5, 1)}


@pytest.mark.parametrize("name", ["z", "x", "y"])
def test_planted_crops_remove_a_voxel_raise_the_minimum_and_starve_a_voxel(name):
    P = vs.planted()
    lo, hi, n_kept, more_small = planted_crops()[name]
    c = ctx(P["tgt"], opts=INCREMENTAL)
    try:
        u = c.crop(lo, hi)
        assert u["n_removed"] > 0
        new = c.target_points()
        ref = vr.voxel_map(new, *PARAMS)
        assert ref["n_kept"] == n_kept and ref["n_small"] == P["vmap"]["n_small"] + more_small, name
        info = assert_follows(c, what=name, want=expected_info(P["tgt"], new, crop_changed(P["tgt"], new, lo, hi)))
        if name == "y":
            assert info["n_refit"] == info["n_touched"] and info["n_kept"] == info["n_carried"]      # refitted, and small now
        else:
            assert info["n_refit"] == 0                                    # the touched voxel is gone
    finally:
        c.close()


# ---- 3. the table
def test_the_lattice_grows_its_table_and_is_cut_through_its_voxels():
    S = vs.lattice()
    rng = np.random.default_rng(78)
    g = np.stack(np.meshgrid(np.arange(16, 24), np.arange(8), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 3)
    add = (np.repeat(g, 6, axis=0) + rng.uniform(0.05, 0.95, (len(g) * 6, 3))).astype(np.float32)
    c = ctx(S["tgt"], S["src"], src_normals=S["src_normals"])
    prm = api.default_lin_params(RADIUS, 1)

    def dumps(what):
        o = fresh(c, src=S["src"], src_normals=S["src_normals"])
        try:
            for mode in (0, 1):
                for stencil in (1, 7, 27):
                    for k in (c, o):
                        k.set_option("voxels_source_cov", mode)
                        k.set_option("voxels_neighbors", stencil)
                    got, want = c.linearize_voxels(S["T"], prm, debug=True), o.linearize_voxels(S["T"], prm, debug=True)
                    vs.assert_dump_bitwise(got, want, (what, mode, stencil))
                    sc.assert_sums_bitwise(got, want, (what, mode, stencil))
                    assert got["n_pt"] > 0
        finally:
            o.close()
            c.set_option("voxels_source_cov", 0)
            c.set_option("voxels_neighbors", 1)

    try:
        assert c.target_voxels_kept() == 4096                             # 8 192 slots
        assert c.insert(add, I4, 0.0)["n_added"] == 6144
        info = assert_follows(c, what="lattice insert", want=expected_info(S["tgt"], c.target_points(), add))
        assert (info["n_touched"], info["n_carried"], info["n_kept"]) == (1024, 4096, 5120)           # 16 384 slots
        dumps("lattice insert")
        old = c.target_points()
        lo, hi = [-BIG] * 3, [float(np.nextafter(np.float32(7.5), np.float32(0.0))), BIG, BIG]      # x < 7.5
        c.crop(lo, hi)
        new = c.target_points()
        ref = vr.voxel_map(new, *PARAMS)
        assert [ref[k] for k in INFO_KEYS[1:]] == [2039, 241, 0, 1798]
        assert_follows(c, what="lattice crop", want=expected_info(old, new, crop_changed(old, new, lo, hi)))
        dumps("lattice crop")
    finally:
        c.close()


# ---- 4. the two filters
def test_remove_outliers_is_followed():
    L = vs.lot()
    c = ctx(L["tgt"], opts=INCREMENTAL)
    try:
        r = c.remove_outliers(api.outlier_params("radius", radius=0.3, min_neighbors=3))
        assert 0 < r["n_out"] < 4000 and len(c.target_points()) == r["n_out"]
        print(assert_follows(c, what="remove_outliers", followed=(1,)))
    finally:
        c.close()


def test_remove_dynamic_is_followed():
    L = vs.lot()
    centre = 0.5 * (L["tgt"].min(axis=0).astype(np.float64) + L["tgt"].max(axis=0))
    store = [shell(4000, 40 + k, r_lo=10.0, r_hi=30.0, el=0.6) for k in range(3)]           # three sensors above the lot that see beyond it
    members = []
    for k in range(3):
        T = pose(k)
        T[:3, 3] += centre + [0.0, 0.0, 1.5]
        members.append((k, T))
    c = ctx(L["tgt"], opts=INCREMENTAL)
    try:
        c.keyframes_reset()
        assert c.keyframes_add(store) == 0
        r = c.remove_dynamic(members, api.visibility_params(rows=16, cols=64))
        assert 0 < r["n_flagged"] and 0 < r["n_out"] < 4000 and len(c.target_points()) == r["n_out"]
        print(assert_follows(c, what="remove_dynamic", followed=(1,)))
    finally:
        c.close()


# ---- 5. incremental and full, merged and re-derived, behind a window
def run_sequence(c, followed, opts):
    L = vs.lot()
    tgt = L["tgt"]
    maps = []

    def step(what):
        assert_follows(c, what=(what, opts), followed=(followed,))
        maps.append(c.kept_target_voxels())
    assert c.insert_source(L["GT"], 0.05)["n_added"] == 53
    step("insert")
    far = patch([tgt[:, 0].max() + 30.0, tgt[:, 1].mean(), tgt[:, 2].mean()], 60, 1)
    u = c.insert(far, I4)                                                  # outside the grid's box: the grid is derived again
    assert u["n_added"] == 60 and u["rebuilt"] == 1
    step("insert outside the box")
    assert c.crop(*crop_box(tgt))["n_removed"] > 0
    step("crop")
    assert c.insert(sc.sized_source(257), L["GT"])["n_added"] == 257
    step("insert after the crop")
    return maps


@pytest.mark.parametrize("name", ["merged", "rederived", "window"])
def test_incremental_and_full_give_the_same_bytes_whatever_the_index_does(name):
    L = vs.lot()
    opts = {"merged": [("map_update", 1)], "rederived": [("map_update", 0)], "window": OPTS_WINDOW}[name]
    runs = []
    for share, followed in ((0.0, 2), (1.0, 1)):
        c = ctx(L["tgt"], L["src"], opts=list(opts) + [("voxels_follow_full_share", share)])
        try:
            if name == "window":
                c.linearize(np.ascontiguousarray(L["INIT"][:3, :3]).reshape(9), L["INIT"][:3, 3], api.default_lin_params(RADIUS))
                assert c.roi_info()["active"]
            runs.append(run_sequence(c, followed, name))
        finally:
            c.close()
    for k, (a, b) in enumerate(zip(*runs)):
        vs.assert_map_bitwise(a, b, (name, k))


# ---- 6. a seeded walk
def test_a_seeded_walk_is_the_fresh_context_after_every_step_and_in_the_engines():
    L = vs.lot()
    rng = np.random.default_rng(4242)
    lo0, hi0 = L["tgt"].min(axis=0).astype(np.float64), L["tgt"].max(axis=0).astype(np.float64)
    c = ctx(L["tgt"], L["src"])
    seen = set()
    try:
        for k in range(12):
            pts = c.target_points()
            lo, hi = pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)
            if k % 4 == 3:                                                 # a crop: a slab of the box goes
                a = int(rng.integers(0, 2))
                cut_lo, cut_hi = lo - 1.0, hi + 1.0
                if rng.integers(0, 2):
                    cut_lo[a] = lo[a] + rng.uniform(0.5, 2.5)
                else:
                    cut_hi[a] = hi[a] - rng.uniform(0.5, 2.5)
                assert c.crop(cut_lo, cut_hi)["n_removed"] > 0
            else:                                                          # an insert: a patch inside the box, or up to 15 m outside it
                centre = rng.uniform(lo0, hi0)
                if rng.integers(0, 2):
                    centre[int(rng.integers(0, 2))] += rng.choice([-1.0, 1.0]) * rng.uniform(20.0, 35.0)
                n = int(rng.integers(20, 201))
                assert c.insert(patch(centre, n, 100 + k, size=float(rng.uniform(0.5, 4.0))), I4)["n_added"] == n
            seen.add(assert_follows(c, what=("walk", k))["followed"])
        assert 1 in seen
        src_normals = vs.lot()["m5"]
        cfg = cfg_pk01()
        c.set_source_normals(np.ascontiguousarray(src_normals))
        o = fresh(c, src=L["src"], src_normals=src_normals)
        try:
            assert timeless(*c.icp_run_voxels(L["INIT"], "Ours", cfg)) == timeless(*o.icp_run_voxels(L["INIT"], "Ours", cfg))
            frames, T0s = [L["src"]] * 4, np.stack([L["INIT"]] * 4)
            a, b = c.register_frames_voxels(frames, T0s, "Ours", cfg), o.register_frames_voxels(frames, T0s, "Ours", cfg)
            assert len(a) == len(b) == 4
            for ra, rb in zip(a, b):
                assert ra.iterations > 1 and timeless(ra, [])[0] == timeless(rb, [])[0]
        finally:
            o.close()
    finally:
        c.close()


# ---- 7. what does not follow
def test_what_drops_the_voxel_map_still_drops_it():
    L = vs.lot()
    c = ctx(L["tgt"], L["src"], follow=0)
    try:
        c.insert_source(L["GT"], 0.05)                                     # the option at 0: as before
        info = c.voxels_follow_info()
        assert c.target_voxels_kept() == 0 and info["followed"] == 0 and info["n_target"] == 4053
        with pytest.raises(api.DcregError) as e:
            c.kept_target_voxels()
        assert "(%d)" % api.E_STATE in str(e.value)
        c.set_option("voxels_follow", 1)                                   # no member: nothing to follow with
        c.insert(patch(L["tgt"][0], 10, 6), I4)
        assert c.target_voxels_kept() == 0 and c.voxels_follow_info()["followed"] == 0
        c.keep_target_voxels(api.voxel_map_params(*PARAMS))
        c.insert(patch(L["tgt"][0], 10, 7), I4)
        assert c.voxels_follow_info()["followed"] == 1
        c.set_target(L["tgt"], RADIUS)                                     # a new map, with the option on
        assert c.target_voxels_kept() == 0 and c.voxels_follow_info() == ZERO
        c.keep_target_voxels(api.voxel_map_params(*PARAMS))                # the option is read at the time of the update
        c.set_option("voxels_follow", 0)
        c.insert(patch(L["tgt"][0], 10, 8), I4)
        assert c.target_voxels_kept() == 0 and c.voxels_follow_info()["followed"] == 0
        assert c._L.dcreg_target_voxels_follow_info(c._h, None) == api.E_INVALID
    finally:
        c.close()


def test_the_follow_refits_with_the_parameters_of_the_keep_that_made_the_member():
    L = vs.lot()
    params = (0.5, 1e-2, 3)
    c = ctx(L["tgt"], L["src"], params=params)
    try:
        c.insert_source(L["GT"], 0.05)
        new = c.target_points()
        assert_follows(c, params, "leaf 0.5", want=expected_info(L["tgt"], new, new[4000:], params))
    finally:
        c.close()


def test_the_normals_follow_beside_it_from_the_same_change():
    L = vs.lot()
    p = api.normal_params(k=5)
    c = ctx(L["tgt"], L["src"], opts=[("normals_follow", 1)])
    try:
        c.keep_target_normals(p)
        c.insert_source(L["GT"], 0.05)
        assert c.normals_follow_info()["followed"] in (1, 2) and c.target_normals_kept() == 1
        assert_follows(c, what="insert beside the normals", followed=(1,))
        c.crop(*crop_box(L["tgt"]))
        assert c.normals_follow_info()["followed"] in (1, 2) and c.target_normals_kept() == 1
        assert_follows(c, what="crop beside the normals", followed=(1,))
    finally:
        c.close()


def test_updates_that_change_nothing_and_refused_updates_leave_every_bit():
    L = vs.lot()
    c = ctx(L["tgt"], L["src"])
    try:
        c.insert(patch(L["tgt"][0], 30, 7), I4)
        base, info = c.kept_target_voxels(), c.voxels_follow_info()
        assert info["followed"] == 1

        def untouched(what):
            assert c.target_voxels_kept() == len(base["count"]) and c.voxels_follow_info() == info, what
            vs.assert_map_bitwise(c.kept_target_voxels(), base, what)
        assert c.insert_source(L["GT"], 100.0)["n_added"] == 0             # everything thinned away
        untouched("thinned insert")
        assert c.crop(L["tgt"].min(axis=0) - 50.0, L["tgt"].max(axis=0) + 50.0)["n_removed"] == 0
        untouched("a crop around everything")
        bad = np.array(L["src"][:8])
        bad[3, 1] = np.nan
        with pytest.raises(api.DcregError):
            c.insert(bad, I4)                                              # a NaN point: refused
        untouched("a NaN point")
        with pytest.raises(api.DcregError):
            c.crop([1e6, 1e6, 1e6], [2e6, 2e6, 2e6])                       # keeps nothing
        untouched("a crop that keeps nothing")
    finally:
        c.close()


def test_a_crop_that_leaves_no_kept_voxel_leaves_no_member():
    P = vs.planted()
    c = ctx(P["tgt"])
    try:
        u = c.crop([2.0, -BIG, -BIG], [3.0, BIG, BIG])                     # the small voxel (2,0,0) alone stays
        assert u["n_target"] == 5
        info = c.voxels_follow_info()
        assert c.target_voxels_kept() == 0 and info["n_kept"] == 0 and info["n_carried"] == 0 and info["n_target"] == 5, info
        o = fresh(c)
        try:
            assert o.target_voxels_kept() == 0
        finally:
            o.close()
    finally:
        c.close()


def test_a_span_the_keep_refuses_drops_the_member_and_the_insert_stands():
    rng = np.random.default_rng(5)
    a = (np.float64([0.0102, 0.0102, 0.0102]) + rng.uniform(0.0, 0.0005, (3, 3))).astype(np.float32)
    b = (np.float64([0.5002, 0.2002, 0.1002]) + rng.uniform(0.0, 0.0005, (3, 3))).astype(np.float32)
    params = (1e-3, 1e-3, 2)
    tgt = np.concatenate([a, b])
    v = vr.voxel_of(tgt, 1e-3)
    assert len(np.unique(a, axis=0)) == 3 and len(np.unique(b, axis=0)) == 3 and len(np.unique(v[:3], axis=0)) == 1 and len(np.unique(v[3:], axis=0)) == 1
    c = ctx(tgt, params=params)
    try:
        assert c.target_voxels_kept() == 2
        u = c.insert(np.float32([[2200.0, 0.0102, 0.0102]]), I4)           # 2.2 million voxels away
        assert u["n_added"] == 1 and u["n_target"] == 7
        info = c.voxels_follow_info()
        assert c.target_voxels_kept() == 0 and info["followed"] == 0 and info["n_target"] == 7, info
        with pytest.raises(api.DcregError) as e:                           # ... as the keep itself refuses the updated map
            c.keep_target_voxels(api.voxel_map_params(*params))
        assert "(%d)" % api.E_INVALID in str(e.value)
    finally:
        c.close()
