"""The map form of the descriptors (dcreg_target_fpfh*, dcreg_target_fpfh_radius*) on maps that updates have changed, the ball walk of the
radius rule past one batch of rows, and the refusal of a stale report.

A. After dcreg_target_insert*, _crop, _remove_outliers or _remove_dynamic under "normals_follow" the map's index is not what a fresh build
   gives: a grid with a margin of empty rows, another origin, points merged into the sorted array, a re-derived grid, renumbered points and
   refitted normals.  include/dcreg.h promises that "a point's result depends on the cloud, the normals and the parameters only - never on
   the index": the walked context is compared, BITWISE and with equal infos, with (1) an oracle context - fresh, the same options,
   set_target(c.target_points()) + keep_target_normals(p) -, (2) the cloud form of (target_points, kept normals) on a third context, and
   (3) itself: index_check all zero, the map's bits and the linearisation's sums unchanged by the descriptor calls.  Both sides run the
   same device code on the same inputs, so the atan2 freedom does not apply and no point is exempt.
B. The radius rule's ball_walk takes the (y, z) rows of the ball 64 a batch.  With the cell edge forced ("cell") the scenes of
   tests/test_fpfh_ball_reference.py put the ball at one, two and seven batches and crowd points inside a later batch; the regime is
   asserted from index_info before the comparison, which is against the numpy references directly (assert_matches of the two descriptor
   suites, their EDGE_CAP condition unchanged).
D. dcreg_fpfh_debug_counts / dcreg_fpfh_radius_debug_counts refuse a report whose index has been rebuilt or whose map has changed since
   (include/dcreg_debug.h): the return code comes from the host, nothing is launched."""
import ctypes as C

import numpy as np
import pytest

import normal_icp_scenes as sc
from dcreg_amd import api
from test_fpfh_ball_reference import (BALL_CAP, BALL_RADIUS, CELLS, K_FORMS, LATTICE_CELLS, LATTICE_RADII, WAVE, ball_rows, box_k_reference,
                                      box_reference, box_scene, grid_of, inner, lattice_reference, lattice_scene)
from test_gpu_fpfh import assert_matches as assert_matches_k
from test_gpu_fpfh_radius import assert_matches as assert_matches_radius
from test_gpu_normals import OPTS_WINDOW, bits, same
from test_gpu_normals_follow import crop_box, ctx, lot_middle, oracle, patch
from test_gpu_visibility import pose, shell

pytestmark = pytest.mark.gpu

RADIUS = sc.RADIUS
I4 = np.eye(4)
NORMAL_SETS = {"k5": dict(k=5), "k5-radius": dict(k=5, search_radius=RADIUS)}       # the second leaves sparse points without a normal


def k_params():
    return [api.fpfh_params(k=16), api.fpfh_params(k=9, search_radius=0.7)]


def radius_params():
    return [api.fpfh_radius_params(0.9), api.fpfh_radius_params(1.2, 30)]


@pytest.fixture(scope="module")
def third():
    c = api.Context(0)
    yield c
    c.close()


def sums(c, windowed):
    """the linearisation's sums at the lot's start pose; behind them the window, where the options ask for one, is the active index"""
    T = sc.lot()["INIT"]
    lin = c.linearize(T[:3, :3], T[:3, 3], api.default_lin_params(RADIUS, 0))
    active = c.roi_info()["active"]
    assert bool(active) == windowed
    return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"], active)


def grid(c):
    i = c.index_info()
    return i.cell, tuple(i.origin), tuple(i.dims)


def compare(c, third, name, opts=(), what="", windowed=False):
    """the walked context against the three yardsticks -> the oracle's grid (cell, origin, dims)"""
    p = api.normal_params(**NORMAL_SETS[name])
    assert c.target_normals_kept() == 1, what
    before = sums(c, windowed)
    assert before[0] > 0
    pts = c.target_points()
    nrm = np.ascontiguousarray(c.kept_target_normals()[0])
    sparse = int(np.isnan(nrm).any(axis=1).sum())
    assert (sparse > 0) == (name == "k5-radius"), (what, sparse)
    o = oracle(c, p, opts)
    try:
        for form, cloud_form, params in (("target_fpfh", third.fpfh, k_params()), ("target_fpfh_radius", third.fpfh_radius, radius_params())):
            for q in params:
                got, info = getattr(c, form)(q)
                want, winfo = getattr(o, form)(q)
                assert same(got, want) and info == winfo, (what, form, info, winfo)
                cl, _, cinfo = cloud_form(pts, nrm, params=q)
                assert same(got, cl) and info == cinfo, (what, form, info, cinfo)
                assert info["n_in"] == len(pts) and info["n_used"] == len(pts) - sparse and info["n_out"] > 0, (what, form, info)
                if sparse:
                    assert info["n_used"] < info["n_in"]              # the map form took its re-index path
        ogrid = grid(o)
    finally:
        o.close()
    assert not any(c.index_check().values()), what
    assert np.array_equal(bits(c.target_points()), bits(pts)), what
    assert same(np.ascontiguousarray(c.kept_target_normals()[0]), nrm), what
    assert sums(c, windowed) == before, what
    return ogrid


def members_above(tgt):
    """three sensors above the lot that see beyond it, as tests/test_gpu_visibility.py poses them -> (store, members)"""
    centre = 0.5 * (tgt.min(axis=0).astype(np.float64) + tgt.max(axis=0))
    store = [shell(4000, 40 + k, r_lo=10.0, r_hi=30.0, el=0.6) for k in range(3)]
    members = []
    for k in range(3):
        T = pose(k)
        T[:3, 3] += centre + [0.0, 0.0, 1.5]
        members.append((k, T))
    return store, members


def far_patch(tgt):
    return patch([tgt[:, 0].max() + 40.0, tgt[:, 1].mean(), tgt[:, 2].mean()], 60, 1)


def high_patch(tgt):
    return patch([tgt[:, 0].mean(), tgt[:, 1].mean(), tgt[:, 2].max() + 3.0], 60, 2)


def step_insert(c, L):
    u = c.insert_source(L["GT"], 0.05)
    assert u["n_added"] == 53 and u["n_target"] == len(c.target_points())


def step_far(c, L):
    u = c.insert(far_patch(L["tgt"]), I4)
    assert u["n_added"] == 60 and u["rebuilt"] == 1


def step_high(c, L):
    u = c.insert(high_patch(L["tgt"]), I4)
    assert u["n_added"] == 60 and u["rebuilt"] == 1


def step_crop(c, L):
    u = c.crop(*crop_box(L["tgt"]))
    assert 0 < u["n_removed"] and u["n_target"] == len(c.target_points())


def step_outliers(c, L):
    n = len(c.target_points())
    r = c.remove_outliers(api.outlier_params("radius", radius=0.3, min_neighbors=3))
    assert 0 < r["n_out"] < n and len(c.target_points()) == r["n_out"]


def step_dynamic(c, L):
    store, members = members_above(L["tgt"])
    c.keyframes_reset()
    assert c.keyframes_add(store) == 0
    r = c.remove_dynamic(members, api.visibility_params(rows=16, cols=64))
    assert 0 < r["n_flagged"] and 0 < r["n_out"] < 4000 and len(c.target_points()) == r["n_out"]


CASES = {"insert": (step_insert,), "insert far": (step_far,), "insert high": (step_high,), "crop": (step_crop,), "remove_outliers": (step_outliers,),
         "remove_dynamic": (step_dynamic,), "chain": (step_insert, step_crop, step_far, step_outliers)}
OTHER_GRID = ("insert far", "insert high")               # the grid is re-derived with its margin: unlike any fresh build's


def middle_of_the_source():
    """the source's points within 2.5 m of its centroid (116 of 523).  The box of the whole source at the start pose, turned by 120
    degrees, with pad and margin on top spans 18.6 m - all of the cropped lot's 18 m, so that no window is built behind a crop ("the whole
    map's index serves inside this box"); this one spans 11.3 m and leaves map points outside after every step"""
    src = sc.lot()["src"]
    return np.ascontiguousarray(src[np.linalg.norm(src - src.mean(axis=0), axis=1) < 2.5])


def run_case(third, case, name, opts=(), windowed=False):
    L = sc.lot()
    c = ctx(L["tgt"], L["src"], api.normal_params(**NORMAL_SETS[name]), opts, follow=1)
    try:
        if windowed:
            c.set_source(middle_of_the_source())
            sums(c, True)                                  # the window is the active index when the first update arrives
        for step in CASES[case]:
            if windowed:
                c.set_source(L["src"])                     # (insert_source inserts the whole source; the window stays active)
                assert c.roi_info()["active"]
            step(c, L)
            if windowed:
                c.set_source(middle_of_the_source())
            assert c.normals_follow_info()["followed"] in (1, 2), (case, step.__name__)
            ogrid = compare(c, third, name, opts, "%s / %s" % (case, step.__name__), windowed)
            if case in OTHER_GRID:                         # the case ran on a grid unlike the fresh build's
                cell, origin, dims = grid(c)
                assert origin != ogrid[1] or dims != ogrid[2], (case, origin, dims, ogrid)
    finally:
        c.close()


# ---- A. the map form behind updates
@pytest.mark.parametrize("name", list(NORMAL_SETS))
@pytest.mark.parametrize("case", list(CASES))
def test_the_map_form_behind_updates_is_the_oracles_and_the_cloud_forms(third, case, name):
    run_case(third, case, name)


@pytest.mark.parametrize("name", list(NORMAL_SETS))
@pytest.mark.parametrize("case", ["insert", "crop", "chain"])
def test_the_same_from_behind_a_window(third, case, name):
    run_case(third, case, name, OPTS_WINDOW, windowed=True)


def refused(c, n):
    """both map forms return DCREG_E_STATE, write nothing and zero the info"""
    L, out = api.load(), np.full((n, 33), 7.0, np.float32)
    info, rinfo = api.FpfhInfo(), api.FpfhRadiusInfo()
    info.n_in = info.n_used = info.n_out = 99
    rinfo.n_in = rinfo.n_used = rinfo.m_sum = 99
    kp, rp = api.fpfh_params(k=16), api.fpfh_radius_params(0.9)
    assert L.dcreg_target_fpfh(c._h, C.byref(kp), out.ctypes.data, n, C.byref(info)) == api.E_STATE
    assert L.dcreg_target_fpfh_radius(c._h, C.byref(rp), out.ctypes.data, n, C.byref(rinfo)) == api.E_STATE
    assert np.all(out == 7.0)
    assert all(getattr(info, f[0]) == 0 for f in info._fields_ if isinstance(getattr(info, f[0]), int))
    assert all(getattr(rinfo, f[0]) == 0 for f in rinfo._fields_ if isinstance(getattr(rinfo, f[0]), int))


def test_the_map_form_is_refused_where_the_normals_did_not_follow():
    L = sc.lot()
    p = api.normal_params(k=5)
    c = ctx(L["tgt"], L["src"], p, follow=0)
    try:
        c.target_fpfh(api.fpfh_params(k=16))                               # kept normals, no update yet: served
        c.insert_source(L["GT"], 0.05)                                     # "normals_follow" 0: the update drops them (dcreg.h:979)
        assert c.target_normals_kept() == 0
        refused(c, 4053)
        c.keep_target_normals(p)
        c.target_fpfh_radius(api.fpfh_radius_params(0.9))
        c.drop_target_normals()
        refused(c, 4053)
        # given normals have no rule to refit with and are dropped by an update under the option too (dcreg.h:981)
        c.set_option("normals_follow", 1)
        holes = np.tile(np.float32([0, 0, 1]), (4053, 1))
        holes[::37, 1] = np.nan
        c.set_target_normals(holes)
        got, info = c.target_fpfh(api.fpfh_params(k=16))
        assert info["n_used"] == 4053 - len(holes[::37])
        c.insert(patch(lot_middle(), 10, 6), I4)
        assert c.target_normals_kept() == 0 and c.normals_follow_info()["followed"] == 0
        refused(c, 4063)
    finally:
        c.close()


# ---- B. the ball walk past one batch of rows, and points on cell faces
def forced(cell):
    c = api.Context(0)
    c.set_option("cell", cell)
    return c


def forced_map(c, cloud, normals, cell):
    """the cloud as the map of a context whose cell edge is forced -> its grid as index_info gives it (origin, dims)"""
    c.set_target(cloud, BALL_RADIUS)
    c.set_target_normals(normals)
    i = c.index_info()
    origin, dims = grid_of(cloud, cell)
    assert i.cell == cell and list(i.dims) == list(dims) and list(i.origin) == list(origin), (i.cell, list(i.dims), list(i.origin))
    return np.array(list(i.origin)), np.array(list(i.dims), np.int64)


@pytest.mark.parametrize("cell", CELLS)
def test_the_ball_walk_below_between_and_above_the_batch_sizes(cell):
    cloud, normals = box_scene()
    c = forced(cell)
    try:
        origin, dims = forced_map(c, cloud, normals, cell)
        rows = ball_rows(cloud, origin, dims, cell, BALL_RADIUS)[0]
        mid = inner(cloud, BALL_RADIUS)
        print("cell %.2f: rows %d .. %d, inside the box %d .. %d" % (cell, rows.min(), rows.max(), rows[mid].min(), rows[mid].max()))
        if cell == 0.5:
            assert rows.max() <= WAVE                                   # one trip of the r0 loop
        elif cell == 0.2:
            assert np.all(rows[mid] > WAVE) and rows.max() <= 2 * WAVE  # a second trip
        else:
            assert np.all(rows[mid] > 2 * WAVE) and rows.min() > WAVE   # a third and more, and no point with one
        for cap, ref in ((api.fpfh_radius_params().max_neighbors, box_reference()), (BALL_CAP, box_reference(BALL_CAP))):
            p = api.fpfh_radius_params(BALL_RADIUS, cap)
            got, info = c.target_fpfh_radius(p)
            assert_matches_radius(c, got, info, ref, "map form, cell %g, cap %d" % (cell, cap))
            cgot, _, cinfo = c.fpfh_radius(cloud, normals, params=p)
            assert_matches_radius(c, cgot, cinfo, ref, "cloud form, cell %g, cap %d" % (cell, cap))
            assert same(got, cgot) and info == cinfo
        # the capped scene: crowded points report cap + 1, have no SPFH, and give their neighbours nothing (the reference's rule)
        assert info["n_crowded"] == ref["n_crowded"] >= 20 and info["m_max"] == BALL_CAP + 1
        counts, m, has = c.fpfh_radius_debug_counts(len(cloud))
        assert np.all(m[ref["crowded"]] == BALL_CAP + 1) and not has[ref["crowded"]].any() and not counts[ref["crowded"]].any()
        assert np.isnan(got[ref["crowded"]]).all()
    finally:
        c.close()


@pytest.mark.parametrize("which", ["at", "above"])
@pytest.mark.parametrize("cell", LATTICE_CELLS)
def test_points_on_cell_faces_and_a_ball_that_ends_on_one(cell, which):
    cloud, normals = lattice_scene()
    ref = lattice_reference(which)
    p = api.fpfh_radius_params(LATTICE_RADII[which])
    c = forced(cell)
    try:
        origin, dims = forced_map(c, cloud, normals, cell)
        f = (cloud.astype(np.float64) - origin) / cell
        assert np.array_equal(f, np.rint(f)) and f.max() == dims[0] - 1       # every point on a face, the max corner in the last cell
        got, info = c.target_fpfh_radius(p)
        assert_matches_radius(c, got, info, ref, "map form")
        cgot, _, cinfo = c.fpfh_radius(cloud, normals, params=p)
        assert_matches_radius(c, cgot, cinfo, ref, "cloud form")
        assert same(got, cgot) and info == cinfo and info["m_max"] == (27 if which == "at" else 30)
    finally:
        c.close()


@pytest.mark.parametrize("k,search_radius", K_FORMS)
def test_the_k_form_through_many_rings_of_small_cells(k, search_radius):
    cloud, normals = box_scene()
    ref = box_k_reference(k, search_radius)
    p = api.fpfh_params(k=k, search_radius=search_radius)
    c = forced(0.1)
    try:
        forced_map(c, cloud, normals, 0.1)
        got, info = c.target_fpfh(p)
        assert_matches_k(c, got, info, ref, "map form")
        cgot, _, cinfo = c.fpfh(cloud, normals, params=p)
        assert_matches_k(c, cgot, cinfo, ref, "cloud form")
        assert same(got, cgot) and info == cinfo
        if search_radius > 0:
            assert (ref["m"] < k).any() and (ref["m"] == k).any()          # the bound, six cells wide, leaves some points short of k
    finally:
        c.close()


# ---- D. a stale report is refused
def test_a_report_behind_a_later_index_build_or_map_update_is_refused():
    L = api.load()
    cloud = sc.lot()["tgt"]
    small, normals = np.ascontiguousarray(cloud[:20]), sc.unit_normals(20, 5)
    raw8, raw32 = np.zeros((4100, 36), np.uint8), np.zeros((4100, 35), np.uint32)
    c = api.Context(0)
    try:
        c.fpfh(small, normals, params=api.fpfh_params(k=5))
        assert L.dcreg_fpfh_debug_counts(c._h, raw8.ctypes.data, 20) == api.OK            # directly behind the call
        assert L.dcreg_fpfh_debug_counts(c._h, raw8.ctypes.data, 20) == api.OK            # ... a report moves nothing
        c.outlier_filter(np.ascontiguousarray(cloud[:3000]), api.outlier_params())
        assert L.dcreg_fpfh_debug_counts(c._h, raw8.ctypes.data, 20) == api.E_STATE       # the scratch index holds 3000 other points
        assert "only valid directly behind" in L.dcreg_last_error(c._h).decode()
        c.fpfh_radius(small, normals, params=api.fpfh_radius_params(0.5))
        assert L.dcreg_fpfh_radius_debug_counts(c._h, raw32.ctypes.data, 20) == api.OK
        c.outlier_filter(np.ascontiguousarray(cloud[:3000]), api.outlier_params())
        assert L.dcreg_fpfh_radius_debug_counts(c._h, raw32.ctypes.data, 20) == api.E_STATE
        c.fpfh_radius(small, normals, params=api.fpfh_radius_params(0.5))
        c.normals(np.ascontiguousarray(cloud[:3000]), api.normal_params(k=5))
        assert L.dcreg_fpfh_radius_debug_counts(c._h, raw32.ctypes.data, 20) == api.E_STATE
        # the map forms read the map's own sorted points: an update moves them
        c.set_option("normals_follow", 1)
        c.set_target(cloud, RADIUS)
        c.keep_target_normals(api.normal_params(k=5))
        c.target_fpfh(api.fpfh_params(k=5))
        assert L.dcreg_fpfh_debug_counts(c._h, raw8.ctypes.data, 4000) == api.OK
        c.insert(patch(lot_middle(), 40, 2), I4)
        assert L.dcreg_fpfh_debug_counts(c._h, raw8.ctypes.data, 4100) == api.E_STATE
        c.target_fpfh_radius(api.fpfh_radius_params(0.5))
        assert L.dcreg_fpfh_radius_debug_counts(c._h, raw32.ctypes.data, 4040) == api.OK
        c.crop(*crop_box(cloud))
        assert L.dcreg_fpfh_radius_debug_counts(c._h, raw32.ctypes.data, 4100) == api.E_STATE
    finally:
        c.close()
