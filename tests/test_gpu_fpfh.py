"""FPFH descriptors on the device (dcreg_fpfh*, dcreg_target_fpfh*) against the numpy reference of tests/fpfh_ref.py, which applies
include/dcreg.h's rule literally: the descriptors, the placement of the NaN and the counts must be BITWISE the reference's for every point
that is neither edge-near nor has an edge-near neighbour (the header's one freedom: atan2 at an interior bin edge of theta); for the others
the SPFH counts may differ in the flagged pairs only.  The map form and the forms of the call are checked against the cloud form."""
import ctypes as C

import numpy as np
import pytest

import fpfh_ref as fr
import helpers as h
from dcreg_amd import api
from test_fpfh_reference import EDGE_CAP, lot_cloud, moved_copy
from test_gpu_device_seam import D2H, DevCloud, hip, strided
from test_gpu_normals import OPTS_WINDOW, bits, same, uniform, with_nan_rows
from test_normals_reference import lattice, line, sphere, tilted_plane

pytestmark = pytest.mark.gpu

RADIUS = 0.5


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def unit_normals(n, seed=0):
    v = np.random.default_rng(77 + seed + n).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def ref_of(cloud, normals, p):
    return fr.fpfh_reference(cloud, normals, k=p.k, search_radius=p.search_radius)


def assert_matches(ctx, got, info, ref, what=""):
    """the descriptors and the info of a call against the reference; the SPFH records behind the call against the reference's counts"""
    n = ref["n_in"]
    assert ref["excluded"].sum() <= EDGE_CAP * max(ref["n_used"], 1), what
    assert info["n_in"] == n and info["n_used"] == ref["n_used"] and info["n_out"] + info["n_empty"] == info["n_used"], (what, info)
    ex, en = ref["excluded"], ref["edge_near"]
    if not ex.any():
        assert info["n_empty"] == ref["n_empty"] and info["n_out"] == ref["n_out"], (what, info)
    assert got.shape == (n, 33) and same(got[~ex], ref["fpfh"][~ex]), what
    counts, m, has = ctx.fpfh_debug_counts(n)
    assert np.array_equal(m, ref["m"]), what
    assert np.array_equal(counts[~en], ref["counts"][~en]) and np.array_equal(has[~en], ref["has_spfh"][~en]), what
    moved = np.abs(counts[en].astype(np.int64) - ref["counts"][en]).sum(axis=1)
    assert np.all(moved <= 2 * ref["edge_pairs"][en]), what          # (a pair at an edge leaves one bin and enters its neighbour)


def check(ctx, cloud, normals, p, what=""):
    ref = ref_of(cloud, normals, p)
    got, _, info = ctx.fpfh(cloud, normals, params=p)
    assert_matches(ctx, got, info, ref, what)
    return got, info, ref


# ---- 1. bitwise against the reference: sizes, k, bounds, ties, special clouds
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 4099])
def test_sizes_across_wave_and_block_boundaries(ctx, n):
    got, info, ref = check(ctx, uniform(n), unit_normals(n), api.fpfh_params(k=5), n)
    assert ref["n_used"] == n and (n < 2 or ref["n_out"] > 0)


@pytest.mark.parametrize("k", [3, 5, 16, 17, 32])
def test_every_heap_size_below_at_and_above_k(ctx, k):
    cloud, normals = uniform(1000), unit_normals(1000)
    for n in (k - 1, k, 1000):
        got, info, ref = check(ctx, cloud[:n], normals[:n], api.fpfh_params(k=k), (k, n))
        assert ref["m"].max() == min(k, n) and info["n_out"] == n


def test_a_bounded_search_keeps_the_neighbours_it_has(ctx):
    cloud = np.concatenate([uniform(300), [[30.0, 0.0, 0.0]], [[40.0, 0.0, 0.0], [40.05, 0.0, 0.0]]]).astype(np.float32)
    normals = unit_normals(len(cloud))
    for k in (8, 16, 32):
        got, info, ref = check(ctx, cloud, normals, api.fpfh_params(k=k, search_radius=0.6), k)
        m = ref["m"]
        assert m[300] == 1 and m[301] == 2 and (m[:300] == k).any() == (k < 32) and ((m[:300] > 1) & (m[:300] < k)).any()
        assert np.isnan(got[300]).all() and info["n_empty"] >= 1
    # the comparison is strict: a neighbour AT the bound does not count
    lat = lattice((4, 4, 4))
    for r, m_max in ((0.25, 1), (float(np.nextafter(np.float32(0.25), np.float32(1))), 7)):
        got, info, ref = check(ctx, lat, unit_normals(64), api.fpfh_params(k=8, search_radius=r), r)
        assert ref["m"].max() == m_max and (info["n_out"] == 0) == (m_max == 1)


@pytest.mark.parametrize("k", [5, 10])
def test_a_lattice_ties_every_distance_and_the_index_decides(ctx, k):
    cloud = lattice()
    normals = unit_normals(len(cloud))
    p = api.fpfh_params(k=k)
    a, _, _ = check(ctx, cloud, normals, p, "lattice")
    perm = np.random.default_rng(8).permutation(len(cloud))
    b, _, _ = check(ctx, np.ascontiguousarray(cloud[perm]), np.ascontiguousarray(normals[perm]), p, "permuted")
    back = np.empty_like(b)
    back[perm] = b
    assert not same(back, a)                      # (other indices, other neighbours: the tie-break is the index)
    axis = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(cloud), 1))
    check(ctx, cloud, axis, p, "axis normals: pairs along z have v = 0")


@pytest.mark.parametrize("copies", [3, 40])
def test_exact_duplicates(ctx, copies):
    cloud, normals = uniform(600), unit_normals(600)
    at = np.random.default_rng(copies).choice(600, copies, replace=False)
    cloud[at] = cloud[at[0]]
    for k in (8, 32):
        got, info, ref = check(ctx, cloud, normals, api.fpfh_params(k=k), (copies, k))
        assert (copies < k) or not ref["has_spfh"][at].any()      # k copies around a point: every pair has d2 == 0


def test_a_line_whose_normals_lie_along_it_is_empty(ctx):
    cloud = line()
    s = np.float32(1.0 / np.sqrt(6.0))
    normals = np.tile(np.array([s, 2 * s, -s], np.float32), (len(cloud), 1))
    got, info, ref = check(ctx, cloud, normals, api.fpfh_params(k=8), "line")
    assert info == dict(n_in=40, n_used=40, n_empty=40, n_out=0) and np.isnan(got).all()


SCENES = {"plane": tilted_plane, "sphere": sphere, "lot": lot_cloud}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_with_nan_rows_and_nan_normals(ctx, name):
    cloud = with_nan_rows(SCENES[name]())
    normals = ctx.normals(cloud, api.normal_params(k=12))[0]
    assert np.isnan(normals).any(axis=1).sum() >= 9
    hit = np.random.default_rng(5).choice(len(cloud), 7, replace=False)
    normals[hit, np.arange(7) % 3] = [np.nan, np.inf, -np.inf, np.nan, np.nan, np.inf, np.nan]
    for k in (5, 16):
        got, info, ref = check(ctx, cloud, normals, api.fpfh_params(k=k), (name, k))
        unused = ~(np.isfinite(cloud).all(axis=1) & np.isfinite(normals).all(axis=1))
        assert info["n_used"] == len(cloud) - unused.sum() and np.isnan(got[unused]).all() and info["n_out"] > 0.9 * info["n_used"]


# ---- 2. the forms of the call
def test_strided_inputs_and_the_device_form(ctx):
    cloud = with_nan_rows(tilted_plane())
    n = len(cloud)
    normals = ctx.normals(cloud, api.normal_params(k=8))[0]
    p = api.fpfh_params(k=11, search_radius=0.9)
    want, info, _ = check(ctx, cloud, normals, p, "plain")
    wide, nwide = strided(cloud, 5), strided(normals, 7, fill=3.0)
    got, _, ginfo = ctx.fpfh(wide, nwide, params=p)
    assert same(got, want) and ginfo == info
    dev, dnrm, out = DevCloud(wide), DevCloud(nwide), DevCloud(np.full((n, 33), 7.0, np.float32))
    try:
        assert ctx.fpfh_device(dev.ptr, n, 5, out.ptr, dnrm.ptr, 7, params=p) == info
        host = np.zeros((n, 33), np.float32)
        assert hip().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(out.ptr), host.nbytes, D2H) == 0
        assert same(host, want)
    finally:
        for d in (dev, dnrm, out):
            d.free()


@pytest.mark.parametrize("radius", [0.0, 0.35], ids=["every point has a normal", "sparse points have none"])
def test_normals_estimated_inside_the_call(ctx, radius):
    cloud = with_nan_rows(uniform(1500))
    n = len(cloud)
    npar = api.normal_params(k=7, search_radius=radius, viewpoint=(0.5, 0.0, 9.0))
    p = api.fpfh_params(k=16)
    normals, _, _, ninfo = ctx.normals(cloud, npar)
    assert (ninfo["n_sparse"] > 0) == (radius > 0)
    want, _, winfo = ctx.fpfh(cloud, normals, params=p)
    got, got_normals, ginfo = ctx.fpfh(cloud, None, npar, p, want_normals=True)
    assert same(got_normals, normals) and same(got, want) and ginfo == winfo and ginfo["n_used"] == ninfo["n_out"]
    assert_matches(ctx, got, ginfo, ref_of(cloud, normals, p), radius)
    dev, out, nout = DevCloud(cloud), DevCloud(np.zeros((n, 33), np.float32)), DevCloud(np.zeros((n, 3), np.float32))
    try:
        assert ctx.fpfh_device(dev.ptr, n, 3, out.ptr, 0, 3, npar, p, nout.ptr) == winfo
        host, hn = np.zeros((n, 33), np.float32), np.zeros((n, 3), np.float32)
        assert hip().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(out.ptr), host.nbytes, D2H) == 0
        assert hip().hipMemcpy(C.c_void_p(hn.ctypes.data), C.c_void_p(nout.ptr), hn.nbytes, D2H) == 0
        assert same(host, want) and same(hn, normals)
    finally:
        for d in (dev, out, nout):
            d.free()


def test_the_library_refuses_what_the_header_lists(ctx):
    L = api.load()
    cloud, out = uniform(20), np.zeros((20, 33), np.float32)
    p, npar, info = api.fpfh_params(), api.normal_params(), api.FpfhInfo()

    def call(xyz=cloud.ctypes.data, n=20, stride=3, nrm=cloud.ctypes.data, nstride=3, np_=None, fp=C.byref(p), o=out.ctypes.data):
        return L.dcreg_fpfh(ctx._h, xyz, n, stride, nrm, nstride, np_, fp, o, None, C.byref(info))

    bad_k = api.fpfh_params()
    bad_k.k = 33
    bad_n = api.normal_params()
    bad_n.k = 2
    assert call() == api.OK
    for kw in (dict(fp=None), dict(fp=C.byref(bad_k)), dict(o=None), dict(nstride=2), dict(nrm=None), dict(nrm=None, np_=C.byref(bad_n)),
               dict(stride=2), dict(n=-1), dict(n=2 ** 31), dict(xyz=None)):
        assert call(**kw) == -1, kw
    assert call(nrm=None, np_=C.byref(npar)) == api.OK and call(n=0, xyz=None) == api.OK
    fresh = api.Context(0)
    try:
        assert L.dcreg_target_fpfh(fresh._h, C.byref(p), out.ctypes.data, 20, None) == -4            # DCREG_E_STATE: no target
        fresh.set_target(cloud, RADIUS)
        assert L.dcreg_target_fpfh(fresh._h, C.byref(p), out.ctypes.data, 20, None) == -4            # ... no kept normals
        fresh.keep_target_normals(api.normal_params(k=5))
        assert L.dcreg_target_fpfh(fresh._h, C.byref(p), out.ctypes.data, 19, None) == -1            # capacity
        assert L.dcreg_target_fpfh(fresh._h, C.byref(p), None, 20, None) == -1
        assert L.dcreg_target_fpfh(fresh._h, C.byref(p), out.ctypes.data, 20, None) == api.OK
    finally:
        fresh.close()


# ---- 3. the map form, and what the calls leave alone
@pytest.fixture(scope="module")
def lot():
    tgt, src = h.scene_parkinglot(n_map=4000, n_frame=1500, extent=12.0, frame_range=5.0)
    return tgt, src, h.pose6d_matrix(**h.PK01_INIT)


@pytest.mark.parametrize("windowed", [False, True], ids=["whole", "window"])
def test_target_fpfh_is_the_cloud_form_of_the_map_and_moves_nothing(ctx, lot, windowed):
    tgt, src, T0 = lot
    prm = api.default_lin_params(RADIUS, 0)
    A = api.Context(0)
    try:
        for k, v in (OPTS_WINDOW if windowed else ()):
            A.set_option(k, v)
        A.set_target(tgt, RADIUS)
        A.set_source(src)
        A.keep_target_normals(api.normal_params(k=10))

        def state():
            lin = A.linearize(T0[:3, :3], T0[:3, 3], prm)
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"], A.roi_info()["active"])

        before = state()
        assert before[0] > 0 and bool(before[6]) == windowed
        cloud = A.target_points()
        normals = A.kept_target_normals()[0]
        assert A.target_normals_kept() and normals.shape == cloud.shape
        for p in (api.fpfh_params(k=16), api.fpfh_params(k=9, search_radius=0.7)):
            got, info = A.target_fpfh(p)
            want, _, winfo = ctx.fpfh(cloud, np.ascontiguousarray(normals), params=p)
            assert same(got, want) and info == winfo and info["n_used"] == len(cloud)
        assert_matches(ctx, want, winfo, ref_of(cloud, normals, p), "map form")
        again, _ = A.target_fpfh(p)
        assert same(again, got)
        assert np.array_equal(bits(A.target_points()), bits(cloud)) and state() == before
        # kept normals that are not all finite: those points are no candidates
        holes = np.ascontiguousarray(normals).copy()
        holes[::37, 1] = np.nan
        A.set_target_normals(holes)
        got, info = A.target_fpfh(p)
        want, _, winfo = ctx.fpfh(cloud, holes, params=p)
        assert same(got, want) and info == winfo and info["n_used"] == len(cloud) - len(holes[::37])
    finally:
        A.close()


def test_repeated_calls_and_a_second_context_give_the_same_bits(ctx, lot):
    cloud = with_nan_rows(lot[0])
    normals = ctx.normals(cloud, api.normal_params(k=9))[0]
    p = api.fpfh_params(k=13, search_radius=1.5)
    a, b = ctx.fpfh(cloud, normals, params=p), ctx.fpfh(cloud, normals, params=p)
    other = api.Context(0)
    try:
        other.set_option("cell", 0.9)
        other.set_target(lot[0], RADIUS)
        other.set_source(lot[1])
        c = other.fpfh(cloud, normals, params=p)
    finally:
        other.close()
    for x in (b, c):
        assert same(a[0], x[0]) and a[2] == x[2]
