"""FPFH descriptors over a radius support on the device (dcreg_fpfh_radius*, dcreg_target_fpfh_radius*) against the numpy reference of
tests/fpfh_radius_ref.py, which applies include/dcreg.h's rule literally: the descriptors, the placement of the NaN, the counts and the info
must be BITWISE the reference's for every point that is neither edge-near nor has an edge-near neighbour (the header's one freedom: atan2
at an interior bin edge of theta); for the others the counts may differ in the flagged pairs only.  The scenes and their references are
those of tests/test_fpfh_radius_reference.py, computed once.  The map form and the forms of the call are checked against the cloud form."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from test_fpfh_radius_reference import CAP_SCENE_CAP, EDGE_CAP, SCENE_CLOUD, SIZES, SUPPORTS, cap_cloud, reference, scene, unit_normals
from test_fpfh_reference import lot_cloud, uniform
from test_gpu_device_seam import D2H, DevCloud, hip, strided
from test_gpu_normals import OPTS_WINDOW, bits, same, with_nan_rows

pytestmark = pytest.mark.gpu

RADIUS = 0.5


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def assert_matches(ctx, got, info, ref, what=""):
    """the descriptors and the info of a call against the reference; the records behind the call against the reference's counts"""
    n = ref["n_in"]
    assert ref["excluded"].sum() <= EDGE_CAP * max(ref["n_used"], 1), what
    assert info["n_out"] + info["n_empty"] == info["n_used"], (what, info)
    for k in ("n_in", "n_used", "n_crowded", "m_max", "m_sum"):
        assert info[k] == ref[k], (what, k, info)
    ex, en = ref["excluded"], ref["edge_near"]
    if not ex.any():
        assert info["n_empty"] == ref["n_empty"] and info["n_out"] == ref["n_out"], (what, info)
    assert got.shape == (n, 33) and same(got[~ex], ref["fpfh"][~ex]), what
    counts, m, has = ctx.fpfh_radius_debug_counts(n)
    assert np.array_equal(m, ref["m"]), what
    assert np.array_equal(counts[~en], ref["counts"][~en]) and np.array_equal(has[~en], ref["has_spfh"][~en]), what
    moved = np.abs(counts[en].astype(np.int64) - ref["counts"][en]).sum(axis=1)
    assert np.all(moved <= 2 * ref["edge_pairs"][en]), what          # (a pair at an edge leaves one bin and enters its neighbour)


def check(ctx, name):
    cloud, normals, radius, cap = scene(name)
    ref = reference(name)
    got, _, info = ctx.fpfh_radius(cloud, normals, params=api.fpfh_radius_params(radius, cap))
    assert_matches(ctx, got, info, ref, name)
    return got, info, ref


# ---- 1. bitwise against the reference
@pytest.mark.parametrize("n", SIZES)
def test_sizes_across_wave_and_block_boundaries(ctx, n):
    got, info, ref = check(ctx, "uniform:%d" % n)
    assert ref["n_used"] == n and (n < 2 or ref["n_out"] > 0)


@pytest.mark.parametrize("m", SUPPORTS)
def test_supports_around_the_k_forms_limit_and_around_a_byte(ctx, m):
    got, info, ref = check(ctx, "clump:%d" % m)
    assert info["m_max"] == ref["m_max"] == m and (ref["m"] == m).sum() == m


def test_the_radius_at_its_edge(ctx):
    """a lattice of spacing 0.25: at radius 0.5 the shell at exactly two steps has d2 == R2 and is out; one float above it is in"""
    at, above = check(ctx, "edge:at"), check(ctx, "edge:above")
    assert at[1]["m_max"] == 27 and above[1]["m_max"] == 30 and above[1]["m_sum"] == at[1]["m_sum"] + 3 * 64
    assert not same(at[0], above[0])


def test_the_cap(ctx):
    got, info, ref = check(ctx, "cap")
    cloud, A, B, P = cap_cloud()
    assert info["n_crowded"] == 41 and info["n_empty"] == 42 and info["m_max"] == CAP_SCENE_CAP + 1
    assert np.isnan(got[B]).all() and np.isnan(got[P]).all() and not np.isnan(got[A]).any()
    counts, m, has = ctx.fpfh_radius_debug_counts(len(cloud))
    assert np.all(m[A] == 40) and np.all(m[B] == 41) and not has[B].any() and not counts[B].any() and has[P[0]]
    # crowded neighbours contribute nothing: P has an SPFH of its own and stays empty; with the cap lifted B gives it a descriptor
    normals = scene("cap")[1]
    lifted, _, linfo = ctx.fpfh_radius(cloud, normals, params=api.fpfh_radius_params(1.0))
    assert linfo["n_crowded"] == 0 and not np.isnan(lifted[P]).any() and same(lifted[A], got[A])


@pytest.mark.parametrize("copies", [3, 40])
def test_exact_duplicates(ctx, copies):
    got, info, ref = check(ctx, "duplicates:%d" % copies)
    assert info["n_out"] > 0


def test_the_clamped_weight_and_the_one_beside_it(ctx):
    got, info, ref = check(ctx, "near")
    assert list(ref["clamped"][300:]) == [1, 1, 0, 0] and not np.isnan(got[300:]).any()


def test_a_line_whose_normals_lie_along_it_is_empty(ctx):
    got, info, ref = check(ctx, "line")
    assert info == dict(n_in=40, n_used=40, n_empty=40, n_crowded=0, n_out=0, m_max=ref["m_max"], m_sum=ref["m_sum"]) and np.isnan(got).all()


@pytest.mark.parametrize("name", sorted(SCENE_CLOUD))
def test_scenes_with_nan_rows_and_nan_normals(ctx, name):
    got, info, ref = check(ctx, name)
    cloud, normals = scene(name)[:2]
    unused = ~(np.isfinite(cloud).all(axis=1) & np.isfinite(normals).all(axis=1))
    assert info["n_used"] == len(cloud) - unused.sum() and np.isnan(got[unused]).all() and info["n_out"] > 0.9 * info["n_used"]
    assert info["m_max"] > 32


# ---- 2. the forms of the call
def test_strided_inputs_and_the_device_form(ctx):
    cloud, normals, radius, cap = scene("plane")
    n = len(cloud)
    p = api.fpfh_radius_params(radius, cap)
    want, info, _ = check(ctx, "plane")
    wide, nwide = strided(cloud, 5), strided(normals, 7, fill=3.0)
    got, _, ginfo = ctx.fpfh_radius(wide, nwide, params=p)
    assert same(got, want) and ginfo == info
    dev, dnrm, out = DevCloud(wide), DevCloud(nwide), DevCloud(np.full((n, 33), 7.0, np.float32))
    try:
        assert ctx.fpfh_radius_device(dev.ptr, n, 5, out.ptr, dnrm.ptr, 7, params=p) == info
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
    p = api.fpfh_radius_params(0.4)
    normals, _, _, ninfo = ctx.normals(cloud, npar)
    assert (ninfo["n_sparse"] > 0) == (radius > 0)
    want, _, winfo = ctx.fpfh_radius(cloud, normals, params=p)
    got, got_normals, ginfo = ctx.fpfh_radius(cloud, None, npar, p, want_normals=True)
    assert same(got_normals, normals) and same(got, want) and ginfo == winfo and ginfo["n_used"] == ninfo["n_out"] and ginfo["n_out"] > 0
    dev, out, nout = DevCloud(cloud), DevCloud(np.zeros((n, 33), np.float32)), DevCloud(np.zeros((n, 3), np.float32))
    try:
        assert ctx.fpfh_radius_device(dev.ptr, n, 3, out.ptr, 0, 3, npar, p, nout.ptr) == winfo
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
    p, npar, info = api.fpfh_radius_params(), api.normal_params(), api.FpfhRadiusInfo()

    def call(xyz=cloud.ctypes.data, n=20, stride=3, nrm=cloud.ctypes.data, nstride=3, np_=None, fp=C.byref(p), o=out.ctypes.data):
        return L.dcreg_fpfh_radius(ctx._h, xyz, n, stride, nrm, nstride, np_, fp, o, None, C.byref(info))

    def block(**kw):
        b = api.fpfh_radius_params()
        for k, v in kw.items():
            setattr(b, k, v)
        return C.byref(b)

    bad_n = api.normal_params()
    bad_n.k = 2
    assert call() == api.OK
    bad = [dict(fp=None), dict(o=None), dict(nstride=2), dict(nrm=None), dict(nrm=None, np_=C.byref(bad_n)), dict(stride=2), dict(n=-1),
           dict(n=2 ** 31), dict(xyz=None)]
    bad += [dict(fp=block(radius=r)) for r in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1.8e19)]
    bad += [dict(fp=block(max_neighbors=c)) for c in (1, 0, -1, 65536)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(nrm=None, np_=C.byref(npar)) == api.OK and call(n=0, xyz=None) == api.OK
    assert call(fp=block(max_neighbors=2)) == api.OK and call(fp=block(radius=1.7e19)) == api.OK
    # the records of one rule are not the other's
    raw8, raw32 = np.zeros((20, 36), np.uint8), np.zeros((20, 35), np.uint32)
    assert call() == api.OK and L.dcreg_fpfh_radius_debug_counts(ctx._h, raw32.ctypes.data, 20) == api.OK
    assert L.dcreg_fpfh_debug_counts(ctx._h, raw8.ctypes.data, 20) == -4
    assert L.dcreg_fpfh_radius_debug_counts(ctx._h, raw32.ctypes.data, 19) == -1 and L.dcreg_fpfh_radius_debug_counts(ctx._h, None, 20) == -1
    ctx.fpfh(cloud, unit_normals(20), params=api.fpfh_params(k=5))
    assert L.dcreg_fpfh_radius_debug_counts(ctx._h, raw32.ctypes.data, 20) == -4
    fresh = api.Context(0)
    try:
        assert L.dcreg_fpfh_radius_debug_counts(fresh._h, raw32.ctypes.data, 20) == -4
        assert L.dcreg_target_fpfh_radius(fresh._h, C.byref(p), out.ctypes.data, 20, None) == -4            # DCREG_E_STATE: no target
        fresh.set_target(cloud, RADIUS)
        assert L.dcreg_target_fpfh_radius(fresh._h, C.byref(p), out.ctypes.data, 20, None) == -4            # ... no kept normals
        fresh.keep_target_normals(api.normal_params(k=5))
        assert L.dcreg_target_fpfh_radius(fresh._h, C.byref(p), out.ctypes.data, 19, None) == -1            # capacity
        assert L.dcreg_target_fpfh_radius(fresh._h, C.byref(p), None, 20, None) == -1
        assert L.dcreg_target_fpfh_radius(fresh._h, block(radius=0.0), out.ctypes.data, 20, None) == -1
        assert L.dcreg_target_fpfh_radius(fresh._h, C.byref(p), out.ctypes.data, 20, None) == api.OK
    finally:
        fresh.close()


# ---- 3. the map form, and what the calls leave alone
@pytest.fixture(scope="module")
def lot():
    tgt, src = h.scene_parkinglot(n_map=4000, n_frame=1500, extent=12.0, frame_range=5.0)
    return tgt, src, h.pose6d_matrix(**h.PK01_INIT)


@pytest.mark.parametrize("windowed", [False, True], ids=["whole", "window"])
def test_target_fpfh_radius_is_the_cloud_form_of_the_map_and_moves_nothing(ctx, lot, windowed):
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
        normals = np.ascontiguousarray(A.kept_target_normals()[0])
        for p in (api.fpfh_radius_params(0.9), api.fpfh_radius_params(1.2, 30)):
            got, info = A.target_fpfh_radius(p)
            want, _, winfo = ctx.fpfh_radius(cloud, normals, params=p)
            assert same(got, want) and info == winfo and info["n_used"] == len(cloud) and info["n_out"] > 0
        assert info["n_crowded"] > 0
        again, _ = A.target_fpfh_radius(p)
        assert same(again, got)
        assert np.array_equal(bits(A.target_points()), bits(cloud)) and state() == before
        # a linearisation in flight: DCREG_E_STATE from every form, nothing written
        L, out, rinfo = api.load(), np.full((len(cloud), 33), 7.0, np.float32), api.FpfhRadiusInfo()
        A.linearize_begin(T0[:3, :3], T0[:3, 3], prm, slot=0)
        assert L.dcreg_target_fpfh_radius(A._h, C.byref(p), out.ctypes.data, len(cloud), C.byref(rinfo)) == -4
        assert L.dcreg_fpfh_radius(A._h, cloud.ctypes.data, len(cloud), 3, normals.ctypes.data, 3, None, C.byref(p), out.ctypes.data, None,
                                   C.byref(rinfo)) == -4
        assert L.dcreg_fpfh_radius_debug_counts(A._h, out.ctypes.data, len(cloud)) == -4
        assert rinfo.n_in == 0 and np.all(out == 7.0)
        A.linearize_end(slot=0)
        assert state() == before
        # kept normals that are not all finite: those points are no candidates
        holes = normals.copy()
        holes[::37, 1] = np.nan
        A.set_target_normals(holes)
        got, info = A.target_fpfh_radius(p)
        want, _, winfo = ctx.fpfh_radius(cloud, holes, params=p)
        assert same(got, want) and info == winfo and info["n_used"] == len(cloud) - len(holes[::37])
    finally:
        A.close()


def test_repeated_calls_and_a_second_context_give_the_same_bits(ctx):
    cloud, normals, radius, cap = scene("lot")
    p = api.fpfh_radius_params(radius, cap)
    a, b = ctx.fpfh_radius(cloud, normals, params=p), ctx.fpfh_radius(cloud, normals, params=p)
    tgt = lot_cloud()
    other = api.Context(0)
    try:
        other.set_option("cell", 0.9)              # another cell edge: the index decides how fast the neighbours are found, never which
        other.set_target(tgt, RADIUS)
        c = other.fpfh_radius(cloud, normals, params=p)
        counts_c = other.fpfh_radius_debug_counts(len(cloud))
    finally:
        other.close()
    ctx.fpfh_radius(cloud, normals, params=p)
    counts_a = ctx.fpfh_radius_debug_counts(len(cloud))
    for x in (b, c):
        assert same(a[0], x[0]) and a[2] == x[2]
    assert all(np.array_equal(x, y) for x, y in zip(counts_a, counts_c))
