"""Surface normals on the device (dcreg_normals*, dcreg_target_normals*) against the numpy reference of tests/normals_ref.py, which applies
include/dcreg.h's rule literally: normals, curvature, eigenvalues, the placement of the NaN and the counts must be BITWISE the
reference's.  The map form and the index independence are checked against the cloud form, which is checked against the reference."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
import normals_ref as nr
from dcreg_amd import api
from test_gpu_device_seam import D2H, DevCloud, _info, hip, strided
from test_gpu_map_update import ZERO, crop_ref
from test_normals_reference import SPHERE_CENTRE, far_cluster, lattice, line, sphere, tilted_plane

pytestmark = pytest.mark.gpu

RADIUS = 0.5
OPTS_WINDOW = [("max_table_entries", 1 << 16), ("roi_index", 2), ("roi_margin", 1.0)]      # a window smaller than the lot


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """bitwise, any NaN equal to any NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def ref_of(cloud, p):
    return nr.normals_reference(cloud, k=p.k, search_radius=p.search_radius, viewpoint=None if p.orient else tuple(p.viewpoint))


def assert_bitwise(got, ref, what=""):
    nrm, cur, eig, info = got
    for key in ("n_in", "n_finite", "n_sparse", "n_out"):
        assert info[key] == ref[key], (what, key, info[key], ref[key])
    assert same(cur, ref["curvature"]), what
    assert same(eig, ref["eigenvalues"]), what
    assert same(nrm, ref["normals"]), what


def assert_same_bits(a, b, what=""):
    for x, y in zip(a[:3], b[:3]):
        assert (x is None and y is None) or same(x, y), what
    assert a[3] == b[3], what


def run(ctx, cloud, p):
    return ctx.normals(cloud, p, want_eigenvalues=True)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def uniform(n, seed=0):
    return (np.random.default_rng(2000 + seed + n).uniform(-2, 2, (n, 3)) * [1.0, 1.0, 0.3]).astype(np.float32)


def with_nan_rows(cloud, seed=1):
    """NaN rows and single non-finite coordinates planted"""
    rng = np.random.default_rng(seed)
    out = np.insert(cloud, rng.choice(len(cloud), 9, replace=False), np.float32(np.nan), axis=0)
    out[len(out) // 2, 1] = np.inf
    out[0, 2] = np.nan
    return out


@pytest.fixture(scope="module")
def lot():
    """the parking-lot scene at a few thousand points, a frame from its middle, the pose of the frame and a start pose"""
    tgt, src = h.scene_parkinglot(n_map=4000, n_frame=1500, extent=12.0, frame_range=5.0)
    return tgt, src, h.pose6d_matrix(**h.PK01_GT), h.pose6d_matrix(**h.PK01_INIT)


# ---- 1. bitwise against the reference: sizes, k, ties, clouds
@pytest.mark.parametrize("n", [1, 4, 5, 63, 64, 65, 255, 257, 4099])
def test_sizes_across_wave_and_block_boundaries_and_around_k(ctx, n):
    cloud = uniform(n)
    p = api.normal_params(k=5)
    ref = ref_of(cloud, p)
    assert ref["n_out"] == (n if n >= 5 else 0) and ref["n_sparse"] == n - ref["n_out"]
    assert_bitwise(run(ctx, cloud, p), ref, n)


@pytest.mark.parametrize("k", [3, 5, 8, 9, 16, 17, 32])
def test_every_heap_size(ctx, k):
    cloud = uniform(1000)
    for n in (k - 1, k):
        p = api.normal_params(k=k)
        assert_bitwise(run(ctx, cloud[:n], p), ref_of(cloud[:n], p), (k, n))
    p = api.normal_params(k=k)
    ref = ref_of(cloud, p)
    assert ref["n_out"] == 1000
    assert_bitwise(run(ctx, cloud, p), ref, k)
    p = api.normal_params(k=k, search_radius=0.3 + 0.02 * k)
    ref = ref_of(cloud, p)
    assert 0 < ref["n_sparse"] < 1000
    assert_bitwise(run(ctx, cloud, p), ref, (k, "bounded"))


@pytest.mark.parametrize("k", [5, 10])
def test_a_lattice_ties_every_distance_and_the_index_decides(ctx, k):
    cloud = lattice()
    p = api.normal_params(k=k)
    assert_bitwise(run(ctx, cloud, p), ref_of(cloud, p), "lattice")
    perm = np.random.default_rng(8).permutation(len(cloud))
    moved = np.ascontiguousarray(cloud[perm])
    ref = ref_of(moved, p)
    assert_bitwise(run(ctx, moved, p), ref, "permuted")
    back = np.empty_like(ref["normals"])
    back[perm] = ref["normals"]
    assert not same(back, ref_of(cloud, p)["normals"])           # (other indices, other neighbours: the tie-break is the index)


@pytest.mark.parametrize("copies", [3, 40])
def test_exact_duplicates(ctx, copies):
    cloud = uniform(600)
    at = np.random.default_rng(copies).choice(600, copies, replace=False)
    cloud[at] = cloud[at[0]]
    for k in (8, 32):
        p = api.normal_params(k=k)
        ref = ref_of(cloud, p)
        assert ref["n_out"] == 600 and (copies < k or np.all(ref["eigenvalues"][at] == 0.0))
        assert_bitwise(run(ctx, cloud, p), ref, (copies, k))


SCENES = {"plane": tilted_plane, "sphere": sphere, "line": line, "lot": lambda: h.scene_parkinglot(n_map=4000, n_frame=1500, extent=8.0)[0]}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_with_nan_rows(ctx, name):
    cloud = with_nan_rows(SCENES[name]())
    for k in (5, 16):
        p = api.normal_params(k=k)
        ref = ref_of(cloud, p)
        assert ref["n_finite"] == np.isfinite(cloud).all(axis=1).sum() <= len(cloud) - 9 and ref["n_out"] == ref["n_finite"]
        assert_bitwise(run(ctx, cloud, p), ref, (name, k))


def test_a_far_cluster_of_fewer_than_k_points_is_sparse_under_a_bound(ctx):
    cloud, far = far_cluster(8)
    p = api.normal_params(k=8, search_radius=1.0)
    got = run(ctx, cloud, p)
    assert got[3]["n_sparse"] == 7 and np.array_equal(np.flatnonzero(np.isnan(got[1])), far)
    assert_bitwise(got, ref_of(cloud, p), "bounded")
    p = api.normal_params(k=8)
    got = run(ctx, cloud, p)
    assert got[3]["n_sparse"] == 0
    assert_bitwise(got, ref_of(cloud, p), "unbounded")
    # the comparison is strict: a neighbour AT the bound does not count
    lat = lattice((4, 4, 4))
    for r, n_out in ((0.25, 0), (float(np.nextafter(np.float32(0.25), np.float32(1))), 64)):
        p = api.normal_params(k=3, search_radius=r)
        got = run(ctx, lat, p)
        assert got[3]["n_out"] == n_out
        assert_bitwise(got, ref_of(lat, p), r)


def test_both_orientations_and_a_viewpoint_off_the_origin(ctx):
    cloud = sphere()
    free = run(ctx, cloud, api.normal_params(k=10, viewpoint=None))
    assert_bitwise(free, ref_of(cloud, api.normal_params(k=10, viewpoint=None)), "none")
    for vp in ((0.0, 0.0, 0.0), tuple(SPHERE_CENTRE), (-4.0, 9.5, 0.25)):
        p = api.normal_params(k=10, viewpoint=vp)
        got = run(ctx, cloud, p)
        assert_bitwise(got, ref_of(cloud, p), vp)
        assert np.array_equal(np.abs(got[0]), np.abs(free[0])) and same(got[1], free[1])
    inward = run(ctx, cloud, api.normal_params(k=10, viewpoint=tuple(SPHERE_CENTRE)))[0]
    assert np.all(np.sum(inward * (SPHERE_CENTRE - cloud.astype(np.float64)), axis=1) > 0.9)


# ---- 2. the forms of the call
def test_the_strided_form_the_device_form_and_every_optional_output(ctx):
    cloud = with_nan_rows(tilted_plane())
    n = len(cloud)
    p = api.normal_params(k=6, viewpoint=(1.0, 2.0, 30.0))
    ref = ref_of(cloud, p)
    wide = strided(cloud, 5)
    assert_bitwise(run(ctx, wide, p), ref, "strided")
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        got = ctx.normals(wide, p, *want)
        for x, key, w in zip(got[:3], ("normals", "curvature", "eigenvalues"), want):
            assert (x is None) if not w else same(x, ref[key]), want
        assert got[3]["n_out"] == ref["n_out"]
    dev = DevCloud(wide)
    outs = [DevCloud(np.full((n, c), 7.0, np.float32)) for c in (3, 1, 3)]
    try:
        for use in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            for o, c in zip(outs, (3, 1, 3)):
                o.write(np.full((n, c), 7.0, np.float32))
            info = ctx.normals_device(dev.ptr, n, 5, p, *[o.ptr if u else 0 for o, u in zip(outs, use)])
            assert info == {key: ref[key] for key in ("n_in", "n_finite", "n_sparse", "n_out")}
            for o, c, u, key in zip(outs, (3, 1, 3), use, ("normals", "curvature", "eigenvalues")):
                host = np.zeros((n, c), np.float32)
                assert hip().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(o.ptr), host.nbytes, D2H) == 0
                assert same(host.reshape(ref[key].shape), ref[key]) if u else np.all(host == 7.0), (use, key)
    finally:
        for d in [dev] + outs:
            d.free()


def test_repeated_calls_and_a_second_context_give_the_same_bits(ctx, lot):
    cloud = with_nan_rows(lot[0])
    p = api.normal_params(k=9, search_radius=1.5)
    a, b = run(ctx, cloud, p), run(ctx, cloud, p)
    other = api.Context(0)
    try:
        other.set_option("cell", 0.9)
        other.set_target(lot[0], RADIUS)
        other.set_source(lot[1])
        c = run(other, cloud, p)
    finally:
        other.close()
    assert_same_bits(a, b, "repeated")
    assert_same_bits(a, c, "second context")


# ---- 3. the index decides how fast the neighbours are found, never which
def test_a_result_does_not_depend_on_the_index(ctx, lot):
    cloud = lot[0]
    for p in (api.normal_params(k=5), api.normal_params(k=16, search_radius=1.0, viewpoint=(-100.0, -400.0, 5.0))):
        want = run(ctx, cloud, p)
        assert_bitwise(want, ref_of(cloud, p), "cloud form")
        cells = []
        for hint in (0.2, 2.5):
            c = api.Context(0)
            try:
                c.set_target(cloud, hint)
                cells.append(c.index_info().cell)
                assert_same_bits(c.target_normals(p, want_eigenvalues=True), want, hint)
            finally:
                c.close()
        assert cells[0] != cells[1]                  # two indices, one answer


# ---- 4. the map form
def _grown_map(A, lot, options=()):
    tgt, src, gt, T0 = lot
    for k, v in options:
        A.set_option(k, v)
    A.set_option("count_searches", 1)
    T2 = gt.copy()
    T2[:3, 3] += [2.0, -1.5, 0.0]
    frames = h.map_frames(tgt, [gt, T2], 1200, seed=4, frame_range=6.0)
    A.set_target(tgt, RADIUS)
    A.insert(frames[0], gt)
    A.insert(frames[1], T2, min_spacing=0.05)
    cloud = A.target_points()
    lo, hi = cloud.min(0).astype(np.float64) + [1.0, 1.0, -1.0], cloud.max(0).astype(np.float64) + 1.0
    A.crop(lo, hi)
    cloud = crop_ref(cloud, lo, hi)
    assert 0 < len(cloud) and np.array_equal(bits(A.target_points()), bits(cloud))
    A.set_source(src)
    return cloud


@pytest.mark.parametrize("windowed", [False, True], ids=["whole", "window"])
def test_target_normals_after_inserts_and_a_crop(ctx, lot, windowed):
    T0 = lot[3]
    prm = api.default_lin_params(RADIUS, 0)
    A = api.Context(0)
    try:
        cloud = _grown_map(A, lot, OPTS_WINDOW if windowed else ())

        def state():
            A.launch_stats(reset=True)
            lin = A.linearize(T0[:3, :3], T0[:3, 3], prm)
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"],
                    A.launch_stats()["points_searched"], A.roi_info()["active"], A.roi_info()["windows_built"], _info(A))

        A.linearize(T0[:3, :3], T0[:3, 3], prm)
        before = state()
        assert before[0] > 0 and before[6] == 0 and bool(before[7]) == windowed
        for p in (api.normal_params(k=5), api.normal_params(k=12, search_radius=0.8, viewpoint=None)):
            got = A.target_normals(p, want_eigenvalues=True)
            want = run(ctx, cloud, p)
            assert got[3]["n_in"] == got[3]["n_finite"] == len(cloud) and 0 < got[3]["n_out"]
            assert_same_bits(got, want, p.k)
        assert_bitwise(got, ref_of(cloud, p), "map form")
        assert np.array_equal(bits(A.target_points()), bits(cloud))
        assert state() == before                     # the map, its window and the warm state served on
        assert A.index_check() == ZERO
    finally:
        A.close()


# ---- 5. the calls leave the rest of the context alone
def test_the_calls_leave_the_rest_of_the_context_alone(lot):
    tgt, src, gt, T0 = lot
    prm = api.default_lin_params(RADIUS, 0)
    cloud = strided(with_nan_rows(sphere()), 5)
    c = api.Context(0)
    dev, out = DevCloud(cloud), DevCloud(np.zeros((len(cloud), 3), np.float32))
    try:
        for k, v in OPTS_WINDOW + [("count_searches", 1)]:
            c.set_option(k, v)
        c.set_target(tgt, RADIUS)
        c.set_source(src)
        c.places_reset(api.place_params())
        c.places_add_clouds([src, tgt[:1000]])
        c.keyframes_reset()
        c.keyframes_add([src, tgt[:700]])
        c.linearize(T0[:3, :3], T0[:3, 3], prm)
        assert c.roi_info()["active"]

        def snapshot():
            c.launch_stats(reset=True)
            lin = c.linearize(T0[:3, :3], T0[:3, 3], prm)
            roi = c.roi_info()
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"],
                    c.launch_stats()["points_searched"], roi["active"], roi["windows_built"], _info(c), c.places_count(),
                    c.places_get(0, 2).tobytes(), c.keyframes_count(), c.keyframes_get(1).tobytes(), c.target_points().tobytes())

        before = snapshot()
        assert before[0] > 0 and before[6] == 0      # warm
        steps = [lambda: c.normals(cloud, api.normal_params(k=5)), lambda: c.normals(tgt, api.normal_params(k=16, search_radius=1.0)),
                 lambda: c.normals_device(dev.ptr, len(cloud), 5, api.normal_params(k=20, viewpoint=None), out.ptr),
                 lambda: c.target_normals(api.normal_params(k=8))]
        for k, step in enumerate(steps):
            step()
            assert snapshot() == before, k
    finally:
        c.close()
        dev.free()
        out.free()


# ---- 6. refusals at the C-ABI
def test_refusals_at_the_c_abi(lot):
    tgt, src, gt, T0 = lot
    L = api.load()
    cloud = np.ascontiguousarray(tilted_plane(500))
    n = len(cloud)
    nrm, cur, eig = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    big = np.zeros((len(tgt), 3), np.float32)
    info = api.NormalInfo()
    info.n_in = -5
    prm = api.default_lin_params(RADIUS, 0)
    c = api.Context(0)
    try:
        c.set_target(tgt, RADIUS)
        c.set_source(src)

        def state():
            lin = c.linearize(T0[:3, :3], T0[:3, 3], prm)
            return (lin["n_eff"], tuple(lin["H_upper"]), _info(c), c.target_points().tobytes())

        before = state()
        good = api.normal_params()

        def bad(**kw):
            p = api.normal_params()
            for key, v in kw.items():
                if key == "viewpoint":
                    p.viewpoint[0], p.viewpoint[1], p.viewpoint[2] = v
                else:
                    setattr(p, key, v)
            return p

        blocks = [bad(k=2), bad(k=33), bad(k=-1), bad(orient=2), bad(orient=-1), bad(search_radius=-1.0), bad(search_radius=np.inf),
                  bad(search_radius=np.nan), bad(viewpoint=(np.nan, 0.0, 0.0)), bad(viewpoint=(0.0, 0.0, np.inf))]
        ptr, g = cloud.ctypes.data, C.byref(good)

        def cl(p, xyz=ptr, m=n, stride=3, o=(nrm, cur, eig), dev=False):
            f = L.dcreg_normals_device if dev else L.dcreg_normals
            return f(c._h, xyz, m, stride, p, *[x.ctypes.data if x is not None else None for x in o], C.byref(info))

        def mp(p, o=(big, None, None), cap=len(tgt), dev=False):
            f = L.dcreg_target_normals_device if dev else L.dcreg_target_normals
            return f(c._h, p, *[x.ctypes.data if x is not None else None for x in o], cap, C.byref(info))

        calls = [lambda p=p: cl(C.byref(p)) for p in blocks] + [lambda p=p: mp(C.byref(p)) for p in blocks]
        calls += [lambda p=p: cl(C.byref(p), dev=True) for p in blocks[:2]] + [lambda p=p: mp(C.byref(p), dev=True) for p in blocks[:2]]
        calls += [lambda: cl(None), lambda: cl(g, stride=2), lambda: cl(g, m=-1), lambda: cl(g, xyz=None), lambda: cl(g, m=2 ** 31),
                  lambda: cl(g, o=(None, None, None)), lambda: cl(g, o=(None, None, None), dev=True), lambda: mp(None),
                  lambda: mp(g, o=(None, None, None)), lambda: mp(g, cap=len(tgt) - 1), lambda: mp(g, cap=-1), lambda: mp(g, cap=0, dev=True)]
        for k, call in enumerate(calls):
            assert call() == -1, k
            assert c._L.dcreg_last_error(c._h)
        assert not nrm.any() and not cur.any() and not eig.any() and not big.any() and info.n_in == -5
        assert state() == before
        # a linearisation in flight: DCREG_E_STATE
        c.linearize_gated_begin(prm)
        for call in (lambda: cl(g), lambda: cl(g, dev=True), lambda: mp(g), lambda: mp(g, dev=True)):
            assert call() == -4
        c.gate_abort()
        assert not nrm.any() and not big.any() and info.n_in == -5
        assert state() == before
        assert cl(g) == 0 and info.n_out == n and mp(g) == 0 and info.n_out == len(tgt)
        assert same(nrm, ref_of(cloud, good)["normals"])
        # no target for the map form; an empty cloud is no error
        e = api.Context(0)
        try:
            assert L.dcreg_target_normals(e._h, g, big.ctypes.data, None, None, len(tgt), C.byref(info)) == -4
            assert L.dcreg_normals(e._h, None, 0, 3, g, nrm.ctypes.data, None, None, C.byref(info)) == 0
            assert (info.n_in, info.n_finite, info.n_sparse, info.n_out) == (0, 0, 0, 0)
        finally:
            e.close()
    finally:
        c.close()
