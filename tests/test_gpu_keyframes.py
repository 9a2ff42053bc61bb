"""The keyframe store and its submaps on the device (dcreg_keyframes_*, dcreg_set_target_keyframes) against the numpy reference of
tests/keyframes_ref.py, which applies include/dcreg.h's rules literally.  Every comparison is bitwise on uint32 views; nothing has a
tolerance.  The reference is the yardstick, never a second device run."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
import keyframes_ref as kr
from dcreg_amd import api
from test_gpu_device_seam import D2H, DevCloud, _info, hip, strided
from test_gpu_frames import _frame_poses
from test_gpu_map_update import RADIUS, ZERO, assert_same_as_fresh, transform
from test_gpu_map_update import park            # noqa: F401  (fixture)
from test_gpu_voxel import voxel_ref

pytestmark = pytest.mark.gpu

I64P, DP = C.POINTER(C.c_int64), C.POINTER(C.c_double)
EMPTY = np.zeros((0, 3), np.float32)
WINDOW_OPTS = [("max_table_entries", 1 << 16), ("roi_index", 2)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def cloud(n, seed=0):
    return np.random.default_rng(7000 + 13 * seed + n).uniform(-30, 30, (n, 3)).astype(np.float32)


def pose(seed, spread=20.0):
    r = np.random.default_rng(500 + seed)
    return h.pose6d_matrix(*r.uniform(-spread, spread, 3), *h.deg2rad(r.uniform(-8, 8, 2)), h.deg2rad(r.uniform(-180, 180)))


def p12(T):
    T = np.asarray(T, np.float64)
    return np.r_[T[:3, :3].ravel(), T[:3, 3]]


def assert_submaps(c, store, members, leaf=None, mode="centroid", min_points=1, what=""):
    got, info = c.keyframe_submaps(members, leaf, mode, min_points)
    ref, rinfo = kr.submaps_ref(store, members, leaf, mode, min_points)
    assert len(got) == len(ref), what
    for g, (a, b) in enumerate(zip(got, ref)):
        assert same(a, b), (what, g, a.shape, b.shape)
    assert info == rinfo, (what, info, rinfo)
    return got, info


def stored_ok(c, store):
    assert c.keyframes_count() == len(store)
    assert list(c.keyframes_sizes()) == [len(s) for s in store]
    return all(same(c.keyframes_get(i), s) for i, s in enumerate(store))


def read_dev(ptr, n):
    out = np.empty((n, 3), np.float32)
    if n:
        assert hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), out.nbytes, D2H) == 0
    return out


# the tile store: keyframes at the tile edges of the gather (a tile = 2048 output points), 300 tiny ones, and empty ones
TILE_SIZES = [1, 2047, 2048, 2049, 4097]


@pytest.fixture(scope="module")
def tiles():
    rng = np.random.default_rng(77)
    store = [cloud(n) for n in TILE_SIZES] + [EMPTY.copy()] + [cloud(int(n), k) for k, n in enumerate(rng.integers(1, 4, 300))] + [EMPTY.copy()]
    c = api.Context(0)
    c.keyframes_reset()
    assert c.keyframes_add(store) == 0
    yield c, store
    c.close()


# ---- 1. the store
def test_the_store_keeps_every_cloud_bit_for_bit(park):        # noqa: F811
    frames = park[5]
    c = api.Context(0)
    dev = None
    try:
        assert c.keyframes_count() == 0
        with pytest.raises(api.DcregError, match=r"\(-4\)"):
            c.keyframes_get(0)
        with pytest.raises(api.DcregError, match=r"\(-4\)"):
            c.keyframes_add([cloud(5)])
        c.keyframes_reset()
        assert c.keyframes_count() == 0 and len(c.keyframes_sizes()) == 0
        store = []
        # one call per keyframe at first: the store grows from 1 point, at least twice before the large ones arrive
        for n in (1, 7, 2047):
            assert c.keyframes_add([cloud(n)]) == len(store)
            store.append(cloud(n))
            assert stored_ok(c, store)
        # host, stride 3 with an empty cloud among the others, then stride 5
        batch = [cloud(2048), EMPTY.copy(), cloud(2049), cloud(20_000)]
        assert c.keyframes_add(batch) == 3
        store += batch
        five = [strided(cloud(300, 1), 5), strided(cloud(11, 2), 5)]
        assert c.keyframes_add(five) == 7
        store += [f[:, :3].copy() for f in five]
        # device memory, stride 4 from an unaligned start
        dclouds = [cloud(4097, 3), cloud(2, 4), EMPTY.copy()]
        dev = DevCloud(strided(np.concatenate(dclouds), 4, fill=7.0), offset=4)
        assert c.keyframes_add_device(dev.ptr, np.r_[0, np.cumsum([len(d) for d in dclouds])], 4) == 9
        store += dclouds
        # the source in its INPUT order (the source itself is kept in curve order), without a target
        c.set_source(frames[0])
        assert c.keyframes_add_source() == 12
        store.append(frames[0])
        big = np.concatenate([frames[1], frames[2]] * 5)[:70_001]        # (a device-path source: bounds on the device)
        c.set_source(big)
        assert c.keyframes_add_source() == 13
        store.append(big)
        assert stored_ok(c, store)
        # a refused add - a NaN in the third cloud of four - changes nothing
        bad = [cloud(50, 5), cloud(3000, 6), cloud(100, 7), cloud(9, 8)]
        bad[2][61, 1] = np.nan
        with pytest.raises(api.DcregError, match=r"\(-1\)"):
            c.keyframes_add(bad)
        bad[2][61, 1] = np.inf
        with pytest.raises(api.DcregError, match=r"\(-1\)"):
            c.keyframes_add(bad)
        assert stored_ok(c, store)
        assert c.keyframes_add([cloud(5, 9)]) == 14
        store.append(cloud(5, 9))
        assert stored_ok(c, store)
        assert list(c.keyframes_sizes(3, 4)) == [2048, 0, 2049, 20_000]
        # reset empties it; ids start again
        c.keyframes_reset()
        assert c.keyframes_count() == 0 and c.keyframes_add([cloud(4)]) == 0 and same(c.keyframes_get(0), cloud(4))
    finally:
        c.close()
        if dev:
            dev.free()


# ---- 2. the gather's tiles, raw form
def _tile_cases():
    tiny = list(range(6, 306))
    T = [pose(k) for k in range(400)]
    all5 = [(i, T[i]) for i in range(5)]
    cases = {
        "edges": [all5],
        "edges reversed": [all5[::-1]],
        "each alone": [[m] for m in all5],
        "tiny": [[(i, T[k % 400]) for k, i in enumerate(tiny)]],
        "tiny behind a tile edge": [[(1, T[0])] + [(i, T[k % 400]) for k, i in enumerate(tiny)] + [(4, T[1])]],
        "empties first middle last": [[(5, T[0]), (2, T[1]), (5, T[2]), (306, T[3]), (0, T[4]), (3, T[5]), (306, T[6])]],
        "only empties": [[(5, T[0]), (306, T[1])]],
        "an empty submap between two": [[(2, T[0])], [], [(3, T[1]), (0, T[2])]],
        "no submap": [],
        "an id three times": [[(3, T[0]), (3, T[1]), (1, T[2]), (3, T[0])], [(3, T[0])], [(4, T[3]), (3, T[4])]],
        "65 submaps": [[(int(i), T[(7 * g + k) % 400]) for k, i in enumerate(np.random.default_rng(g).integers(0, 307, 1 + g % 9))] for g in range(65)],
    }
    return cases


@pytest.mark.parametrize("name", list(_tile_cases()))
def test_the_raw_form_is_the_reference(tiles, name):
    c, store = tiles
    members = _tile_cases()[name]
    got, info = assert_submaps(c, store, members, what=name)
    assert info["n_voxels"] == 0 and info["n_in"] == info["n_out"] == sum(len(g) for g in got)
    if name == "65 submaps":          # a submap's points do not depend on the submaps it shares the call with
        for g in (0, 17, 64):
            assert same(c.keyframe_submaps([members[g]])[0][0], got[g])


# ---- 3. poses
def test_poses_are_applied_as_written():
    store = [cloud(3000), np.array([[-0.0, 0.0, -0.0], [1.0, -0.0, 2.0], [1.0, 2.0, 3.0]], np.float32), cloud(100, 1)]
    far = h.pose6d_matrix(5e4, -5e4, 5e4 / 3, 0.01, -0.02, h.deg2rad(33.0))
    shear = np.eye(4)
    shear[:3, :3] = [[2.0, 0.5, 0.0], [0.0, 2.0, -0.25], [0.125, 0.0, 2.0]]
    shear[:3, 3] = [1.0, -2.0, 3.0]
    big = np.eye(4)
    big[0, 0] = 1e39
    c = api.Context(0)
    try:
        c.keyframes_reset()
        c.keyframes_add(store)
        (ident,), _ = assert_submaps(c, store, [[(1, np.eye(4))]], what="identity")
        assert np.array_equal(bits(ident[0]), bits(np.zeros(3))) and np.array_equal(ident, store[1])     # -0.0 -> +0.0, values kept
        (whole,), _ = assert_submaps(c, store, [[(0, np.eye(4))]])
        assert same(whole, store[0] + np.float32(0.0))
        assert_submaps(c, store, [[(0, far), (2, far)], [(0, shear)], [(1, shear), (0, far)]], what="far and shear")
        assert_submaps(c, store, [[(0, far)], [(0, shear)]], leaf=0.25, what="far and shear, voxels")
        # a pose that overflows float: the raw form writes inf, the voxel form drops and counts it, the raw set-target form refuses
        (raw,), _ = assert_submaps(c, store, [[(1, big), (2, np.eye(4))]], what="overflow")
        assert np.isinf(raw[1:3, 0]).all() and np.isfinite(raw[0]).all()
        _, info = assert_submaps(c, store, [[(1, big), (2, np.eye(4))]], leaf=0.5, what="overflow, voxels")
        assert info["n_in"] - info["n_finite"] == 2
        c.set_target(store[0], RADIUS)
        before = c.target_points().tobytes()
        with pytest.raises(api.DcregError, match=r"\(-1\).*non-finite"):
            c.set_target_keyframes([(1, big), (2, np.eye(4))], RADIUS)
        assert c.target_points().tobytes() == before
        info = c.set_target_keyframes([(1, big), (2, np.eye(4))], RADIUS, leaf=0.5)
        assert info["n_finite"] == 101 and same(c.target_points(), kr.submaps_ref(store, [[(1, big), (2, np.eye(4))]], 0.5)[0][0])
    finally:
        c.close()


# ---- 4. the voxel form
@pytest.fixture(scope="module")
def twelve(park):        # noqa: F811
    """12 frames of ~2 k points cut from the parking-lot scene, their poses, and 4 overlapping submaps of them"""
    tgt, gt = park[0], park[2]
    T, _ = _frame_poses(gt, 12, seed=5, step=8.0)
    frames = h.map_frames(tgt, T, 2000, seed=3)
    groups = [[0, 1, 2, 3, 4], [3, 4, 5, 6, 7], [6, 7, 8, 9, 10], [9, 10, 11, 0]]
    members = [[(i, T[i]) for i in g] for g in groups]
    c = api.Context(0)
    c.keyframes_reset()
    c.keyframes_add(frames)
    yield c, frames, T, members
    c.close()


@pytest.mark.parametrize("leaf", [0.2, (0.3, 0.2, 0.5)], ids=["cubic", "three"])
@pytest.mark.parametrize("mode", ["centroid", "first"])
def test_the_voxel_form_is_the_reference(twelve, mode, leaf):
    c, frames, T, members = twelve
    raw, _ = c.keyframe_submaps(members)
    for mp in (1, 3):
        got, info = assert_submaps(c, frames, members, leaf, mode, mp, what=(mode, leaf, mp))
        assert info["n_out"] < info["n_in"] == sum(len(r) for r in raw)
        # ... the voxel pass of the raw form's output, and each submap in a call of its own
        vox, vinfo = c.voxel_downsample(raw, leaf, mode, mp)
        assert vinfo == info and all(same(a, b) for a, b in zip(got, vox))
        for g, sub in enumerate(members):
            assert same(c.keyframe_submaps([sub], leaf, mode, mp)[0][0], got[g])


def test_a_voxel_block_is_taken_as_a_leaf_is(twelve):
    c, frames, T, members = twelve
    a, ia = c.keyframe_submaps(members, api.voxel_params((0.3, 0.2, 0.5), "first", 2))
    b, ib = c.keyframe_submaps(members, (0.3, 0.2, 0.5), "first", 2)
    assert ia == ib and all(same(x, y) for x, y in zip(a, b))


# ---- 5. the device output and the capacity protocol
@pytest.mark.parametrize("leaf", [None, 0.2], ids=["raw", "voxel"])
def test_the_device_output_and_the_capacity_protocol(twelve, leaf):
    c, frames, T, members = twelve
    host, hinfo = c.keyframe_submaps(members, leaf)
    want = np.concatenate(host)
    n = len(want)
    sentinel = np.full((n + 1, 3), 7.0, np.float32)
    for offset in (0, 4):          # 16-byte aligned and not: the vector and the scalar stores of the raw form
        out = DevCloud(sentinel, offset=offset)
        try:
            for cap in (0, n - 1):
                with pytest.raises(api.CapacityError) as e:
                    c.keyframe_submaps_device(members, out.ptr, cap, leaf)
                assert e.value.info == hinfo and list(np.diff(e.value.out_offsets)) == [len(x) for x in host]
                assert same(read_dev(out.ptr, n + 1), sentinel)          # nothing written
            off, info = c.keyframe_submaps_device(members, out.ptr, n, leaf)          # the exact capacity
            got = read_dev(out.ptr, n + 1)
            assert info == hinfo and list(np.diff(off)) == [len(x) for x in host]
            assert same(got[:n], want) and same(got[n:], sentinel[n:])
        finally:
            out.free()


# ---- 6. the map from keyframes
def _lin_state(c, T0, prm):
    lin = c.linearize(T0[:3, :3], T0[:3, 3], prm)
    return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"], _info(c), c.target_points().tobytes())


def test_set_target_keyframes_is_set_target_of_the_submap(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    members = list(zip(range(6), T))
    A = api.Context(0)
    try:
        A.keyframes_reset()
        A.keyframes_add(frames)
        info = A.set_target_keyframes(members, RADIUS)
        (expected,), rinfo = kr.submaps_ref(frames, [members])
        assert info == rinfo
        assert_same_as_fresh(A, expected, src, T0[0], cfg, frames=frames[:3])
        info = A.set_target_keyframes(members, RADIUS, leaf=0.2, min_points=2)
        (expected,), rinfo = kr.submaps_ref(frames, [members], 0.2, "centroid", 2)
        assert info == rinfo
        assert_same_as_fresh(A, expected, src, T0[1], cfg)
        assert stored_ok(A, frames)
    finally:
        A.close()


def test_a_rebuild_after_the_pose_graph_moved(park):        # noqa: F811
    """on a context that already has a map, warm states and a window index option set"""
    tgt, src, gt, T, T0, frames, cfg, _ = park
    prm = api.default_lin_params(RADIUS, 0)
    A = api.Context(0)
    try:
        for k, v in WINDOW_OPTS:
            A.set_option(k, v)
        A.set_target(tgt, RADIUS)
        A.set_source(src)
        A.reserve_warm_states(3)
        A.linearize(T0[0][:3, :3], T0[0][:3, 3], prm)
        A.keyframes_reset()
        for f in frames:
            A.keyframes_add([f])
        moved = [T[k] @ h.pose6d_matrix(*(0.05 * np.random.default_rng(k).uniform(-1, 1, 3)), 0.0, 0.0, h.deg2rad(0.3 * (k - 2))) for k in range(6)]
        for poses, leaf in ((T, 0.25), (moved, 0.25), (moved, None)):
            members = [(k, poses[k]) for k in (4, 0, 5, 1, 3, 2, 0)]          # any order, an id twice
            A.set_target_keyframes(members, RADIUS, leaf)
            (expected,), _ = kr.submaps_ref(frames, [members], leaf)
            assert_same_as_fresh(A, expected, src, T0[2], cfg, options=WINDOW_OPTS)
        # refused calls leave that map answering as before
        before = _lin_state(A, T0[2], prm)
        L = api.load()
        ids = np.array([0, 6], np.int64)
        two = np.concatenate([p12(T[0]), p12(T[1])])
        nan = two.copy()
        nan[17] = np.nan
        assert L.dcreg_set_target_keyframes(A._h, 2, ids.ctypes.data_as(I64P), two.ctypes.data_as(DP), None, RADIUS, None) == -1       # id 6 of 6
        ids[1] = 1
        assert L.dcreg_set_target_keyframes(A._h, 2, ids.ctypes.data_as(I64P), nan.ctypes.data_as(DP), None, RADIUS, None) == -1
        with pytest.raises(api.DcregError, match=r"\(-1\).*no point"):
            A.set_target_keyframes([(0, T[0])], RADIUS, leaf=0.01, min_points=50)
        assert _lin_state(A, T0[2], prm) == before
    finally:
        A.close()


# ---- 7. independence
def test_the_store_survives_everything_else(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    store = [frames[0], EMPTY.copy(), cloud(2049), frames[1][:700]]
    c = api.Context(0)
    try:
        c.keyframes_reset()
        c.keyframes_add(store)
        c.places_reset(api.place_params())
        steps = [lambda: c.set_target(tgt[:100_000], RADIUS), lambda: c.set_source(src), lambda: c.icp_run(T0[0], "Ours", cfg),
                 lambda: c.insert_source(T[0]), lambda: c.crop(tgt.min(0) + [5.0, 5.0, -1.0], tgt.max(0) - [5.0, 5.0, -1.0]),
                 lambda: c.remove_outliers(api.outlier_params(k=4, search_radius=1.0)), lambda: c.places_add_source(),
                 lambda: c.places_reset(api.place_params()), lambda: c.register_frames(frames[:3], np.stack(T0[:3]), "Ours", cfg, slots=4),
                 lambda: c.register_pairs(frames[:2], [tgt[:40_000], tgt[:30_000]], np.stack(T0[:2]), "Ours", cfg, slots=4),
                 lambda: c.voxel_downsample([tgt[:50_000]], 0.3), lambda: c.set_target_voxel(tgt[:80_000], RADIUS, 0.3),
                 lambda: c.set_source_voxel(src, 0.2)]
        for k, step in enumerate(steps):
            step()
            assert stored_ok(c, store), k
        assert_submaps(c, store, [[(0, T[0]), (2, T[1])], [(3, T[2])]], leaf=0.3)
    finally:
        c.close()


def test_the_store_and_submap_calls_leave_the_rest_of_the_context_alone(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    prm = api.default_lin_params(RADIUS, 0)
    pp = api.place_params()
    c = api.Context(0)
    n = sum(len(f) for f in frames[:3])
    dev, out = DevCloud(np.concatenate(frames[:2])), DevCloud(np.zeros((n, 3), np.float32))
    try:
        for k, v in WINDOW_OPTS + [("count_searches", 1)]:
            c.set_option(k, v)
        c.set_target(tgt, RADIUS)
        c.set_source(src)
        c.places_reset(pp)
        c.places_add_clouds(frames[:3])
        T1 = T0[0]
        c.linearize(T1[:3, :3], T1[:3, 3], prm)

        def snapshot():
            c.launch_stats(reset=True)
            lin = c.linearize(T1[:3, :3], T1[:3, 3], prm)
            roi = c.roi_info()
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"],
                    c.launch_stats()["points_searched"], roi["active"], roi["windows_built"], _info(c), c.places_count(),
                    c.places_get(0, 3).tobytes())

        before = snapshot()
        assert before[6] == 0                        # warm
        members = [[(0, T[0]), (1, T[1])], [(2, T[2])]]
        steps = [lambda: c.keyframes_reset(), lambda: c.keyframes_add(frames[:2]),
                 lambda: c.keyframes_add_device(dev.ptr, [0, len(frames[0]), len(frames[0]) + len(frames[1])], 3), lambda: c.keyframes_add_source(),
                 lambda: c.keyframes_get(1), lambda: c.keyframes_sizes(), lambda: c.keyframe_submaps(members),
                 lambda: c.keyframe_submaps(members, 0.2), lambda: c.keyframe_submaps_device(members, out.ptr, n),
                 lambda: c.keyframe_submaps_device(members, out.ptr, n, 0.2, "first"), lambda: c.keyframes_reset()]
        for k, step in enumerate(steps):
            step()
            assert snapshot() == before, k
    finally:
        c.close()
        dev.free()
        out.free()


# ---- 8. repeated calls and a second context
def test_repeated_calls_and_a_second_context_give_the_same_bits(twelve):
    c, frames, T, members = twelve
    d = api.Context(0)
    try:
        d.keyframes_reset()
        d.keyframes_add([cloud(999)])             # the other store holds something else in front
        d.set_target(frames[0], RADIUS)
        d.keyframes_add(frames)
        shifted = [[(i + 1, P) for i, P in sub] for sub in members]
        for leaf in (None, 0.2):
            a, ia = c.keyframe_submaps(members, leaf)
            b, ib = c.keyframe_submaps(members, leaf)
            e, ie = d.keyframe_submaps(shifted, leaf)
            assert ia == ib == ie and all(same(x, y) and same(x, z) for x, y, z in zip(a, b, e))
    finally:
        d.close()


# ---- 9. refusals at the C-ABI
def test_refusals_at_the_c_abi(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    L = api.load()
    prm = api.default_lin_params(RADIUS, 0)
    store = [frames[0][:3000], cloud(10), EMPTY.copy()]
    c = api.Context(0)
    try:
        c.set_target(tgt[:60_000], RADIUS)
        c.set_source(src)
        # before the first reset: DCREG_E_STATE from everything but reset / count
        first, sizes, vinfo = C.c_int64(-5), np.full(4, -5, np.int64), api.VoxelInfo()
        xyz = np.ascontiguousarray(frames[0][:100])
        off = np.array([0, 40, 100], np.int64)
        out = np.full((4000, 3), 7.0, np.float32)
        out_off = np.full(3, -5, np.int64)
        moff = np.array([0, 1, 2], np.int64)
        ids = np.array([0, 1], np.int64)
        poses = np.concatenate([p12(T[0]), p12(T[1])])
        good_v = api.voxel_params(0.2)

        def add(n=2, x=xyz.ctypes.data, o=off, stride=3, f=C.byref(first)):
            return L.dcreg_keyframes_add_clouds(c._h, n, x, o.ctypes.data_as(I64P) if o is not None else None, stride, f)

        def submaps(n=2, mo=moff, i=ids, p=poses, v=None, o=out.ctypes.data, cap=4000, oo=out_off):
            return L.dcreg_keyframes_submaps(c._h, n, mo.ctypes.data_as(I64P) if mo is not None else None, i.ctypes.data_as(I64P) if i is not None else None,
                                             p.ctypes.data_as(DP) if p is not None else None, C.byref(v) if v is not None else None, o, cap,
                                             oo.ctypes.data_as(I64P) if oo is not None else None, C.byref(vinfo))

        def set_tgt(n=2, i=ids, p=poses, v=None):
            return L.dcreg_set_target_keyframes(c._h, n, i.ctypes.data_as(I64P) if i is not None else None, p.ctypes.data_as(DP) if p is not None else None,
                                                C.byref(v) if v is not None else None, RADIUS, None)

        def get(i=0, o=out.ctypes.data, cap=4000):
            return L.dcreg_keyframes_get(c._h, i, o, cap)

        def sz(f=0, n=3):
            return L.dcreg_keyframes_sizes(c._h, f, n, sizes.ctypes.data_as(I64P))

        early = [add, submaps, set_tgt, get, sz, lambda: L.dcreg_keyframes_add_source(c._h, C.byref(first))]
        for k, call in enumerate(early):
            assert call() == -4, k
        assert L.dcreg_keyframes_count(c._h) == 0
        c.keyframes_reset()
        c.keyframes_add(store)

        def state():
            lin = c.linearize(T0[3][:3, :3], T0[3][:3, 3], prm)
            return (lin["n_eff"], tuple(lin["H_upper"]), _info(c), c.target_points().tobytes(), c.keyframes_count(),
                    [c.keyframes_get(i).tobytes() for i in range(3)])

        before = state()

        def arr(*v):
            return np.array(v, np.int64)

        def bad_pose(v):
            p = poses.copy()
            p[20] = v
            return p

        def bad_voxel(**kw):
            p = api.voxel_params(0.2)
            for key, val in kw.items():
                if key == "leaf":
                    p.leaf[2] = val
                else:
                    setattr(p, key, val)
            return p

        nan_cloud = xyz.copy()
        nan_cloud[77, 2] = np.nan
        calls = [
            # add: offsets, stride, null buffers, non-finite coordinates
            lambda: add(n=-1), lambda: add(o=None), lambda: add(o=arr(1, 40, 100)), lambda: add(o=arr(0, 60, 40)), lambda: add(stride=2),
            lambda: add(x=None), lambda: add(x=nan_cloud.ctypes.data), lambda: add(n=1, o=arr(0, 2 ** 31 - 1)),
            # sizes / get
            lambda: sz(f=-1), lambda: sz(f=2, n=2), lambda: sz(n=-1), lambda: L.dcreg_keyframes_sizes(c._h, 0, 3, None),
            lambda: get(i=3), lambda: get(i=-1), lambda: get(cap=2999), lambda: get(o=None),
            # submaps: null arrays, negative counts, offsets, ids, poses, the voxel pass's own refusals
            lambda: submaps(n=-1), lambda: submaps(mo=None), lambda: submaps(i=None), lambda: submaps(p=None), lambda: submaps(oo=None),
            lambda: submaps(cap=-1), lambda: submaps(mo=arr(1, 1, 2)), lambda: submaps(mo=arr(0, 2, 1)), lambda: submaps(i=arr(0, 3)),
            lambda: submaps(i=arr(-1, 1)), lambda: submaps(p=bad_pose(np.nan)), lambda: submaps(p=bad_pose(np.inf)),
            lambda: submaps(v=bad_voxel(leaf=0.0)), lambda: submaps(v=bad_voxel(leaf=np.nan)), lambda: submaps(v=bad_voxel(mode=3)),
            lambda: submaps(v=bad_voxel(leaf=1e-9)),                 # a submap spans 2^21 voxels
            lambda: submaps(o=None), lambda: submaps(cap=3009), lambda: submaps(v=good_v, cap=5),
            # set_target_keyframes: the same, no member, no point left
            lambda: set_tgt(n=0), lambda: set_tgt(n=-1), lambda: set_tgt(i=None), lambda: set_tgt(p=None), lambda: set_tgt(i=arr(0, 3)),
            lambda: set_tgt(p=bad_pose(-np.inf)), lambda: set_tgt(v=bad_voxel(leaf=-1.0)), lambda: set_tgt(n=1, i=arr(2)),
            lambda: set_tgt(v=bad_voxel(min_points=4000)),
        ]
        for k, call in enumerate(calls):
            assert call() == -1, k
            assert c._L.dcreg_last_error(c._h)
        assert np.all(out == 7.0) and first.value == -5 and np.all(sizes == -5)
        # the capacity protocol fills the sizes of a refused call
        assert submaps(cap=3009) == -1 and list(out_off) == [0, 3000, 3010] and (vinfo.n_in, vinfo.n_finite, vinfo.n_voxels, vinfo.n_out) == (3010, 3010, 0, 3010)
        assert np.all(out == 7.0)
        assert state() == before
        # 2^31 - 1 or more member points in one call: a keyframe of 2^20 points 2048 times
        big = api.Context(0)
        try:
            big.keyframes_reset()
            big.keyframes_add([np.zeros((1 << 20, 3), np.float32)])
            m = 2048
            many_off, many_ids, many_poses = np.array([0, m], np.int64), np.zeros(m, np.int64), np.tile(p12(np.eye(4)), m)
            oo = np.zeros(2, np.int64)
            for mm in (m, m - 1):
                many_off[1] = mm
                rc = L.dcreg_keyframes_submaps(big._h, 1, many_off.ctypes.data_as(I64P), many_ids.ctypes.data_as(I64P), many_poses.ctypes.data_as(DP), None,
                                               None, 0, oo.ctypes.data_as(I64P), None)
                assert rc == -1          # (m - 1 members: 2^31 - 2^20 points fit the call, the capacity 0 does not)
                assert (oo[1] == (m - 1) << 20) == (mm == m - 1)
                oo[:] = 0
        finally:
            big.close()
        # a linearisation in flight: DCREG_E_STATE from every call but count
        c.linearize_begin(T0[3][:3, :3], T0[3][:3, 3], prm, slot=0)
        for k, call in enumerate(early + [lambda: L.dcreg_keyframes_reset(c._h)]):
            assert call() == -4, k
        assert L.dcreg_keyframes_count(c._h) == 3
        c.linearize_end(slot=0)
        assert state() == before
        # add_source without a source
        e = api.Context(0)
        try:
            e.keyframes_reset()
            assert L.dcreg_keyframes_add_source(e._h, C.byref(first)) == -4 and first.value == -5
            assert L.dcreg_keyframes_add_clouds(e._h, 0, None, None, 3, C.byref(first)) == 0 and first.value == 0 and e.keyframes_count() == 0
        finally:
            e.close()
        assert add() == 0 and first.value == 3 and submaps() == 0 and list(out_off) == [0, 3000, 3010]
    finally:
        c.close()


# ---- 10. end to end
def test_a_keyframe_loop_and_the_map_rebuilt_from_its_results(park):        # noqa: F811
    tgt, src, gt, T, T0, frames, cfg, _ = park
    A = api.Context(0)
    try:
        A.set_target(tgt[:150_000], RADIUS)
        A.keyframes_reset()
        A.places_reset(api.place_params())
        results = []
        for k, f in enumerate(frames):
            A.set_source(f)
            res, _ = A.icp_run(T0[k], "Ours", cfg)
            Tr = np.eye(4)
            Tr[:3, :3] = np.array(res.R[:]).reshape(3, 3)
            Tr[:3, 3] = res.t[:]
            A.insert_source(Tr)
            A.places_add_source()
            assert A.keyframes_add_source() == k == A.places_count() - 1          # one index for both
            results.append(Tr)
        info = A.set_target_keyframes(list(zip(range(6), results)), RADIUS, leaf=0.2)
        expected = voxel_ref(np.concatenate([transform(f, Tr) for f, Tr in zip(frames, results)]), 0.2)
        assert info["n_in"] == sum(len(f) for f in frames) and info["n_out"] == len(expected)
        assert same(A.target_points(), expected) and A.index_check() == ZERO
        assert stored_ok(A, frames)
    finally:
        A.close()
