"""The fourth engine's pairs form without a device: the exports, the refusals of the C-ABI that need no context or no device (null
arguments, a stride below 3, offsets that do not start at 0 or decrease, a null target buffer, the voxel map parameters - checked before
the empty call returns), n_pairs == 0, the plan of the build batches under a set "pairs_max_bytes", the voxel box a build refuses, and the
arguments the Context methods check before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

NEW = ("dcreg_register_pairs_voxels", "dcreg_pairs_plan_voxels", "dcreg_pairs_voxels_build", "dcreg_pairs_voxels_get", "dcreg_pairs_voxels_kept",
       "dcreg_voxel_map_params_check", "dcreg_pairs_voxels_box_check", "dcreg_pairs_voxels_batch_begin")
FP, I64P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
I4 = np.eye(4)
# bytes a target point is planned at with stride 3 (context.hip pair_voxel_target_bytes), and per target
PER_POINT, PER_TARGET = 4.0 * 3 + 16.0 + 12.0 + 20.0 + 24.0 + 16.0 + 48.0 + 52.0, 256.0


class _Ctx(C.Structure):
    """a zeroed block of memory stands in for a context: the refusals below leave their text in it and read nothing but its options"""
    _fields_ = [("bytes", C.c_char * (1 << 16))]


def _pairs(n=3, pts=4):
    xyz = np.zeros((n * pts, 3), np.float32)
    off = np.arange(n + 1, dtype=np.int64) * pts
    R0 = np.tile(np.eye(3).reshape(9), (n, 1))
    t0 = np.zeros((n, 3))
    return xyz, off, R0, t0


def _ptr(a, kind):
    return None if a is None else a.ctypes.data_as(kind)


def _ref(p):
    return None if p is None else C.byref(p)


def _register(L, ctx, n, sxyz, soff, txyz, toff, stride, tv, sn, R0, t0, cfg, res):
    return L.dcreg_register_pairs_voxels(ctx, n, _ptr(sxyz, FP), _ptr(soff, I64P), _ptr(txyz, FP), _ptr(toff, I64P), stride, _ref(tv), _ref(sn),
                                         None if R0 is None else api._dp(R0), None if t0 is None else api._dp(t0), 0, 0, _ref(cfg), 0, res)


def _plan(L, ctx, counts, stride=3):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ends, nb = (C.c_int32 * max(len(counts), 1))(), C.c_int(-1)
    assert L.dcreg_pairs_plan_voxels(ctx, len(counts), off.ctypes.data_as(I64P), stride, ends, C.byref(nb)) == api.OK
    return [int(e) for e in ends[:nb.value]]


def _bad_blocks():
    """(field, value) of every voxel map parameter the header refuses"""
    return (("leaf", 0.0), ("leaf", np.nan), ("leaf", np.inf), ("leaf", -1.0), ("epsilon", 0.5e-6), ("epsilon", 1.5), ("min_points", 1))


def _block(field, value):
    p = api.voxel_map_params()
    setattr(p, field, value)
    return p


def test_every_symbol_is_exported_and_no_struct_moved():
    L = api.load()
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name, cls in (("dcreg_trial_result", api.TrialResult), ("dcreg_lin_out", api.LinOut), ("dcreg_lin_params", api.LinParams),
                      ("dcreg_normal_params", api.NormalParams), ("dcreg_voxel_map_params", api.VoxelMapParams),
                      ("dcreg_voxel_map_info", api.VoxelMapInfo), ("dcreg_config", api.Config)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    xyz, off, R0, t0 = _pairs()
    cfg, q, tv = api.default_config(), api.default_lin_params(0.5), api.voxel_map_params()
    res = (api.TrialResult * 3)()
    infos = (api.VoxelMapInfo * 3)()
    ids = np.zeros(3, np.int32)
    ends, nb = (C.c_int32 * 3)(), C.c_int(-1)
    coords, count, mean, cov = np.zeros((4, 3), np.int64), np.zeros(4, np.int32), np.zeros((4, 3), np.float32), np.zeros((4, 6), np.float32)
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    for n in (3, 0):
        assert _register(L, None, n, xyz, off, xyz, off, 3, tv, None, R0, t0, cfg, res) == api.E_INVALID
    assert L.dcreg_pairs_plan_voxels(None, 3, off.ctypes.data_as(I64P), 3, ends, C.byref(nb)) == api.E_INVALID and nb.value == -1
    assert L.dcreg_pairs_voxels_build(None, 3, xyz.ctypes.data_as(FP), off.ctypes.data_as(I64P), 3, C.byref(tv), infos) == api.E_INVALID
    assert L.dcreg_pairs_voxels_get(None, 0, coords.ctypes.data, count.ctypes.data, mean.ctypes.data, cov.ctypes.data, 4) == api.E_INVALID
    assert L.dcreg_pairs_voxels_kept(None, 0) == 0
    assert L.dcreg_voxel_map_params_check(None, C.byref(tv)) == api.E_INVALID
    assert L.dcreg_pairs_voxels_box_check(None, lo.ctypes.data_as(FP), hi.ctypes.data_as(FP), 1.0, 0) == api.E_INVALID
    assert L.dcreg_pairs_voxels_batch_begin(None, 0, 3, api._dp(R0), api._dp(t0), ids.ctypes.data_as(I32P), ids.ctypes.data_as(I32P), C.byref(q)) == api.E_INVALID
    assert all(r.iterations == 0 and r.status == 0 for r in res) and all(i.n_points == 0 for i in infos)


def test_argument_refusals_that_need_no_device():
    L = api.load()
    L.dcreg_last_error.restype = C.c_char_p
    xyz, off, R0, t0 = _pairs()
    cfg, tv, sn = api.default_config(), api.voxel_map_params(), api.normal_params()
    res = (api.TrialResult * 3)()
    for r in res:
        r.iterations = -7
    blob = _Ctx()
    ctx = C.c_void_p(C.addressof(blob))
    good = dict(n=3, sxyz=xyz, soff=off, txyz=xyz, toff=off, stride=3, tv=tv, sn=None, R0=R0, t0=t0, cfg=cfg, res=res)

    def call(**kw):
        return _register(L, ctx, **dict(good, **kw))

    assert call(n=-1) == api.E_INVALID
    assert call(stride=2) == api.E_INVALID
    assert call(cfg=None) == api.E_INVALID
    for name in ("soff", "toff", "R0", "t0", "res"):
        assert call(**{name: None}) == api.E_INVALID, name
    for name in ("soff", "toff"):
        assert call(**{name: off + 1}) == api.E_INVALID, name
        assert b"start at 0" in L.dcreg_last_error(ctx)
        assert call(**{name: np.array([0, 8, 4, 12], np.int64)}) == api.E_INVALID, name
        assert b"decrease" in L.dcreg_last_error(ctx)
    assert call(txyz=None) == api.E_INVALID
    assert b"null target buffer" in L.dcreg_last_error(ctx)
    # the voxel map parameters: a null block and every value the header refuses, with pairs and - before the empty call returns - without
    for n in (3, 0):
        assert call(n=n, tv=None) == api.E_INVALID
        assert b"null voxel map parameters" in L.dcreg_last_error(ctx)
        for field, value in _bad_blocks():
            assert call(n=n, tv=_block(field, value)) == api.E_INVALID, (n, field, value)
            assert field.split("_")[0].encode() in L.dcreg_last_error(ctx), (n, field, value)
    # n_pairs == 0 does nothing, whatever else is passed - after the parameter refusals; mode 0: source_normals is not read
    bad_normals = api.normal_params()
    bad_normals.k = 2
    assert call(n=0, sxyz=None, soff=None, txyz=None, toff=None, R0=None, t0=None, res=None) == api.OK
    assert call(n=0, sn=bad_normals) == api.OK
    assert call(n=0, sn=sn) == api.OK
    assert all(r.iterations == -7 and r.status == 0 for r in res)
    # ---- the parameter check on its own
    assert L.dcreg_voxel_map_params_check(ctx, C.byref(tv)) == api.OK
    assert L.dcreg_voxel_map_params_check(ctx, None) == api.E_INVALID
    for field, value in _bad_blocks():
        assert L.dcreg_voxel_map_params_check(ctx, C.byref(_block(field, value))) == api.E_INVALID, (field, value)
    for field, value in (("epsilon", 1e-6), ("epsilon", 1.0), ("min_points", 2), ("leaf", 1e-30)):
        assert L.dcreg_voxel_map_params_check(ctx, C.byref(_block(field, value))) == api.OK, (field, value)
    # ---- the build: parameters and arguments first (a zeroed block has no device behind it, so nothing further is tried here)
    infos = (api.VoxelMapInfo * 3)()
    build = lambda n, x, o, stride, p: L.dcreg_pairs_voxels_build(ctx, n, _ptr(x, FP), _ptr(o, I64P), stride, _ref(p), infos)
    assert build(3, xyz, off, 3, None) == api.E_INVALID
    for field, value in _bad_blocks():
        assert build(3, xyz, off, 3, _block(field, value)) == api.E_INVALID, (field, value)
    assert build(-1, xyz, off, 3, tv) == api.E_INVALID
    assert build(3, xyz, None, 3, tv) == api.E_INVALID
    assert build(3, xyz, off, 2, tv) == api.E_INVALID
    assert build(3, xyz, off + 1, 3, tv) == api.E_INVALID
    assert build(3, xyz, np.array([0, 8, 4, 12], np.int64), 3, tv) == api.E_INVALID
    assert b"decrease" in L.dcreg_last_error(ctx)
    assert build(3, None, off, 3, tv) == api.E_INVALID
    assert b"null point buffer" in L.dcreg_last_error(ctx)
    assert build(3, xyz, np.array([0, 4, 8, 2 ** 31], np.int64), 3, tv) == api.E_INVALID
    assert b"too many points" in L.dcreg_last_error(ctx)
    assert all(i.n_points == 0 for i in infos)
    # ---- the getters and the launch on a block without a batch
    coords, count, mean, cov = np.zeros((4, 3), np.int64), np.zeros(4, np.int32), np.zeros((4, 3), np.float32), np.zeros((4, 6), np.float32)
    assert L.dcreg_pairs_voxels_kept(ctx, 0) == 0 and L.dcreg_pairs_voxels_kept(ctx, -1) == 0
    assert L.dcreg_pairs_voxels_get(ctx, 0, None, count.ctypes.data, mean.ctypes.data, cov.ctypes.data, 4) == api.E_INVALID
    assert L.dcreg_pairs_voxels_get(ctx, 0, coords.ctypes.data, count.ctypes.data, mean.ctypes.data, cov.ctypes.data, 4) == api.E_STATE
    q = api.default_lin_params(0.5)
    ids = np.zeros(3, np.int32)
    begin = lambda slot, n, R, t, s, g, p: L.dcreg_pairs_voxels_batch_begin(ctx, slot, n, None if R is None else api._dp(R), None if t is None else api._dp(t),
                                                                            _ptr(s, I32P), _ptr(g, I32P), _ref(p))
    for slot in (-1, 2):
        assert begin(slot, 3, R0, t0, ids, ids, q) == api.E_INVALID
    assert begin(0, 0, R0, t0, ids, ids, q) == api.E_INVALID
    assert begin(0, 65536, R0, t0, ids, ids, q) == api.E_INVALID
    for kw in (dict(R=None), dict(t=None), dict(s=None), dict(g=None), dict(p=None)):
        args = dict(dict(R=R0, t=t0, s=ids, g=ids, p=q), **kw)
        assert begin(0, 3, args["R"], args["t"], args["s"], args["g"], args["p"]) == api.E_INVALID, kw
    assert begin(0, 3, R0, t0, ids, ids, q) == api.E_STATE               # valid arguments: the state is next


def test_the_plan_counts_what_the_voxel_build_allocates_and_never_splits_a_pair():
    L = api.load()
    blob = _Ctx()
    ctx = C.c_void_p(C.addressof(blob))
    counts = [1000, 4000, 0, 2500, 4000, 10, 3999]
    one = lambda m: PER_TARGET + PER_POINT * m
    # a budget that holds the largest target alone, and no two of the large ones: the 4 000-point targets stand alone (a pair is never
    # split: a batch always holds whole targets), the small ones ride with a neighbour while they fit
    budget = one(4000) + 600.0                      # ... and an empty target beside it, not a 10-point one
    assert L.dcreg_set_option(ctx, b"pairs_max_bytes", C.c_double(budget)) == api.OK
    ends = _plan(L, ctx, counts)
    assert ends[-1] == len(counts) and ends == sorted(set(ends))
    first = [0] + ends[:-1]
    for a, b in zip(first, ends):
        assert b > a
        assert b - a == 1 or sum(one(m) for m in counts[a:b]) <= budget, (a, b)      # a batch never exceeds its budget
        if b < len(counts):
            assert sum(one(m) for m in counts[a:b + 1]) > budget, (a, b)              # ... and closes only when the next target does not fit
    assert [counts[a:b] for a, b in zip(first, ends)] == [[1000], [4000, 0], [2500], [4000], [10], [3999]]
    # one target at a time
    assert L.dcreg_set_option(ctx, b"pairs_max_bytes", C.c_double(1.0)) == api.OK
    assert _plan(L, ctx, counts) == list(range(1, len(counts) + 1))
    # everything in one batch; the stride is part of the count
    assert L.dcreg_set_option(ctx, b"pairs_max_bytes", C.c_double(sum(one(m) for m in counts))) == api.OK
    assert _plan(L, ctx, counts) == [len(counts)]
    assert len(_plan(L, ctx, counts, stride=4)) == 2
    assert _plan(L, ctx, []) == []
    # bad arguments
    ends_i, nb = (C.c_int32 * len(counts))(), C.c_int(-1)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert L.dcreg_pairs_plan_voxels(ctx, -1, off.ctypes.data_as(I64P), 3, ends_i, C.byref(nb)) == api.E_INVALID
    assert L.dcreg_pairs_plan_voxels(ctx, 3, None, 3, ends_i, C.byref(nb)) == api.E_INVALID
    assert L.dcreg_pairs_plan_voxels(ctx, 3, off.ctypes.data_as(I64P), 3, None, C.byref(nb)) == api.E_INVALID
    assert L.dcreg_pairs_plan_voxels(ctx, 3, off.ctypes.data_as(I64P), 3, ends_i, None) == api.E_INVALID


def test_the_voxel_box_of_float_bounds_is_refused_as_a_build_refuses_it():
    """the host check of dcreg_register_pairs_voxels for the targets of its later build batches: the voxels of the coordinate-wise minimum
    and maximum (leaf 2^-7: voxel = x * 128 exactly)"""
    L = api.load()
    L.dcreg_last_error.restype = C.c_char_p
    blob = _Ctx()
    ctx = C.c_void_p(C.addressof(blob))
    leaf = 2.0 ** -7

    def check(lo, hi, lf=leaf):
        a, b = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        return L.dcreg_pairs_voxels_box_check(ctx, a.ctypes.data_as(FP), b.ctypes.data_as(FP), lf, 5)

    lo = -(1 << 20) * leaf
    widest = ((1 << 20) - 2) * leaf                 # voxels -2^20 .. 2^20 - 2: 2^21 - 1 of them, the most that is taken
    assert check([lo] * 3, [widest] * 3) == api.OK
    assert check([lo] * 3, [widest + 0.5 * leaf] * 3) == api.OK
    for axis in range(3):
        hi = [widest] * 3
        hi[axis] = widest + leaf                    # 2^21 voxels on this axis
        assert check([lo] * 3, hi) == api.E_INVALID
        assert b"pair target 5 spans 2097152 voxels on axis %d" % axis in L.dcreg_last_error(ctx)
    assert check([0.0] * 3, [0.0] * 3) == api.OK
    assert check([-1e30, 0, 0], [-1e30, 0, 0], 1e-12) == api.E_INVALID and b"2^62" in L.dcreg_last_error(ctx)
    assert check([0, 0, 3e38], [0, 0, 3e38], 1.0) == api.E_INVALID and b"2^62" in L.dcreg_last_error(ctx)
    assert check([0, 0, 4.0e18], [0, 0, 4.0e18], 1.0) == api.OK           # below 2^62 = 4.6e18
    assert L.dcreg_pairs_voxels_box_check(ctx, None, None, 1.0, 0) == api.E_INVALID


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_the_methods_check_their_arguments():
    c = _ctx()
    cfg = api.default_config()
    f = [np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32)]
    with pytest.raises(ValueError, match="one target per source"):
        c.register_pairs_voxels(f, f[:1], [I4, I4], "Ours", cfg)
    with pytest.raises(ValueError, match="one initial pose per pair"):
        c.register_pairs_voxels(f, f, [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="float32"):
        c.register_pairs_voxels([np.zeros((4, 3))], f[:1], [I4], "Ours", cfg)
    with pytest.raises(ValueError, match="columns"):
        c.register_pairs_voxels(f, [f[0], np.zeros((4, 4), np.float32)], [I4, I4], "Ours", cfg)
    with pytest.raises(ValueError, match="voxel_map_params"):
        c.register_pairs_voxels(f, f, [I4, I4], "Ours", cfg, target_voxels=5)
    with pytest.raises(ValueError, match="normal_params"):
        c.register_pairs_voxels(f, f, [I4, I4], "Ours", cfg, source_normals=5)
    bad_n = api.normal_params()
    bad_n.k = 40
    with pytest.raises(ValueError, match="k in"):
        c.register_pairs_voxels(f, f, [I4, I4], "Ours", cfg, source_normals=bad_n)
    for field, value, text in (("leaf", 0.0, "leaf"), ("leaf", np.nan, "leaf"), ("leaf", np.inf, "leaf"), ("epsilon", 0.5e-6, "epsilon"),
                               ("epsilon", 1.5, "epsilon"), ("min_points", 1, "min_points")):
        bad = _block(field, value)
        with pytest.raises(ValueError, match=text):
            c.register_pairs_voxels(f, f, [I4, I4], "Ours", cfg, target_voxels=bad)
        with pytest.raises(ValueError, match=text):
            c.pairs_voxels_build(f, bad)
    with pytest.raises(ValueError, match="float32"):
        c.pairs_voxels_build([np.zeros((4, 3))])
    with pytest.raises(ValueError, match="columns"):
        c.pairs_voxels_build([f[0], np.zeros((4, 4), np.float32)])
    euler = api.default_lin_params(0.5, euler_rpy=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="parameterization"):
        c.pairs_voxels_batch_begin([I4], [0], [0], params=euler)
    with pytest.raises(ValueError):
        c.pairs_voxels_batch_begin([I4, I4], [0], [0, 1])                # one source id per pose
