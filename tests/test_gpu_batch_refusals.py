"""The refusal ladders of the six batched launches of the second, third and fourth engine (include/dcreg_debug.h:
dcreg_normals_batch_begin, dcreg_gicp_batch_begin, dcreg_pairs_normals_batch_begin, dcreg_pairs_gicp_batch_begin, dcreg_voxels_batch_begin,
dcreg_pairs_voxels_batch_begin), rung by rung in the header's order: every rung is one raw call with exactly that defect and every later
condition satisfied, and is checked by its return code and a distinguishing part of dcreg_last_error.  After every refusal nothing is
queued: _end on the slot finds nothing in flight, and a valid _begin / _end on the same slot returns the sums of a fresh context, bitwise.
Calls with two defects pin the order where the launches differ.  The codes and texts are written out by hand from the header and the
sources; the clouds are the smallest that reach every rung (a 300-point target, a 100-point source, frames of 70 and 0 points, pair
targets of which one is empty or keeps no voxel)."""
import ctypes as C
import functools

import numpy as np
import pytest

from dcreg_amd import api

pytestmark = pytest.mark.gpu

RADIUS = 1.0
I32P = C.POINTER(C.c_int32)
INVALID, STATE = api.E_INVALID, api.E_STATE
KINDS = ("normals", "gicp", "pairs_normals", "pairs_gicp", "voxels", "pairs_voxels")
PAIRS = ("pairs_normals", "pairs_gicp", "pairs_voxels")
VOXELS = ("voxels", "pairs_voxels")
END = {"normals": "dcreg_normals_batch_end", "gicp": "dcreg_gicp_batch_end", "pairs_normals": "dcreg_normals_batch_end",
       "pairs_gicp": "dcreg_normals_batch_end", "voxels": "dcreg_voxels_batch_end", "pairs_voxels": "dcreg_voxels_batch_end"}
WHAT = {k: ("voxel" if k in VOXELS else "normal") for k in KINDS}      # (the GICP launches say "normal" too: they share the second engine's begin)
NOUN = {k: ("pair source" if k == "pairs_voxels" else "frame") for k in KINDS}
NORMALS_5 = api.normal_params(k=5)
VOXEL_MAP = api.voxel_map_params(1.0, 1.0e-3, 6)


@functools.lru_cache(None)
def clouds():
    rng = np.random.default_rng(20)
    tgt = (rng.random((300, 3)) * np.array([3.0, 3.0, 0.2])).astype(np.float32)          # a slab: 9 voxels of leaf 1 with ~33 points each
    src = (tgt[:100] + rng.normal(0.0, 0.01, (100, 3))).astype(np.float32)
    frame = (tgt[100:170] + rng.normal(0.0, 0.01, (70, 3))).astype(np.float32)
    empty = np.zeros((0, 3), np.float32)
    few = tgt[:5].copy()                                                                 # a target that keeps no voxel (min_points 6)
    return {"tgt": tgt, "src": src, "frame": frame, "empty": empty, "few": few}


def poses(n=2):
    Ts = np.tile(np.eye(4), (n, 1, 1))
    Ts[:, 0, 3] = 0.01 * (1 + np.arange(n) % 3)
    return Ts


def lin_params(radius=RADIUS):
    return api.default_lin_params(radius, 1)


def prepare(c, kind, mode=0):
    """everything the kind's valid launch needs (and a target and a source for the first engine's launches of the state rungs)"""
    K = clouds()
    c.set_target(K["tgt"], RADIUS)
    c.set_source(K["src"])
    if kind in ("normals", "gicp"):
        c.keep_target_normals(NORMALS_5)
        c.frames_load([K["frame"], K["empty"]])
        if kind == "gicp":
            c.keep_source_normals(NORMALS_5)
            c.frames_normals_keep(NORMALS_5)
    elif kind in ("pairs_normals", "pairs_gicp"):
        c.pairs_sources_load([K["src"], K["empty"]])
        c.pairs_build([K["tgt"], K["empty"]], RADIUS)
        c.pairs_normals_keep(NORMALS_5)
        if kind == "pairs_gicp":
            c.pairs_sources_normals_keep(NORMALS_5)
    elif kind == "voxels":
        c.keep_target_voxels(VOXEL_MAP)
        c.frames_load([K["frame"], K["empty"]])
    else:
        c.pairs_sources_load([K["src"], K["empty"]])
        c.pairs_voxels_build([K["tgt"], K["few"]], VOXEL_MAP)
    if mode:
        c.set_option("voxels_source_cov", 1)


def begin(c, kind, h="ctx", slot=0, n=None, Ts=None, R9="poses", t3="poses", states=None, ids=(0, 0), tids=(0, 0), prm="default"):
    """the raw call: the valid launch of the kind (two poses, both on cloud 0 and target 0) with the given arguments replaced"""
    Rs, ts, m = api._poses_arg(poses() if Ts is None else Ts)
    n = m if n is None else n
    i32 = lambda a: None if a is None else np.ascontiguousarray(np.resize(np.asarray(a, np.int32), max(m, 1)))
    ptr = lambda a: None if a is None else a.ctypes.data_as(I32P)
    st, f, t = i32(states), i32(ids), i32(tids)
    p = lin_params() if isinstance(prm, str) else prm
    head = (c._h if h == "ctx" else h, slot, n, api._dp(Rs) if isinstance(R9, str) else R9, api._dp(ts) if isinstance(t3, str) else t3)
    tail = (None if p is None else C.byref(p),)
    L = c._L
    if kind in ("normals", "gicp"):
        return getattr(L, "dcreg_%s_batch_begin" % kind)(*head, ptr(st), ptr(f), *tail)
    if kind in ("pairs_normals", "pairs_gicp"):
        return getattr(L, "dcreg_%s_batch_begin" % kind)(*head, ptr(st), ptr(f), ptr(t), *tail)
    if kind == "voxels":
        return L.dcreg_voxels_batch_begin(*head, ptr(f), *tail)
    return L.dcreg_pairs_voxels_batch_begin(*head, ptr(f), ptr(t), *tail)


def end(c, kind, slot=0, n=2):
    outs = (api.LinOut * n)()
    rc = getattr(c._L, END[kind])(c._h, slot, outs)
    return rc, [(bytes(o.H_upper), bytes(o.g), o.sum_r2, o.sum_b2, o.n_eff, o.n_pt) for o in outs]


def last_error(c):
    return c._L.dcreg_last_error(c._h).decode()


@functools.lru_cache(None)
def fresh(kind):
    """the sums of the kind's valid launch on a context that has seen nothing else"""
    c = api.Context(0)
    try:
        prepare(c, kind)
        assert begin(c, kind) == api.OK, last_error(c)
        rc, sums = end(c, kind)
        assert rc == api.OK and sums[0][4] > 10, (rc, sums[0][4:])              # (the launch is not an empty one)
        return sums
    finally:
        c.close()


def refused(c, kind, code, text, valid_after=True, exact=False, **defect):
    rc = begin(c, kind, **defect)
    msg = last_error(c)
    assert rc == code and (msg == text if exact else text in msg), (kind, defect.keys(), rc, msg)
    nothing_queued(c, kind, defect.get("slot", 0), valid_after)


def nothing_queued(c, kind, slot=0, valid_after=True):
    for s in {0, 1, slot} & {0, 1}:
        rc, _ = end(c, kind, s)
        assert rc == STATE and "has no batched normal linearisation in flight" in last_error(c), (kind, s, rc, last_error(c))
    if valid_after:
        s = slot if slot in (0, 1) else 0
        assert begin(c, kind, slot=s) == api.OK, (kind, last_error(c))
        rc, sums = end(c, kind, s)
        assert rc == api.OK and sums == fresh(kind), kind


def nan_pose():
    Ts = poses()
    Ts[1, 1, 3] = np.nan
    return Ts


# ---- 1. the front of the ladder, the same for the six launches but for what the header says: arguments, slots, parameters, poses
@pytest.mark.parametrize("kind", KINDS)
def test_the_front_of_the_ladder_rung_by_rung(kind):
    K = clouds()
    one_nn = kind not in VOXELS
    euler = api.default_lin_params(RADIUS, euler_rpy=(0.0, 0.0, 0.0))
    so3 = "the %s linearisation has the SO(3) row only" % WHAT[kind]
    c = api.Context(0)
    try:
        prepare(c, kind)
        assert begin(c, kind, h=None) == INVALID                                         # a null context: no text to leave anywhere
        nothing_queued(c, kind)
        if kind in ("pairs_normals", "pairs_gicp"):                                      # the 1-NN pairs launches: null ids before anything else
            refused(c, kind, INVALID, "null argument", exact=True, ids=None, slot=2)
            refused(c, kind, INVALID, "null argument", exact=True, tids=None, n=0)
        for slot in (2, -1):
            refused(c, kind, INVALID, "invalid slot %d" % slot, slot=slot)
        if kind == "pairs_voxels":                                                       # ... the voxel pairs launch: with the null arguments
            refused(c, kind, INVALID, "invalid slot 2", ids=None, slot=2)
            refused(c, kind, INVALID, "null linearisation arguments", ids=None)
            refused(c, kind, INVALID, "null linearisation arguments", tids=None)
        for defect in ({"R9": None}, {"t3": None}, {"prm": None}, {"n": 0}, {"n": -1}):
            refused(c, kind, INVALID, "null linearisation arguments", **defect)
        refused(c, kind, INVALID, "null linearisation arguments", n=70000, prm=None)     # (before the count is looked at)
        refused(c, kind, INVALID, "at most 65535 poses per batched launch (grid.y limit), got 65536", Ts=poses(65536))
        # a waiting gate, a pending slot of the first engine, the slot itself pending
        c.linearize_gated_begin(lin_params(), slot=1)
        refused(c, kind, STATE, "a gated linearisation still waits for its pose", valid_after=False)
        refused(c, kind, STATE, "a gated linearisation still waits for its pose", valid_after=False, prm=euler, Ts=nan_pose())
        c.gate_abort()
        nothing_queued(c, kind)
        c.linearize_begin(np.eye(3), np.zeros(3), lin_params(), slot=1)
        refused(c, kind, STATE, "a linearisation is still in flight", valid_after=False)
        c.linearize_end(slot=1)
        nothing_queued(c, kind)
        for slot in (0, 1):
            assert begin(c, kind, slot=slot) == api.OK
            rc = begin(c, kind, slot=slot, prm=euler)
            assert rc == STATE and "slot %d still has a batched normal linearisation in flight" % slot in last_error(c), (rc, last_error(c))
            rc, sums = end(c, kind, slot)
            assert rc == api.OK and sums == fresh(kind)                                  # the refused call changed nothing of the pending one
        # the parameter block and the poses
        refused(c, kind, INVALID, so3, prm=euler)
        refused(c, kind, INVALID, so3, prm=euler, Ts=nan_pose())                         # the parameterization before the poses
        for r in (0.0, -1.0, np.nan, np.inf):
            bad = lin_params()
            bad.search_radius = r
            if one_nn:
                refused(c, kind, INVALID, "search_radius is", prm=bad)
                refused(c, kind, INVALID, "search_radius is", prm=bad, Ts=nan_pose())    # ... the radius between them
                bad.parameterization = euler.parameterization
                refused(c, kind, INVALID, so3, prm=bad)
            else:                                                                        # the voxel launches do not read it
                assert begin(c, kind, prm=bad) == api.OK, last_error(c)
                rc, sums = end(c, kind)
                assert rc == api.OK and sums == fresh(kind)
        refused(c, kind, INVALID, "a pose is not finite", Ts=nan_pose())
        Ts = poses()
        Ts[0, 0, 0] = np.inf
        refused(c, kind, INVALID, "a pose is not finite", Ts=Ts)
        # a non-finite pose before any state refusal: the same call on a context that has nothing
        bare = api.Context(0)
        try:
            rc = begin(bare, kind, Ts=nan_pose())
            assert rc == INVALID and "a pose is not finite" in last_error(bare), (rc, last_error(bare))
        finally:
            bare.close()
    finally:
        c.close()
    assert K["tgt"].shape == (300, 3)


# ---- 2. the state refusals and the clouds, each launch its own
@pytest.mark.parametrize("kind", ["normals", "gicp"])
def test_the_one_nn_launches_state_rungs(kind):
    K = clouds()
    c = api.Context(0)
    try:
        c.set_source(K["src"])
        refused(c, kind, STATE, "no target: dcreg_set_target first", valid_after=False, ids=None)
        refused(c, kind, STATE, "no target: dcreg_set_target first", valid_after=False)
        c.set_target(K["tgt"], RADIUS)
        refused(c, kind, STATE, "no kept normals: dcreg_target_normals_keep or dcreg_target_normals_set first", valid_after=False)
        c.keep_target_normals(NORMALS_5)
        refused(c, kind, STATE, "no frames: dcreg_frames_load first", valid_after=False)
        c.frames_load([K["frame"], K["empty"]])
        if kind == "gicp":
            refused(c, kind, INVALID, "frame 2 is not loaded or empty", valid_after=False, ids=(0, 2))     # the ids before the kept normals
            refused(c, kind, STATE, "no kept frame normals: dcreg_frames_normals_keep or dcreg_frames_normals_set first", valid_after=False)
            refused(c, kind, STATE, "no kept source normals: dcreg_source_normals_keep or dcreg_source_normals_set first", valid_after=False, ids=None)
            c.frames_normals_keep(NORMALS_5)
            refused(c, kind, STATE, "no kept source normals", ids=None)                  # the frames' are not the source's
            c.keep_source_normals(NORMALS_5)
        for bad in (2, -1, 1):                                                           # outside the load, and the empty frame
            refused(c, kind, INVALID, "frame %d is not loaded or empty" % bad, ids=(0, bad))
        # the warm slots, last
        refused(c, kind, INVALID, "warm slot 0 was not reserved", states=(-1, 0))
        refused(c, kind, INVALID, "frame 2 is not loaded or empty", states=(-1, 0), ids=(0, 2))
        c.normals_reserve_slots(1, frames=True)
        refused(c, kind, INVALID, "warm slot 0 is used by two poses of one launch", states=(0, 0))
        refused(c, kind, INVALID, "warm slot 1 was not reserved", states=(0, 1))
        refused(c, kind, INVALID, "the warm slots were reserved for other clouds", states=(0, -1), ids=None)
        # no source: the launch over the own source only
        n = api.Context(0)
        try:
            n.set_target(K["tgt"], RADIUS)
            n.keep_target_normals(NORMALS_5)
            refused(n, kind, STATE, "no source: dcreg_set_source first", valid_after=False, ids=None)
        finally:
            n.close()
    finally:
        c.close()


@pytest.mark.parametrize("kind", ["pairs_normals", "pairs_gicp"])
def test_the_one_nn_pairs_launches_state_rungs(kind):
    K = clouds()
    c = api.Context(0)
    try:
        c.pairs_sources_load([K["src"], K["empty"]])
        refused(c, kind, STATE, "no pair batch built: dcreg_pairs_build first", valid_after=False)
        c.pairs_build([K["tgt"], K["empty"]], RADIUS)
        refused(c, kind, STATE, "no kept pair normals: dcreg_pairs_normals_keep or dcreg_pairs_normals_set first", valid_after=False)
        refused(c, kind, STATE, "no kept pair normals", valid_after=False, prm=lin_params(2.0 * RADIUS), tids=(0, 2))
        c.pairs_normals_keep(NORMALS_5)
        if kind == "pairs_gicp":
            refused(c, kind, INVALID, "frame 2 is not loaded or empty", valid_after=False, ids=(0, 2))
            refused(c, kind, STATE, "no kept pair source normals: dcreg_pairs_sources_normals_keep or dcreg_pairs_sources_normals_set first",
                    valid_after=False)
            c.pairs_sources_normals_keep(NORMALS_5)
        refused(c, kind, INVALID, "the pair targets were built for another search radius", prm=lin_params(2.0 * RADIUS))
        refused(c, kind, INVALID, "the pair targets were built for another search radius", prm=lin_params(2.0 * RADIUS), tids=(0, 2))
        for bad in (2, -1, 1):                                                           # outside the batch, and the empty target
            refused(c, kind, INVALID, "pair target %d is not built" % bad, tids=(0, bad))
        for bad in (2, -1, 1):                                                           # (these launches call a pair source a frame)
            refused(c, kind, INVALID, "frame %d is not loaded or empty" % bad, ids=(0, bad))
        # every target before any source, whichever pose it belongs to
        refused(c, kind, INVALID, "pair target 2 is not built", ids=(0, 3), tids=(2, 0))
        refused(c, kind, INVALID, "pair target 2 is not built", ids=(3, 0), tids=(0, 2))
        refused(c, kind, INVALID, "warm slot 0 was not reserved", states=(0, -1))
        n = api.Context(0)
        try:
            n.pairs_build([K["tgt"], K["empty"]], RADIUS)
            n.pairs_normals_keep(NORMALS_5)
            refused(n, kind, STATE, "no pair sources: dcreg_pairs_sources_load first", valid_after=False)
            refused(n, kind, INVALID, "pair target 2 is not built", valid_after=False, tids=(0, 2))
        finally:
            n.close()
    finally:
        c.close()


def test_the_voxel_launch_state_rungs():
    K = clouds()
    kind = "voxels"
    c = api.Context(0)
    try:
        c.set_source(K["src"])
        refused(c, kind, STATE, "no target: dcreg_set_target first", valid_after=False)
        c.set_target(K["tgt"], RADIUS)
        refused(c, kind, STATE, "no kept voxels: dcreg_target_voxels_keep first", valid_after=False)
        refused(c, kind, STATE, "no kept voxels: dcreg_target_voxels_keep first", valid_after=False, ids=None)
        c.keep_target_voxels(VOXEL_MAP)
        refused(c, kind, STATE, "no frames: dcreg_frames_load first", valid_after=False)
        c.frames_load([K["frame"], K["empty"]])
        for bad in (2, -1, 1):
            refused(c, kind, INVALID, "frame %d is not loaded or empty" % bad, ids=(0, bad))
        c.set_option("voxels_source_cov", 1)
        refused(c, kind, INVALID, "frame 2 is not loaded or empty", valid_after=False, ids=(0, 2))
        refused(c, kind, STATE, "no kept frame normals: dcreg_frames_normals_keep or dcreg_frames_normals_set first", valid_after=False)
        refused(c, kind, STATE, "no kept source normals: dcreg_source_normals_keep or dcreg_source_normals_set first", valid_after=False, ids=None)
        c.set_option("voxels_source_cov", 0)
        nothing_queued(c, kind)
        n = api.Context(0)
        try:
            n.set_target(K["tgt"], RADIUS)
            n.keep_target_voxels(VOXEL_MAP)
            refused(n, kind, STATE, "no source: dcreg_set_source first", valid_after=False, ids=None)
        finally:
            n.close()
    finally:
        c.close()


def test_the_voxel_pairs_launch_state_rungs():
    K = clouds()
    kind = "pairs_voxels"
    c = api.Context(0)
    try:
        refused(c, kind, STATE, "no pair voxel batch built: dcreg_pairs_voxels_build first", valid_after=False)
        infos = c.pairs_voxels_build([K["tgt"], K["few"]], VOXEL_MAP)
        assert infos[0]["n_kept"] >= 4 and infos[1]["n_kept"] == 0
        refused(c, kind, STATE, "no pair sources: dcreg_pairs_sources_load first", valid_after=False)
        c.pairs_sources_load([K["src"], K["empty"]])
        for bad in (2, -1, 1):                                                           # outside the load, and the empty source
            refused(c, kind, INVALID, "pair source %d is not loaded or empty" % bad, ids=(0, bad))
        for bad in (2, -1):
            refused(c, kind, INVALID, "pair target %d is not in the voxel batch" % bad, tids=(0, bad))
        # pose by pose, a pose's source before its target
        refused(c, kind, INVALID, "pair target 2 is not in the voxel batch", ids=(0, 3), tids=(2, 0))
        refused(c, kind, INVALID, "pair source 3 is not loaded or empty", ids=(3, 0), tids=(0, 2))
        refused(c, kind, INVALID, "pair source 3 is not loaded or empty", ids=(3, 0), tids=(2, 0))
        # a target without a member is no refusal: the zero row
        assert begin(c, kind, tids=(0, 1)) == api.OK, last_error(c)
        rc, sums = end(c, kind)
        assert rc == api.OK and sums[0] == fresh(kind)[0]
        assert sums[1] == (bytes(21 * 8), bytes(6 * 8), 0.0, 0.0, 0, 0)
        c.set_option("voxels_source_cov", 1)
        refused(c, kind, INVALID, "pair target 2 is not in the voxel batch", valid_after=False, tids=(0, 2))
        refused(c, kind, STATE, "no kept pair source normals: dcreg_pairs_sources_normals_keep or dcreg_pairs_sources_normals_set first",
                valid_after=False)
        c.set_option("voxels_source_cov", 0)
        nothing_queued(c, kind)
    finally:
        c.close()
