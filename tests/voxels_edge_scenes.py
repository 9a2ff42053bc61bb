"""Scenes of the fourth engine's edge tests (tests/test_voxels_edge_scenes.py, test_gpu_voxels_edges.py): leaves that binary cannot
represent with points at and next to the voxel faces, a map whose voxel box is as wide as the key allows (and one voxel wider), lookup
tables of two slots and around a doubling, one voxel of 20 000 points, and the parking lot 1e5 m from the origin.  Every scene carries its
reference voxel map (tests/voxels_ref.py); everything is computed once per process and never modified."""
import functools

import numpy as np

import normal_icp_scenes as sc
import voxels_ref as vr
import voxels_scenes as vs

frozen = sc.frozen


# ---- 1. a leaf that binary cannot represent
# The rule is v = floor((double)q / leaf), an IEEE double division.  Two cheaper computations that a kernel could slip into:
def voxel_float_division(x, leaf):
    """floor(q / (float)leaf) in float32"""
    return np.floor(np.asarray(x, np.float32) / np.float32(leaf)).astype(np.float64)


def voxel_reciprocal(x, leaf):
    """floor((double)q * (1.0 / leaf))"""
    return np.floor(np.asarray(x, np.float32).astype(np.float64) * (np.float64(1.0) / np.float64(leaf)))


def face_floats(leaf, reach=2000.0):
    """-> (k [m], x [m, 3] float32): for every face k * leaf with |k * leaf| < reach the float32 nearest to it and its two neighbours"""
    kmax = int(reach / leaf) - 1
    k = np.arange(-kmax, kmax + 1)
    mid = (k.astype(np.float64) * np.float64(leaf)).astype(np.float32)
    x = np.stack([np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))], axis=1)
    return k, x


def teeth(x, leaf, alt):
    """which float32 values land in another voxel under the computation alt than under the rule"""
    return alt(x, leaf) != vr.voxel_of(np.asarray(x, np.float32).reshape(-1, 1), leaf).reshape(np.shape(x))


LEAF_SCENES = {0.1: (voxel_float_division, 240), 0.7: (voxel_reciprocal, 102)}      # leaf -> (the computation it has teeth for, faces)
LEAF_MIN_POINTS = 2                                   # a misassigned point changes a kept record's count and mean
CROSS = 3                                             # the voxel coordinate of a face's points on the other two axes


@functools.lru_cache(maxsize=None)
def leafy(leaf):
    """-> dict tgt, src, src_normals, T (identity), vmap, leaf, params (leaf, EPS, 2), faces (axis, k), n_face (the first n_face points of
    src are the face floats).  Per chosen face k * leaf of an axis - those where one of the three floats at the face changes voxel under
    LEAF_SCENES' cheaper computation, spread evenly over +-2000 m and dealt to the three axes in turn - the map holds the three floats and
    two interior points of the voxel on either side, all inside voxel CROSS of the other two axes: both voxels reach min_points = 2
    wherever the floats fall, so a float in the wrong voxel moves two kept records.  The source is the face floats again and points one
    voxel outside the map's box; at the identity pose body_to_global returns the point itself."""
    alt, n_faces = LEAF_SCENES[leaf]
    rng = np.random.default_rng(int(round(leaf * 1000)))
    k, x = face_floats(leaf)
    has = np.flatnonzero(teeth(x, leaf, alt).any(axis=1))
    pick = has[np.unique(np.linspace(0, len(has) - 1, n_faces).astype(np.int64))]
    lf = np.float64(leaf)
    tgt, face, faces = [], [], []
    for j, i in enumerate(pick):
        a = j % 3
        for xa in x[i]:                                                # the three floats at the face
            p = (rng.uniform(CROSS + 0.2, CROSS + 0.8, 3) * lf).astype(np.float32)
            p[a] = xa
            tgt.append(p); face.append(p)
        for side in (-1, 0):                                           # two interior points of voxel k - 1 and of voxel k
            for _ in range(2):
                p = (rng.uniform(CROSS + 0.2, CROSS + 0.8, 3) * lf).astype(np.float32)
                p[a] = np.float32((k[i] + side + rng.uniform(0.3, 0.7)) * lf)
                tgt.append(p)
        faces.append((a, int(k[i])))
    tgt = np.array(tgt, np.float32)
    tgt = tgt[rng.permutation(len(tgt))]
    lo, hi = vs.box_of(tgt, leaf)
    out = []
    for a in range(3):                                                 # one voxel outside each face of the map's box
        for v in (lo[a] - 1, hi[a] + 1):
            p = (rng.uniform(CROSS + 0.2, CROSS + 0.8, 3) * lf).astype(np.float32)
            p[a] = np.float32((v + 0.5) * lf)
            out.append(p)
    src = np.concatenate([np.array(face, np.float32), np.array(out, np.float32)])
    nrm = np.array(sc.unit_normals(len(src), 7 + len(src)))
    nrm[5::11, 2] = np.nan
    vmap = vr.voxel_map(tgt, leaf, vs.EPS, LEAF_MIN_POINTS)
    return dict(tgt=frozen(tgt), src=frozen(src), src_normals=frozen(nrm), T=frozen(np.eye(4)), vmap=vmap, leaf=leaf, faces=faces,
                n_face=len(face), alt=alt, params=(leaf, vs.EPS, LEAF_MIN_POINTS))


# ---- 2. key widths at the limit
WIDE_LEAF = 2.0 ** -7
WIDE_GRID = 2.0 ** -10                                # eight steps per voxel; exact in float32 up to 8 192 m
WIDE_LO = -(1 << 20)
WIDE_SPAN_MAX = (1 << 21) - 1                         # include/dcreg.h: 2^21 or more voxels on an axis are refused
# the same map seen through a leaf a little smaller: voxel -2^20 splits, the box grows by one voxel to 2^21 (see wide())
WIDE_LEAF_ONE_MORE = WIDE_LEAF * (1.0 - 2.0 ** -22)


def _cluster(rng, v, n, first=None, kmax=8):
    """n distinct points of voxel v on the 2^-10 grid (steps 0 .. kmax - 1 per axis), `first` among them"""
    steps = set() if first is None else {tuple(first)}
    while len(steps) < n:
        steps.add(tuple(int(s) for s in rng.integers(0, kmax, 3)))
    steps = sorted(steps)
    return (np.asarray(v, np.float64) * WIDE_LEAF + np.array(steps, np.float64) * WIDE_GRID).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wide(top):
    """-> dict tgt (27 points), src, src_normals, T (identity), T_step (a translation by grid steps), vmap, span.  Clusters of 6 points in
    the voxels (lo, lo, lo), (top, top, top), (lo, top, 0) and 9 in (0, 0, 0), leaf 2^-7, lo = -2^20.  top = 2^20 - 2: the box is 2^21 - 1
    voxels wide on every axis, the widest the library takes - 21 bits per axis, 63 bits of voxel key, with the cloud bit a 64-bit sort
    key; top = 2^20 - 1: 2^21 voxels, refused.  The cluster in (lo, lo, lo) holds the voxel's own corner and the one in (top, top, top)
    stays in the lower 6/8 of its voxel: through WIDE_LEAF_ONE_MORE the corner falls into voxel -2^20 - 1 and nothing else moves up, so
    the SAME points span one voxel more.  The source: points in all eight corner voxels of the box, one voxel outside each of its faces, in
    the kept voxel at the origin and in the empty interior."""
    rng = np.random.default_rng(2100 + (top & 3))
    lo = WIDE_LO
    parts = [_cluster(rng, (lo, lo, lo), 6, first=(0, 0, 0)), _cluster(rng, (top, top, top), 6, kmax=6), _cluster(rng, (lo, top, 0), 6),
             _cluster(rng, (0, 0, 0), 9)]
    tgt = np.concatenate(parts)
    tgt = tgt[rng.permutation(len(tgt))]
    vox = [(a, b, c) for a in (lo, top) for b in (lo, top) for c in (lo, top)]            # the eight corners (two of them kept)
    vox += [(lo, top, 0), (0, 0, 0), (0, 0, 0), (5, -7, 11), (lo + 1, lo, lo), (top - 1, top, top), (lo, top, 1), (1 << 19, -(1 << 19), 3)]
    for a in range(3):                                                                     # one voxel outside each face
        for v in (lo - 1, top + 1):
            w = [lo, top, 0]
            w[a] = v
            vox.append(tuple(w))
    src = np.concatenate([_cluster(rng, v, 3) for v in vox])
    nrm = np.array(sc.unit_normals(len(src), 88))
    nrm[4::9, 0] = np.nan
    step = np.eye(4)
    step[:3, 3] = [3 * WIDE_GRID, -2 * WIDE_GRID, 5 * WIDE_GRID]
    vmap = vr.voxel_map(tgt, WIDE_LEAF, vs.EPS, vs.MIN_POINTS)
    mn, mx = vs.box_of(tgt, WIDE_LEAF)
    return dict(tgt=frozen(tgt), src=frozen(src), src_normals=frozen(nrm), T=frozen(np.eye(4)), T_step=frozen(step), vmap=vmap,
                span=tuple(int(s) for s in (mx - mn + 1)))


# ---- 3. table sizes and a full voxel
@functools.lru_cache(maxsize=None)
def single():
    """one cluster of 9 points in voxel (3, -2, 0): n_kept = 1, a table of two slots (mask 1).  The source: points in it, in its 26
    neighbours and far outside"""
    rng = np.random.default_rng(31)
    tgt = vs._in_voxel(rng, (3, -2, 0), 9)
    nb = [(3 + a, -2 + b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    src = np.concatenate([vs._in_voxel(rng, v, 2) for v in nb] + [vs._in_voxel(rng, (3, -2, 0), 20), np.float32([[40.0, 0.5, 0.5], [3.5, -1.5, -9.5]])])
    vmap = vr.voxel_map(tgt, vs.LEAF, vs.EPS, vs.MIN_POINTS)
    assert vmap["n_kept"] == 1
    return dict(tgt=frozen(tgt), src=frozen(src), src_normals=sc.unit_normals(len(src), 32), T=frozen(np.eye(4)), vmap=vmap)


LATTICE_EXTRA = (16, 3, 9)                            # beside the lattice's box of 16^3 voxels
LATTICE_MISSING = (5, 7, 3)


def _lattice_source(rng):
    L = vs.lattice()
    more = np.concatenate([vs._in_voxel(rng, LATTICE_EXTRA, 8), vs._in_voxel(rng, LATTICE_MISSING, 8)])
    return frozen(np.concatenate([L["src"], more])), sc.unit_normals(len(L["src"]) + len(more), 93)


@functools.lru_cache(maxsize=None)
def lattice_plus():
    """voxels_scenes.lattice() and six points in one more voxel: n_kept = 4 097, the table doubles to 16 384 slots.  The source: the
    lattice's, and points in the added voxel and in the one lattice_minus() lacks"""
    rng = np.random.default_rng(78)
    L = vs.lattice()
    tgt = np.concatenate([L["tgt"], vs._in_voxel(rng, LATTICE_EXTRA, 6)])
    tgt = tgt[rng.permutation(len(tgt))]
    src, nrm = _lattice_source(rng)
    vmap = vr.voxel_map(tgt, vs.LEAF, vs.EPS, vs.MIN_POINTS)
    assert vmap["n_kept"] == 4097
    return dict(tgt=frozen(tgt), src=src, src_normals=nrm, T=L["T"], vmap=vmap)


@functools.lru_cache(maxsize=None)
def lattice_minus():
    """voxels_scenes.lattice() without one point of voxel LATTICE_MISSING: five are left, it is not kept, n_kept = 4 095 (8 192 slots)"""
    rng = np.random.default_rng(78)
    L = vs.lattice()
    inside = np.flatnonzero((vr.voxel_of(L["tgt"], vs.LEAF) == np.array(LATTICE_MISSING, np.float64)).all(axis=1))
    assert len(inside) == 6
    tgt = np.delete(L["tgt"], inside[2], axis=0)
    src, nrm = _lattice_source(rng)
    vmap = vr.voxel_map(tgt, vs.LEAF, vs.EPS, vs.MIN_POINTS)
    assert (vmap["n_kept"], vmap["n_small"]) == (4095, 1)
    return dict(tgt=frozen(tgt), src=src, src_normals=nrm, T=L["T"], vmap=vmap)


FULL_VOXEL, N_FULL = (8, 0, 0), 20000


@functools.lru_cache(maxsize=None)
def full():
    """voxels_scenes.planted() and 20 000 points in voxel (8, 0, 0) beside it, shuffled into the map: one lane sums them left to right.
    The source: planted()'s and 300 points inside the full voxel"""
    rng = np.random.default_rng(79)
    P = vs.planted()
    tgt = np.concatenate([P["tgt"], vs._in_voxel(rng, FULL_VOXEL, N_FULL, 0.02, 0.98)])
    tgt = tgt[rng.permutation(len(tgt))]
    src = np.concatenate([P["src"], vs._in_voxel(rng, FULL_VOXEL, 300, 0.0, 1.0)])
    nrm = np.concatenate([P["src_normals"], sc.unit_normals(300, 94)])
    vmap = vr.voxel_map(tgt, vs.LEAF, vs.EPS, vs.MIN_POINTS)
    assert int(vmap["count"].max()) == N_FULL and len(tgt) == N_FULL + len(P["tgt"])
    return dict(tgt=frozen(tgt), src=frozen(src), src_normals=frozen(nrm), T=frozen(sc.offset(np.eye(4), 0.01, -0.02, 0.005, 0.002)), vmap=vmap)


TABLES = {"single": single, "lattice_plus": lattice_plus, "lattice_minus": lattice_minus, "full": full}

# ---- 4. far from the origin
FAR_SHIFT = np.array([100000.0, -60000.0, 35.0])


@functools.lru_cache(maxsize=None)
def far_lot():
    """voxels_scenes.lot() with the map shifted by FAR_SHIFT in double and rounded to float32 (the points sit on a 4 to 8 mm lattice
    there), GT / INIT / MID with the same shift in their translation; the frame and its normals are the lot's"""
    L = dict(vs.lot())
    tgt = (L["tgt"].astype(np.float64) + FAR_SHIFT).astype(np.float32)
    for k in ("GT", "INIT", "MID"):
        T = np.array(L[k], np.float64)
        T[:3, 3] += FAR_SHIFT
        L[k] = frozen(T)
    L["tgt"] = frozen(tgt)
    L["vmap"] = vr.voxel_map(tgt, vs.LEAF, vs.EPS, vs.MIN_POINTS)
    for k in ("n5", "nb", "cur5", "curb"):                             # (the map's normals belong to the unshifted points)
        del L[k]
    return L
