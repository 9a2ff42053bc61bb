"""Scenes of the fourth engine's tests (tests/test_voxels_reference.py, test_emul_vlin.py, test_gpu_voxels*.py): the parking lot of the
second engine's tests with its reference voxel map, a planted map with one voxel of every kind, a lattice of 4 096 voxels for the lookup
table, and the bitwise comparison of a dump with the reference's.  Everything is computed once per process and never modified."""
import functools

import numpy as np

import normal_icp_scenes as sc
import voxels_ref as vr

LEAF, EPS, MIN_POINTS = 1.0, 1e-3, 6
GICP_EPS = 1e-3
DUMP_KEYS = ("voxel_idx", "flag", "mean", "cov", "normal_src", "w", "r", "row")
frozen = sc.frozen


def box_of(xyz, leaf=LEAF):
    """(minimum voxel, maximum voxel) of a map's points, int64"""
    v = vr.voxel_of(xyz, leaf).astype(np.int64)
    return v.min(axis=0), v.max(axis=0)


@functools.lru_cache(maxsize=None)
def lot():
    """normal_icp_scenes.lot() with its voxel map at leaf 1.0: 668 occupied voxels, 383 kept; 395 of the 523 source points fall into a kept
    voxel at GT and 365 at INIT.  m5: source normals (k = 5; every point has one), mb: bounded at 0.5 (some have none)"""
    import normals_ref as nr
    L = dict(sc.lot())
    L["vmap"] = vr.voxel_map(L["tgt"], LEAF, EPS, MIN_POINTS)
    a, b = nr.normals_reference(L["src"], k=5), nr.normals_reference(L["src"], k=5, search_radius=sc.RADIUS)
    L["m5"], L["mb"] = frozen(a["normals"]), frozen(b["normals"])
    assert (L["vmap"]["n_voxels"], L["vmap"]["n_kept"]) == (668, 383)
    return L


def _in_voxel(rng, v, n, lo=0.1, hi=0.9):
    return (np.asarray(v, np.float64) + rng.uniform(lo, hi, (n, 3))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted():
    """-> dict tgt, src, src_normals, T (identity), flags0 / flags1 (the flags in mode 0 / 1).  The map, leaf 1.0, min_points 6:
    voxel (0,0,0) 8 points and (-0.0, .3, .3); (0,2,0) exactly 6; (2,0,0) 5 (small); (4,0,0) 6 coincident (degenerate); (6,0,0) 7 collinear
    (two clamped eigenvalues); (-1,0,0) 6 points down to x = -1e-6; (1,0,0) 6 points, one exactly on the face x = 1; (0,0,-1) 6 points."""
    rng = np.random.default_rng(2024)
    line = np.array([6.1, 0.1, 0.5]) + np.linspace(0.0, 0.7, 7)[:, None] * np.array([1.0, 1.0, 0.0])
    neg = _in_voxel(rng, (-1, 0, 0), 6)
    neg[0, 0] = -1e-6
    face = _in_voxel(rng, (1, 0, 0), 6)
    face[0] = (1.0, 0.5, 0.5)
    parts = [_in_voxel(rng, (0, 0, 0), 8), np.array([[-0.0, 0.3, 0.3]], np.float32), _in_voxel(rng, (0, 2, 0), 6), _in_voxel(rng, (2, 0, 0), 5),
             np.tile(np.array([[4.5, 0.5, 0.5]], np.float32), (6, 1)), line.astype(np.float32), neg, face, _in_voxel(rng, (0, 0, -1), 6)]
    tgt = np.concatenate(parts).astype(np.float32)
    tgt = tgt[rng.permutation(len(tgt))]                  # (a voxel's points are not contiguous in the map)
    src = np.array([[0.5, 0.5, 0.5],      # kept voxel
                    [0.4, 2.6, 0.2],      # the voxel with exactly min_points
                    [2.5, 0.5, 0.5],      # small voxel: none
                    [4.5, 0.5, 0.5],      # degenerate voxel: none
                    [6.3, 0.4, 0.5],      # the collinear voxel
                    [-0.5, 0.5, 0.5],     # negative side of 0
                    [-0.0, 0.5, 0.5],     # -0.0 is voxel 0
                    [1.0, 0.2, 0.7],      # exactly on the face: voxel 1
                    [0.99999994, 0.2, 0.7],   # the float below 1: voxel 0
                    [3.5, 0.5, 0.5],      # inside the box, an empty voxel
                    [50.0, 50.0, 50.0],   # outside the box
                    [-30.0, 0.5, 0.5],    # outside the box
                    [0.5, 0.5, -0.5],     # negative z
                    [0.2, 0.8, 0.4],      # mode 1: a source normal with a NaN
                    [0.7, 0.3, 0.6]],     # mode 1: a source normal of length 2
                   np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(src), 1))
    nrm[1] = (0.6, 0.0, 0.8)
    nrm[13] = (np.nan, 0.0, 1.0)
    nrm[14] = (0.0, 2.0, 0.0)
    flags0 = [1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    flags1 = flags0[:13] + [3, 5]
    return dict(tgt=frozen(tgt), src=frozen(src), src_normals=frozen(nrm), T=frozen(np.eye(4)), flags0=flags0, flags1=flags1,
                vmap=vr.voxel_map(tgt, LEAF, EPS, MIN_POINTS))


@functools.lru_cache(maxsize=None)
def lattice():
    """16^3 = 4 096 voxels of 6 points each (24 576 points, shuffled) and 1 000 source points in and around them: the lookup table sees
    collisions and probe sequences"""
    rng = np.random.default_rng(77)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 3)
    tgt = (np.repeat(g, 6, axis=0) + rng.uniform(0.05, 0.95, (len(g) * 6, 3))).astype(np.float32)
    tgt = tgt[rng.permutation(len(tgt))]
    src = rng.uniform(-1.0, 17.0, (1000, 3)).astype(np.float32)
    vmap = vr.voxel_map(tgt, LEAF, EPS, MIN_POINTS)
    assert vmap["n_kept"] == 4096
    return dict(tgt=frozen(tgt), src=frozen(src), src_normals=sc.unit_normals(1000, 91), T=frozen(sc.offset(np.eye(4), 0.03, -0.02, 0.01, 0.01)),
                vmap=vmap)


MAPS = {"lot": lot, "planted": planted, "lattice": lattice}


def assert_map_bitwise(got, want, what=""):
    for k, dt in (("coords", np.int64), ("count", np.int32), ("mean", np.float32), ("cov", np.float32)):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == dt and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


def assert_dump_bitwise(got, want, what="", keys=DUMP_KEYS):
    for k in keys:
        assert sc.same_bits(np.asarray(got[k]), np.asarray(want[k])), (what, k)
