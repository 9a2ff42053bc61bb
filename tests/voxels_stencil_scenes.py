"""Scenes of the neighbour-voxel tests (tests/test_voxels_stencil_reference.py, test_emul_vlin_stencil.py, test_gpu_voxels_stencil.py): the
planted map of tests/voxels_scenes.py with three more source points whose over-long normals make some of their correspondences not
positive definite in mode 1, and the bitwise comparison of a dump with its axis of S correspondences.  tests/test_voxels_stencil_reference.py
asserts, on the reference alone, what the scene holds.  Everything is computed once per process and never modified."""
import functools

import numpy as np

import voxels_scenes as vs

frozen = vs.frozen
LONG = float(np.sqrt(1.5))         # a normal of this length: S = C' + (I - c*1.5 u u^T) is positive definite only where C' is wide along u


@functools.lru_cache(maxsize=None)
def planted7():
    """voxels_scenes.planted() - 15 source points; every kept voxel at an edge of the map's voxel box (x -1..6, y 0..2, z -1..0) holds
    one - and three points in voxel (0,0,0), whose kept neighbours are (1,0,0), (-1,0,0) and (0,0,-1), with normals of length sqrt(1.5)
    along x, y and z: 18 source points, one wave"""
    P = vs.planted()
    extra = np.array([[0.6, 0.4, 0.5], [0.3, 0.6, 0.4], [0.5, 0.5, 0.3]], np.float32)
    nrm = np.array([[LONG, 0.0, 0.0], [0.0, LONG, 0.0], [0.0, 0.0, LONG]], np.float32)
    return dict(tgt=P["tgt"], src=frozen(np.concatenate([P["src"], extra])), src_normals=frozen(np.concatenate([P["src_normals"], nrm])),
                T=P["T"], vmap=P["vmap"])


SCENES = {"lot": vs.lot, "planted7": planted7, "lattice": vs.lattice}


def pose_of(S):
    return S["T"] if "T" in S else S["INIT"]


def normals_of(S):
    return S["src_normals"] if "src_normals" in S else S["mb"]


def assert_dump_bitwise(got, want, what="", keys=vs.DUMP_KEYS):
    """voxels_scenes.assert_dump_bitwise over the S axis: shapes, dtypes and every byte"""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
    vs.assert_dump_bitwise(got, want, what, keys)
