"""The keyframe store's rules (include/dcreg.h, "keyframe store") literally in numpy: the yardstick of tests/test_gpu_keyframes.py.

A store is a list of [n, 3] float32 arrays.  A submap is an ordered list of (keyframe id, T 4x4) members; its point sequence is member after
member, each member's stored points in stored order moved by q_a = (float)(R[a][0] p_x + R[a][1] p_y + R[a][2] p_z + t[a]) - evaluated in
double, left to right, every product and sum rounded (`transform` of tests/test_gpu_map_update.py states it).  Without a leaf the output is that
sequence; with one it is `voxel_ref` (tests/test_gpu_voxel.py) of each submap's sequence on its own."""
import numpy as np

from test_gpu_map_update import transform
from test_gpu_voxel import voxel_ref

EMPTY = np.zeros((0, 3), np.float32)


def moved(cloud, T):
    """the stored points of one member at its pose; a coordinate that overflows float becomes inf, as the float store of the device does"""
    with np.errstate(over="ignore", invalid="ignore"):
        return transform(np.asarray(cloud, np.float32).reshape(-1, 3), T)


def submap_sequence(store, members):
    """the raw form of one submap: [m, 3] float32"""
    parts = [moved(store[i], T) for i, T in members]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else EMPTY.copy()


def submaps_ref(store, members, leaf=None, mode="centroid", min_points=1):
    """members = a list (one per submap) of lists of (id, T) -> (a list of [m, 3] float32 arrays, the dcreg_voxel_info counts)"""
    seqs = [submap_sequence(store, sub) for sub in members]
    n_in = sum(len(s) for s in seqs)
    if leaf is None:
        return seqs, {"n_in": n_in, "n_finite": n_in, "n_voxels": 0, "n_out": n_in}
    outs = [voxel_ref(s, leaf, mode, min_points) for s in seqs]
    return outs, {"n_in": n_in, "n_finite": sum(int(np.all(np.isfinite(s), 1).sum()) for s in seqs),
                  "n_voxels": sum(len(voxel_ref(s, leaf, "first", 1)) for s in seqs), "n_out": sum(len(o) for o in outs)}
