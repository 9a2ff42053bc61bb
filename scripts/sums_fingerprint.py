"""A fingerprint of what the second, third and fourth engine's linearisations return, to compare two builds of the library on one device:
one line per case with a hash of the raw bytes of the returned sums (H_upper, g, sum_r2, sum_b2, n_eff, n_pt of every pose) and, for the
debug forms, of every dump array.  Two builds compute the same if and only if their outputs are the same text (diff them).

The cases sit at the edges the kernel bodies care about - sources of 1, 63, 64, 65, 255, 256, 257 and 513 points: the wave and block
boundaries, a last block with one live lane, more than one block.
  voxels   single pose and debug, frames (one launch over all sizes: the blocks past a short frame's end exit early; and the own source)
           and pairs (among them poses whose target keeps no voxel: the zero row), in both "voxels_source_cov" modes, "robust_kernel"
           off and on
  normals, gicp   single pose, debug and frames, "robust_kernel" off and on
Every case runs once: this is a comparison, not a stress loop.

usage: [DCREG_LIB=<another build of the library>] python scripts/sums_fingerprint.py > fingerprint.txt"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api  # noqa: E402

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
RADIUS = 1.0
SUM_KEYS = ("H_upper", "g", "sum_r2", "sum_b2", "n_eff", "n_pt")
NORMALS_5 = api.normal_params(k=5)
VOXEL_MAP = api.voxel_map_params(1.0, 1.0e-3, 6)


def scene():
    rng = np.random.default_rng(11)
    xy = rng.random((6000, 2)) * 8.0
    z = 0.3 * np.sin(xy[:, 0]) + 0.2 * np.cos(1.7 * xy[:, 1]) + rng.normal(0.0, 0.02, 6000)
    tgt = np.column_stack([xy, z]).astype(np.float32)
    srcs = [(tgt[rng.choice(6000, n, replace=False)] + rng.normal(0.0, 0.02, (n, 3))).astype(np.float32) for n in SIZES]
    few = tgt[:5].copy()                       # a pair target that keeps no voxel
    return tgt, srcs, few


def pose(k):
    a = 0.01 * (k + 1)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.05 - 0.01 * k, 0.02 * k, 0.03]
    return T


def digest(outs, dump_keys=False):
    h = hashlib.sha256()
    for o in outs if isinstance(outs, list) else [outs]:
        for k in SUM_KEYS if not dump_keys else sorted(o):
            h.update(np.ascontiguousarray(o[k]).tobytes())
    return h.hexdigest()[:32]


def line(name, outs, dump=False):
    first = outs[0] if isinstance(outs, list) else outs
    print("%-44s %s%s  n_eff %d" % (name, digest(outs), (" dump " + digest(outs, True)) if dump else "", first["n_eff"]), flush=True)


def main():
    tgt, srcs, few = scene()
    prm = api.default_lin_params(RADIUS, 1)
    Ts = [pose(k) for k in range(len(SIZES))]
    for robust in (0, 1):
        c = api.Context(0)
        try:
            c.set_option("robust_kernel", robust)
            c.set_target(tgt, RADIUS)
            c.keep_target_normals(NORMALS_5)
            c.keep_target_voxels(VOXEL_MAP)
            c.frames_load(srcs)
            c.frames_normals_keep(NORMALS_5)
            c.pairs_sources_load(srcs)
            c.pairs_sources_normals_keep(NORMALS_5)
            c.pairs_voxels_build([tgt, few, tgt[:3000]], VOXEL_MAP)
            tag = "robust%d" % robust
            # ---- the single pose, plain and debug, every engine
            for n, s, T in zip(SIZES, srcs, Ts):
                c.set_source(s)
                c.keep_source_normals(NORMALS_5)
                for name, lin in (("normals", c.linearize_normals), ("gicp", c.linearize_gicp)):
                    line("%s %s single n=%d" % (tag, name, n), lin(T, prm))
                    line("%s %s debug n=%d" % (tag, name, n), lin(T, prm, debug=True), dump=True)
                for mode in (0, 1):
                    c.set_option("voxels_source_cov", mode)
                    line("%s voxels mode%d single n=%d" % (tag, mode, n), c.linearize_voxels(T, prm))
                    line("%s voxels mode%d debug n=%d" % (tag, mode, n), c.linearize_voxels(T, prm, debug=True), dump=True)
            # ---- frames: one launch over all sizes (the blocks of the largest frame: the short frames' later blocks exit early), and
            # the own source (the last one set: 513 points)
            fids = list(range(len(SIZES)))
            for name, batch in (("normals", c.normals_batch), ("gicp", c.gicp_batch)):
                line("%s %s frames" % (tag, name), batch(Ts, None, fids, prm))
                line("%s %s own source" % (tag, name), batch(Ts[:3], None, None, prm, slot=1))
            tids = [0, 1, 2, 0, 1, 2, 0, 2]     # target 1 has no member
            for mode in (0, 1):
                c.set_option("voxels_source_cov", mode)
                line("%s voxels mode%d frames" % (tag, mode), c.voxels_batch(Ts, fids, prm))
                line("%s voxels mode%d own source" % (tag, mode), c.voxels_batch(Ts[:3], None, prm, slot=1))
                got = c.pairs_voxels_batch(Ts, fids, tids, prm)
                assert all(g["n_pt"] == 0 and not np.any(g["H_upper"]) for g, t in zip(got, tids) if t == 1)
                line("%s voxels mode%d pairs" % (tag, mode), got)
                line("%s voxels mode%d pairs reversed" % (tag, mode), c.pairs_voxels_batch(Ts[::-1], fids[::-1], tids, prm, slot=1))
        finally:
            c.close()


if __name__ == "__main__":
    main()
