"""The kept voxel map through a keyframe loop: the mapping front-end on the fourth engine (dcreg_set_source + dcreg_icp_run_voxels +
dcreg_target_insert_source of the result, and every --crop-every keyframes dcreg_target_crop to a box around the vehicle) with
"voxels_follow" on (leg a), beside the same loop with the option off that calls dcreg_target_voxels_keep after every update (leg b: the
only way without the option, and the yardstick) - two contexts in one process on one device, the legs alternating keyframe by keyframe
(the leg that goes first alternates too).  Maps of 1 M, 10 M and 50 M points (scenes.scene_prior_map, extent scaled to keep its
density), 8 k-point frames along a path through it (scenes.drive), leaf 1.0 and 0.5.  A host clock around calls that end in a
synchronise; keyframe 0 is a warm-up.  Checks that both legs register every keyframe to bitwise the same pose and end with bitwise the
same voxel map.  Per map and leaf: ms per keyframe of both legs, the cost of one followed insert and one followed crop against the plain
update plus the keep - medians with minimum and maximum - and n_touched / n_refit / n_carried of every followed update.  Prints one JSON
line.

usage: python scripts/voxels_follow_throughput.py [--maps 1000000,10000000,50000000] [--leaves 1.0,0.5] [--keyframes 10] [--points 8000]
                                                  [--crop-every 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402

RADIUS = 0.5
OFFSET = scenes.pose6d_matrix(0.05, -0.04, 0.02, 0.0, 0.0, 0.005)


def pose_of(res):
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    return T


def crop_box(T, half):
    c = T[:3, 3]
    return [c[0] - half, c[1] - half, -1e9], [c[0] + half, c[1] + half, 1e9]


def clock(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def spread(xs):
    return None if not xs else {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


class Leg:
    def __init__(self, world, params, follow):
        self.follow, self.params = follow, params
        self.ctx = api.Context(0)
        self.ctx.set_option("voxels_follow", 1 if follow else 0)
        self.ctx.set_target(world, RADIUS)
        _, self.first_keep_ms = clock(lambda: self.ctx.keep_target_voxels(params))
        self.frame_ms, self.insert_ms, self.crop_ms, self.keep_ms, self.updates, self.poses = [], [], [], [], [], []

    def update(self, call, times, warm):
        """one update of the map and what keeps the voxel map beside it: the follow inside the call, or the keep behind it"""
        _, ms = clock(call)
        if self.follow:
            info = self.ctx.voxels_follow_info()
            assert info["followed"] in (1, 2), info
            self.updates.append({k: info[k] for k in ("n_touched", "n_refit", "n_carried", "n_kept", "followed")})
        else:
            _, k_ms = clock(lambda: self.ctx.keep_target_voxels(self.params))
            ms += k_ms
            if not warm:
                self.keep_ms.append(k_ms)
        if not warm:
            times.append(ms)

    def keyframe(self, k, T, frame, cfg, crop_every, half):
        t0 = time.perf_counter()
        self.ctx.set_source(frame)
        res, _ = self.ctx.icp_run_voxels(T @ OFFSET, "Ours", cfg)
        Tr = pose_of(res)
        self.update(lambda: self.ctx.insert_source(Tr), self.insert_ms, k == 0)
        if crop_every and k % crop_every == crop_every - 1:
            lo, hi = crop_box(T, half)
            self.update(lambda: self.ctx.crop(lo, hi), self.crop_ms, k == 0)
        self.poses.append(Tr)
        if k > 0:                  # (keyframe 0: warm-up)
            self.frame_ms.append((time.perf_counter() - t0) * 1e3)

    def report(self):
        out = {"ms_per_keyframe": spread(self.frame_ms), "insert_ms": spread(self.insert_ms), "crop_ms": spread(self.crop_ms),
               "first_keep_ms": self.first_keep_ms, "final_map_points": self.ctx.index_info().n_target, "kept_voxels": self.ctx.target_voxels_kept()}
        if self.follow:
            out["updates"] = self.updates
        else:
            out["keep_ms"] = spread(self.keep_ms)
        return out


def run(world, n_map, extent, leaf, args):
    poses, frames = scenes.drive(world, args.keyframes + 1, step=1.5, n_frame=args.points, seed=1, start=(world[:, 0].mean(), world[:, 1].mean()))
    cfg = api.default_config(search_radius=RADIUS, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1)
    params = api.voxel_map_params(leaf, 1e-3, 6)
    half = 0.8 * extent
    a, b = Leg(world, params, True), Leg(world, params, False)
    try:
        for k, (T, f) in enumerate(zip(poses, frames)):
            for leg in ((a, b) if k % 2 == 0 else (b, a)):
                leg.keyframe(k, T, f, cfg, args.crop_every, half)
        va, vb = a.ctx.kept_target_voxels(), b.ctx.kept_target_voxels()
        same = all(np.array_equal(x, y) for x, y in zip(a.poses, b.poses)) and all(va[k].tobytes() == vb[k].tobytes() for k in va)
        ra, rb = a.report(), b.report()
    finally:
        a.ctx.close()
        b.ctx.close()
    return {"map_points": n_map, "leaf": leaf, "followed": ra, "rekeep": rb, "same_poses_and_voxels": bool(same),
            "speedup_per_keyframe": rb["ms_per_keyframe"]["median"] / ra["ms_per_keyframe"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="1000000,10000000,50000000")
    ap.add_argument("--leaves", default="1.0,0.5")
    ap.add_argument("--keyframes", type=int, default=10)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--crop-every", type=int, default=5)
    args = ap.parse_args()
    rows = []
    for n_map in (int(n) for n in args.maps.split(",")):
        extent = 350.0 * np.sqrt(n_map / 50e6)
        world, _ = scenes.scene_prior_map(n_map, extent=extent)
        for leaf in (float(x) for x in args.leaves.split(",")):
            rows.append(run(world, n_map, extent, leaf, args))
            print("# %d points, leaf %g: %.2f ms (followed) vs %.2f ms (rekeep) per keyframe" % (
                n_map, leaf, rows[-1]["followed"]["ms_per_keyframe"]["median"], rows[-1]["rekeep"]["ms_per_keyframe"]["median"]), file=sys.stderr, flush=True)
    print(json.dumps({"voxels_follow_throughput": rows}))


if __name__ == "__main__":
    main()
