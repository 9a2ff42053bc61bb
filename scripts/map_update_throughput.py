"""A growing map: the keyframe loop of a mapping front-end (dcreg_set_source + dcreg_icp_run + dcreg_target_insert_source of the result,
and every --crop-every keyframes dcreg_target_crop to a box around the vehicle) against the same loop that keeps the map on the host and
calls dcreg_set_target with the accumulated map at every keyframe.  Maps of 1 M, 10 M and 50 M points (scenes.scene_prior_map, extent
scaled to keep its density), 8 k-point frames along a path through it (scenes.drive).  A host clock around calls that end in a
synchronise; one warm-up keyframe of each loop first.  Checks that both loops register every keyframe to bitwise the same pose.  Per map:
per-call ms of insert and crop (median), how many calls re-derived the grid, ms per keyframe of both loops, and (--rebuild-probe) one insert
that re-derives the grid: its time, and cell edge, dims, whole_map_capped and ms per registration before and after.  Prints one JSON line.

usage: python scripts/map_update_throughput.py [--maps 1000000,10000000,50000000] [--keyframes 20] [--points 8000] [--crop-every 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402

RADIUS = 0.5


def transform(xyz, T):
    p = xyz.astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    return np.stack([R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1] + R[a, 2] * p[:, 2] + t[a] for a in range(3)], 1).astype(np.float32)


def pose_of(res):
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    return T


def crop_box(T, half):
    c = T[:3, 3]
    return [c[0] - half, c[1] - half, -1e9], [c[0] + half, c[1] + half, 1e9]


def grid_of(ctx):
    i = ctx.index_info()
    return {"cell": i.cell, "dims": list(i.dims[:]), "whole_map_capped": ctx.roi_info()["whole_map_capped"]}


def reg_ms(ctx, f, T, cfg, repeats=5):
    ctx.set_source(f)
    T0 = T @ scenes.pose6d_matrix(0.05, -0.04, 0.02, 0.0, 0.0, 0.005)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ctx.icp_run(T0, "Ours", cfg)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def rebuild_probe(ctx, f, T, cfg):
    """one re-derivation of the grid: a frame inserted 40 m beyond the map's box in x; the grid and the registration time before and after"""
    before = dict(grid_of(ctx), ms_per_registration=reg_ms(ctx, f, T, cfg))
    i = ctx.index_info()
    Ts = T.copy()
    Ts[0, 3] = i.origin[0] + i.dims[0] * i.cell + 40.0
    t0 = time.perf_counter()
    info = ctx.insert(f, Ts)
    ms = (time.perf_counter() - t0) * 1e3
    after = dict(grid_of(ctx), ms_per_registration=reg_ms(ctx, f, T, cfg))
    return {"rebuilt": info["rebuilt"], "insert_ms": ms, "before": before, "after": after}


def run(n_map, args):
    extent = 350.0 * np.sqrt(n_map / 50e6)
    world, _ = scenes.scene_prior_map(n_map, extent=extent)
    poses, frames = scenes.drive(world, args.keyframes + 1, step=1.5, n_frame=args.points, seed=1,
                                 start=(world[:, 0].mean(), world[:, 1].mean()))
    cfg = api.default_config(search_radius=RADIUS, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1)
    half = 0.8 * extent
    out = {"map_points": n_map}
    # ---- the map updated on the device
    ctx = api.Context(0)
    ins_ms, crop_ms, rebuilt, poses_upd = [], [], 0, []
    try:
        ctx.set_target(world, RADIUS)
        t_loop = 0.0
        for k, (T, f) in enumerate(zip(poses, frames)):
            t0 = time.perf_counter()
            ctx.set_source(f)
            res, _ = ctx.icp_run(T @ scenes.pose6d_matrix(0.05, -0.04, 0.02, 0.0, 0.0, 0.005), "Ours", cfg)
            Tr = pose_of(res)
            t1 = time.perf_counter()
            info = ctx.insert_source(Tr)
            t2 = time.perf_counter()
            c_ms = None
            if args.crop_every and k % args.crop_every == args.crop_every - 1:
                lo, hi = crop_box(T, half)
                ci = ctx.crop(lo, hi)
                c_ms = (time.perf_counter() - t2) * 1e3
                rebuilt += ci["rebuilt"] if k > 0 else 0
            t3 = time.perf_counter()
            poses_upd.append(Tr)
            if k > 0:            # (keyframe 0: warm-up)
                t_loop += t3 - t0
                ins_ms.append((t2 - t1) * 1e3)
                rebuilt += info["rebuilt"]
                if c_ms is not None:
                    crop_ms.append(c_ms)
        out["insert_ms"] = float(np.median(ins_ms))
        out["crop_ms"] = float(np.median(crop_ms)) if crop_ms else None
        out["rebuilt_calls"] = rebuilt
        out["update_calls"] = len(ins_ms) + len(crop_ms)
        out["ms_per_keyframe_update"] = t_loop * 1e3 / args.keyframes
        out["final_map_points"] = ctx.index_info().n_target
        if args.rebuild_probe:
            out["rebuild_probe"] = rebuild_probe(ctx, frames[-1], poses[-1], cfg)
    finally:
        ctx.close()
    # ---- the map kept on the host, set_target at every keyframe
    ctx = api.Context(0)
    same = True
    try:
        m = world
        ctx.set_target(m, RADIUS)
        t_loop, st_ms = 0.0, []
        for k, (T, f) in enumerate(zip(poses, frames)):
            t0 = time.perf_counter()
            ctx.set_source(f)
            res, _ = ctx.icp_run(T @ scenes.pose6d_matrix(0.05, -0.04, 0.02, 0.0, 0.0, 0.005), "Ours", cfg)
            Tr = pose_of(res)
            same = same and np.array_equal(Tr, poses_upd[k])
            m = np.concatenate([m, transform(f, Tr)])
            if args.crop_every and k % args.crop_every == args.crop_every - 1:
                lo, hi = crop_box(T, half)
                p = m.astype(np.float64)
                m = m[np.all((p >= lo) & (p <= hi), 1)]
            t1 = time.perf_counter()
            ctx.set_target(m, RADIUS)
            t2 = time.perf_counter()
            if k > 0:
                t_loop += t2 - t0
                st_ms.append((t2 - t1) * 1e3)
        out["set_target_ms"] = float(np.median(st_ms))
        out["ms_per_keyframe_set_target"] = t_loop * 1e3 / args.keyframes
    finally:
        ctx.close()
    out["same_poses"] = bool(same)
    out["speedup_per_keyframe"] = out["ms_per_keyframe_set_target"] / out["ms_per_keyframe_update"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="1000000,10000000,50000000")
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--crop-every", type=int, default=10)
    ap.add_argument("--rebuild-probe", type=int, default=1, help="1: after the loop, one insert that re-derives the grid (grid and ms per registration before and after)")
    args = ap.parse_args()
    res = [run(int(n), args) for n in args.maps.split(",")]
    print(json.dumps({"map_update_throughput": res}))


if __name__ == "__main__":
    main()
