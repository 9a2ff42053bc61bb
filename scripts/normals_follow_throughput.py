"""Kept normals through a keyframe loop: the mapping front-end on the second engine (dcreg_set_source + dcreg_icp_run_normals +
dcreg_target_insert_source of the result, and every --crop-every keyframes dcreg_target_crop to a box around the vehicle) with
"normals_follow" on, beside the same loop with the option off that calls dcreg_target_normals_keep after every update - in one process,
on one device.  Maps of 1 M, 10 M and 50 M points (scenes.scene_prior_map, extent scaled to keep its density), 8 k-point frames along a
path through it (scenes.drive).  A host clock around calls that end in a synchronise; keyframe 0 of each loop is a warm-up.  Checks that
both loops register every keyframe to bitwise the same pose and end with bitwise the same normals.  Per map: ms per keyframe of both
loops, the median ms of an insert and a crop with and without following, of a full keep, and n_refit of every keyframe.
--share-probe: on the first map, inserts of growing clouds with the fallback threshold out of the way ("normals_follow_full_share" 1):
the dirty share, the cost of following incrementally (followed insert minus plain insert) and the cost of the full keep it competes with
- the numbers behind the default threshold.  Prints one JSON line.

usage: python scripts/normals_follow_throughput.py [--maps 1000000,10000000,50000000] [--keyframes 20] [--points 8000] [--crop-every 10]"""
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


def loop(world, poses, frames, cfg, p, half, args, follow):
    """-> dict of times, the registered poses, the final normals"""
    ctx = api.Context(0)
    ins, crops, keeps, refit, Ts, t_loop = [], [], [], [], [], 0.0
    try:
        ctx.set_option("normals_follow", 1 if follow else 0)
        ctx.set_target(world, RADIUS)
        _, keep0 = clock(lambda: ctx.keep_target_normals(p))
        for k, (T, f) in enumerate(zip(poses, frames)):
            t0 = time.perf_counter()
            ctx.set_source(f)
            res, _ = ctx.icp_run_normals(T @ OFFSET, "Ours", cfg)
            Tr = pose_of(res)
            _, i_ms = clock(lambda: ctx.insert_source(Tr))
            k_ms = 0.0 if follow else clock(lambda: ctx.keep_target_normals(p))[1]
            if follow:
                refit.append(ctx.normals_follow_info())
            c_ms = None
            if args.crop_every and k % args.crop_every == args.crop_every - 1:
                lo, hi = crop_box(T, half)
                _, c_ms = clock(lambda: ctx.crop(lo, hi))
                if follow:
                    refit.append(ctx.normals_follow_info())
                else:
                    k_ms += clock(lambda: ctx.keep_target_normals(p))[1]
            Ts.append(Tr)
            if k > 0:            # (keyframe 0: warm-up)
                t_loop += time.perf_counter() - t0
                ins.append(i_ms)
                if not follow:
                    keeps.append(k_ms)
                if c_ms is not None:
                    crops.append(c_ms)
        assert ctx.target_normals_kept() == 1
        out = {"ms_per_keyframe": t_loop * 1e3 / args.keyframes, "insert_ms": float(np.median(ins)),
               "crop_ms": float(np.median(crops)) if crops else None, "first_keep_ms": keep0, "final_map_points": ctx.index_info().n_target}
        if follow:
            out["updates"] = [{"n_refit": r["n_refit"], "followed": r["followed"]} for r in refit]
        else:
            out["keep_ms_per_keyframe"] = float(np.median(keeps))
        return out, Ts, ctx.kept_target_normals()
    finally:
        ctx.close()


def run(n_map, args):
    extent = 350.0 * np.sqrt(n_map / 50e6)
    world, _ = scenes.scene_prior_map(n_map, extent=extent)
    poses, frames = scenes.drive(world, args.keyframes + 1, step=1.5, n_frame=args.points, seed=1,
                                 start=(world[:, 0].mean(), world[:, 1].mean()))
    cfg = api.default_config(search_radius=RADIUS, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1)
    p = api.normal_params(k=args.k)
    half = 0.8 * extent
    a, Ta, na = loop(world, poses, frames, cfg, p, half, args, True)
    b, Tb, nb = loop(world, poses, frames, cfg, p, half, args, False)
    same = all(np.array_equal(x, y) for x, y in zip(Ta, Tb)) and all(
        x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and x[~np.isnan(x)].tobytes() == y[~np.isnan(y)].tobytes() for x, y in zip(na, nb))
    return {"map_points": n_map, "followed": a, "rekeep": b, "same_poses_and_normals": bool(same),
            "speedup_per_keyframe": b["ms_per_keyframe"] / a["ms_per_keyframe"]}


def share_probe(n_map, args):
    """inserts of growing clouds spread over the whole map: dirty share, cost of the incremental refit, cost of the full keep"""
    extent = 350.0 * np.sqrt(n_map / 50e6)
    world, _ = scenes.scene_prior_map(n_map, extent=extent)
    p = api.normal_params(k=args.k)
    rng = np.random.default_rng(5)
    out = []
    for frac in (0.002, 0.01, 0.03, 0.06, 0.12, 0.25):
        m = int(frac * n_map)
        cloud = (world[rng.choice(n_map, m, replace=False)].astype(np.float64) + rng.normal(0.0, 0.02, (m, 3))).astype(np.float32)
        row = {"n_inserted": m}
        for name, follow in (("plain", 0), ("followed", 1)):
            ctx = api.Context(0)
            try:
                ctx.set_option("normals_follow", follow)
                ctx.set_option("normals_follow_full_share", 1.0)
                ctx.set_target(world, RADIUS)
                ctx.keep_target_normals(p)
                _, row[name + "_insert_ms"] = clock(lambda: ctx.insert(cloud, np.eye(4)))
                if follow:
                    info = ctx.normals_follow_info()
                    row["dirty_share"] = info["n_refit"] / info["n_target"]
                    row["mode"] = info["followed"]
                else:
                    _, row["keep_ms"] = clock(lambda: ctx.keep_target_normals(p))
            finally:
                ctx.close()
        row["follow_ms"] = row["followed_insert_ms"] - row["plain_insert_ms"]
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="1000000,10000000,50000000")
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--crop-every", type=int, default=10)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--share-probe", type=int, default=1, help="1: the dirty-share sweep on the first map (the fallback threshold's numbers)")
    args = ap.parse_args()
    maps = [int(n) for n in args.maps.split(",")]
    res = {"normals_follow_throughput": [run(n, args) for n in maps]}
    if args.share_probe:
        res["share_probe"] = {"map_points": maps[0], "rows": share_probe(maps[0], args)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
