"""What neighbour-voxel correspondences ("voxels_neighbors" = 7 / 27; include/dcreg.h) cost and what they reach, beside the one-voxel form.
One process, one box; the legs that are compared run ALTERNATING in the same loop, so the yardstick of every figure is the figure beside
it.  A host clock around calls that end in a synchronise, after warm-up.
  lin        the time of one dcreg_linearize_voxels at a settled pose at S = 1 / 7 / 27, in both modes of "voxels_source_cov", on the three
             sizes of scripts/voxels_throughput.py: the 8 k frame against the 200 k parking-lot map (at the pose a GICP run reaches),
             200 k x 200 k and the 1 M x 1 M corridor (the map's own points with 1 cm of noise as the source, at the identity); per leg
             the median over all rounds and the spread of the rounds' medians, and the counts of the call; every other round runs the
             legs in reverse order.  With
             --parent-lib (the libdcreg_hip.so of another build, the parent commit's) one more leg runs that build's call - S = 1, the
             only form it has - in the same loop, on a context of its own
  run        one registration ("Ours", thresholds on, max_iterations 40) of the 8 k frame from PK01_INIT per S and mode: iterations,
             time, final error
  far        the far-start pairs of scripts/pairs_voxels_throughput.py (submap pairs started 1 to 2 m and up to 3 degrees per axis off)
             through dcreg_register_pairs_voxels per S, for leaf 1.0 and 0.5 and both modes, without a robust kernel and with
             --robust (kernel, scale): converged pairs, mean iterations and final errors
Prints one JSON line.

usage: python scripts/voxels_stencil_throughput.py [--rounds 7] [--calls 10] [--pairs 256] [--skip c3x,c4,far] [--parent-lib PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402
from pairs_voxels_throughput import stage  # noqa: E402
from voxels_throughput import pose_of, timed  # noqa: E402

SIZES = (1, 7, 27)


def other_build(path):
    """-> a function that makes a Context of the library at `path` beside this tree's own (api.load keeps one library per process)"""
    mine = api.load()
    api._lib, api.LIB_PATH = None, path
    theirs = api.load()
    api._lib = mine

    def make():
        api._lib = theirs
        try:
            return api.Context(0)
        finally:
            api._lib = mine
    return make


def lin_leg(ctx, parent, T, prm, rounds, calls):
    out = {}
    for mode in (0, 1):
        legs = {}
        for S in SIZES:
            def leg(S=S):
                ctx.set_option("voxels_neighbors", S)
                return lambda: ctx.linearize_voxels(T, prm)
            legs["S%d" % S] = leg
        if parent is not None:
            legs["parent_S1"] = lambda: (lambda: parent.linearize_voxels(T, prm))
        for c in (ctx, parent):
            if c is not None:
                c.set_option("voxels_source_cov", mode)
        per, counts = {k: [] for k in legs}, {}
        for k, leg in legs.items():                     # warm-up of every code path
            fn = leg()
            for _ in range(3):
                r = fn()
            counts[k] = (r["n_eff"], r["n_pt"])
        for rnd in range(rounds):
            for k in (list(legs) if rnd % 2 == 0 else list(legs)[::-1]):      # (every other round backwards: no leg always follows the same one)
                fn = legs[k]()
                fn()
                per[k].append(timed(fn, calls))
        rec = {k: {"us": 1e3 * float(np.median(v)), "rounds_min_us": 1e3 * float(np.min(v)), "rounds_max_us": 1e3 * float(np.max(v)),
                   "n_eff": counts[k][0], "n_pt": counts[k][1]} for k, v in per.items()}
        for S in SIZES[1:]:
            rec["S%d_over_S1" % S] = rec["S%d" % S]["us"] / rec["S1"]["us"]
        if parent is not None:
            rec["S1_minus_parent_us"] = rec["S1"]["us"] - rec["parent_S1"]["us"]
        out["mode_%d" % mode] = rec
    ctx.set_option("voxels_neighbors", 1)
    ctx.set_option("voxels_source_cov", 0)
    return out


def run_leg(ctx, init, cfg, gt, rounds):
    legs = [(mode, S) for mode in (0, 1) for S in SIZES]
    rec, per = {}, {}

    def run(mode, S):
        ctx.set_option("voxels_source_cov", mode)
        ctx.set_option("voxels_neighbors", S)
        return ctx.icp_run_voxels(init, "Ours", cfg, log_capacity=0)[0]

    for mode, S in legs:
        res = run(mode, S)
        te, re_ = api.pose_error(gt, pose_of(res))
        rec[(mode, S)] = {"mode": mode, "S": S, "iterations": int(res.iterations), "converged": int(res.converged), "status": int(res.status),
                          "trans_err_m": te, "rot_err_deg": re_}
        per[(mode, S)] = []
    for _ in range(rounds):
        for mode, S in legs:
            t0 = time.perf_counter()
            run(mode, S)
            per[(mode, S)].append((time.perf_counter() - t0) * 1e3)
    for k in legs:
        rec[k]["run_ms"] = float(np.median(per[k]))
        rec[k]["ms_per_iteration"] = rec[k]["run_ms"] / max(rec[k]["iterations"], 1)
    ctx.set_option("voxels_neighbors", 1)
    ctx.set_option("voxels_source_cov", 0)
    return [rec[k] for k in legs]


def far_leg(n_pairs, points, submap, robust):
    tgt, _ = scenes.scene_parkinglot()
    rng = np.random.default_rng(5)
    gt = scenes.pose6d_matrix(**scenes.PK01_GT)
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1)
    poses = [gt @ scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-20, 20))) for _ in range(n_pairs)]
    srcs, tgts, Tt = scenes.scan_pairs(tgt, poses, points, seed=3, mode="submap", n_submap=submap, submap_radius=45.0)
    far = []
    for T in Tt:
        d = rng.normal(size=3)
        d *= rng.uniform(1.0, 2.0) / np.linalg.norm(d)
        far.append(T @ scenes.pose6d_matrix(*d, *np.deg2rad(rng.uniform(-3.0, 3.0, 3))))
    sn = api.normal_params(k=5)
    legs = []
    ctx = api.Context(0)
    try:
        for kernel, scale in ((0, 1.0), robust):
            ctx.set_robust(kernel, gicp_scale=scale)
            for leaf in (1.0, 0.5):
                for mode in (0, 1):
                    ctx.set_option("voxels_source_cov", mode)
                    for S in SIZES:
                        ctx.set_option("voxels_neighbors", S)
                        t0 = time.perf_counter()
                        recs = ctx.register_pairs_voxels(srcs, tgts, far, "Ours", cfg, api.voxel_map_params(leaf), sn if mode else None, slots=64)
                        ms = (time.perf_counter() - t0) * 1e3
                        legs.append({"kernel": kernel, "scale": scale, "leaf": leaf, "mode": mode, "S": S, "pairs": n_pairs, "call_ms": ms,
                                     **stage(recs, Tt)})
    finally:
        ctx.close()
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--submap", type=int, default=100_000)
    ap.add_argument("--robust", default="3,1.0")
    ap.add_argument("--skip", default="")
    ap.add_argument("--parent-lib", default="")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    robust = (int(args.robust.split(",")[0]), float(args.robust.split(",")[1]))
    make_parent = other_build(args.parent_lib) if args.parent_lib else None
    out = {"rounds": args.rounds, "calls": args.calls, "parent_lib": bool(args.parent_lib)}
    k5 = api.normal_params(k=5)
    vp = api.voxel_map_params()
    pk_gt, pk_init = scenes.pose6d_matrix(**scenes.PK01_GT), scenes.pose6d_matrix(**scenes.PK01_INIT)

    def context(make, tgt, src, radius):
        ctx = make()
        ctx.set_target(tgt, radius)
        ctx.set_source(src)
        ctx.keep_source_normals(k5)
        ctx.keep_target_voxels(vp)
        return ctx

    def both(tgt, src, radius):
        return context(lambda: api.Context(0), tgt, src, radius), (context(make_parent, tgt, src, radius) if make_parent else None)

    def settled(ctx, init, cfg):
        ctx.keep_target_normals(k5)
        res, _ = ctx.icp_run_gicp(init, "Ours", cfg)
        return pose_of(res)

    def close(*cs):
        for c in cs:
            if c is not None:
                c.close()

    tgt, src = scenes.scene_parkinglot()
    if "c3" not in skip:
        cfg = api.default_config(search_radius=0.5, max_iterations=40, use_weight_derivative=0, gt_matrix=pk_gt.reshape(-1))
        ctx, parent = both(tgt, src, 0.5)
        rec = {"map_points": int(len(tgt)), "frame_points": int(len(src))}
        rec["lin"] = lin_leg(ctx, parent, settled(ctx, pk_init, cfg), api.default_lin_params(0.5, 0), args.rounds, args.calls)
        rec["run"] = run_leg(ctx, pk_init, cfg, pk_gt, max(args.rounds // 2, 3))
        out["c3_pk01_200k_x_8k"] = rec
        close(ctx, parent)
    if "c3x" not in skip:
        dense = (tgt + np.random.default_rng(1000).normal(0, 0.01, tgt.shape)).astype(np.float32)
        ctx, parent = both(tgt, dense, 0.5)
        rec = {"map_points": int(len(tgt)), "frame_points": int(len(dense))}
        rec["lin"] = lin_leg(ctx, parent, np.eye(4), api.default_lin_params(0.5, 0), max(args.rounds // 2, 3), max(args.calls // 2, 5))
        out["c3x_pk01_200k_x_200k"] = rec
        close(ctx, parent)
    if "c4" not in skip:
        big = scenes.scene_corridor(1_000_000, seed=0)
        noisy = (big + np.random.default_rng(1000).normal(0, 0.01, big.shape)).astype(np.float32)
        ctx, parent = both(big, noisy, 1.0)
        rec = {"map_points": int(len(big)), "frame_points": int(len(noisy))}
        rec["lin"] = lin_leg(ctx, parent, np.eye(4), api.default_lin_params(1.0, 1), max(args.rounds // 2, 3), max(args.calls // 2, 5))
        out["c4_corridor_1m"] = rec
        close(ctx, parent)
    if "far" not in skip:
        out["far_start_pairs"] = far_leg(args.pairs, args.points, args.submap, robust)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
