"""What the robust kernels of the second and third engine cost and what they buy ("robust_kernel", include/dcreg.h).  One process, one
box; every leg runs kernel 0 (none: the code path from before the option) and kernel 3 (Geman-McClure) ALTERNATING in the same loop, so
the yardstick of every figure is kernel 0 beside it.  A host clock around calls that end in a synchronise, after warm-up.
  lin        the time of one dcreg_linearize_normals / dcreg_linearize_gicp call at a settled pose (the same pose again: warm), for the
             parking lot's 8 k frame against its 200 k map (c3) and for the 1 M x 1 M corridor (c4): per kernel the median over all
             rounds, and the spread of the rounds' medians (min .. max) - the difference between the kernels is to be read against the
             spread of kernel 0 alone
  clean      one registration ("Ours", thresholds on, max_iterations 40) of the 8 k frame with both engines: time, iterations, final error
             - for kernels 0, 2 (Cauchy) and 3, and "staged": kernel 0 to its end, then kernel 3 from the pose it reached
  dirty      the same for the CONTAMINATED 8 k frame: the fifth of its points nearest a seeded frame point moved by (0.125, 0, 0.25) m
             in the sensor frame, as an object that has moved since the map was built
Scales: robust_scale 0.05 m, gicp_robust_scale 1.0.  Prints one JSON line.

usage: python scripts/robust_throughput.py [--rounds 9] [--calls 20] [--skip c4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402

KERNELS = (0, 3)
SCALE, GICP_SCALE = 0.05, 1.0


def pose_of(res):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.array(res.R[:]).reshape(3, 3), res.t[:]
    return T


def lin_leg(ctx, lin, T, rounds, calls):
    """per kernel: every round's median time of one call at T, kernels alternating round by round"""
    per = {k: [] for k in KERNELS}
    for k in KERNELS:                                   # warm-up of both code paths
        ctx.set_option("robust_kernel", k)
        for _ in range(3):
            lin(T)
    for _ in range(rounds):
        for k in KERNELS:
            ctx.set_option("robust_kernel", k)
            lin(T)
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                lin(T)
                ts.append((time.perf_counter() - t0) * 1e3)
            per[k].append(float(np.median(ts)))
    ctx.set_option("robust_kernel", 0)
    out = {}
    for k in KERNELS:
        out["kernel_%d" % k] = {"ms": float(np.median(per[k])), "rounds_min_ms": float(np.min(per[k])), "rounds_max_ms": float(np.max(per[k]))}
    out["kernel_3_minus_0_us"] = 1e3 * (out["kernel_3"]["ms"] - out["kernel_0"]["ms"])
    out["kernel_0_spread_us"] = 1e3 * (out["kernel_0"]["rounds_max_ms"] - out["kernel_0"]["rounds_min_ms"])
    return out


def run_leg(ctx, run, init, cfg, gt, rounds, kernels=(0, 2, 3)):
    """per kernel (Cauchy too): one registration from `init` - time (median over the rounds, kernels alternating), iterations, final
    error; and "staged": kernel 0 to its end, then Geman-McClure from the pose it reached (both runs timed together)"""
    per = {k: [] for k in kernels}
    rec = {}
    for k in kernels:
        ctx.set_option("robust_kernel", k)
        res, logs = run(init, "Ours", cfg, log_capacity=cfg.max_iterations)
        te, re_ = api.pose_error(gt, pose_of(res))
        rec["kernel_%d" % k] = {"iterations": int(res.iterations), "converged": int(res.converged), "status": int(res.status),
                                "trans_err_m": te, "rot_err_deg": re_, "n_eff_last": int(logs[-1].effective_points) if logs else 0}
    staged = []
    for _ in range(rounds):
        for k in kernels:
            ctx.set_option("robust_kernel", k)
            t0 = time.perf_counter()
            run(init, "Ours", cfg, log_capacity=0)
            per[k].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctx.set_option("robust_kernel", 0)
        first, _ = run(init, "Ours", cfg, log_capacity=0)
        ctx.set_option("robust_kernel", 3)
        second, _ = run(pose_of(first), "Ours", cfg, log_capacity=0)
        staged.append((time.perf_counter() - t0) * 1e3)
    ctx.set_option("robust_kernel", 0)
    for k in kernels:
        e = rec["kernel_%d" % k]
        e["run_ms"] = float(np.median(per[k]))
        e["ms_per_iteration"] = e["run_ms"] / max(e["iterations"], 1)
    te, re_ = api.pose_error(gt, pose_of(second))
    rec["staged_0_then_3"] = {"run_ms": float(np.median(staged)), "iterations": int(first.iterations) + int(second.iterations),
                              "converged": int(second.converged), "trans_err_m": te, "rot_err_deg": re_}
    return rec


def contaminate(src, share=0.2, shift=(0.125, 0.0, 0.25), seed=7):
    rng = np.random.default_rng(seed)
    s = int(rng.integers(len(src)))
    d = np.linalg.norm(src[:, :3].astype(np.float64) - src[s, :3].astype(np.float64), axis=1)
    moved = np.argsort(d, kind="stable")[:int(round(share * len(src)))]
    out = np.array(src)
    out[moved, :3] = (out[moved, :3].astype(np.float64) + np.array(shift)).astype(np.float32)
    return out, len(moved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip", default="")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    out = {"robust_scale": SCALE, "gicp_robust_scale": GICP_SCALE}
    k5 = api.normal_params(k=5)
    pk_gt, pk_init = scenes.pose6d_matrix(**scenes.PK01_GT), scenes.pose6d_matrix(**scenes.PK01_INIT)
    small = scenes.pose6d_matrix(0.05, -0.08, 0.03, scenes.deg2rad(0.2), scenes.deg2rad(-0.1), scenes.deg2rad(0.5))

    def context(tgt, src, radius):
        ctx = api.Context(0)
        ctx.set_target(tgt, radius)
        ctx.set_source(src)
        ctx.keep_target_normals(k5)
        ctx.keep_source_normals(k5)
        ctx.set_option("robust_scale", SCALE)
        ctx.set_option("gicp_robust_scale", GICP_SCALE)
        return ctx

    def engines(ctx, prm):
        return (("normals", ctx.icp_run_normals, lambda T: ctx.linearize_normals(T, prm)),
                ("gicp", ctx.icp_run_gicp, lambda T: ctx.linearize_gicp(T, prm)))

    if "c3" not in skip:
        tgt, src = scenes.scene_parkinglot()
        cfg = api.default_config(search_radius=0.5, max_iterations=40, use_weight_derivative=0, gt_matrix=pk_gt.reshape(-1))
        prm = api.default_lin_params(0.5, 0)
        ctx = context(tgt, src, 0.5)
        rec = {"map_points": int(len(tgt)), "frame_points": int(len(src))}
        for name, run, lin in engines(ctx, prm):
            res, _ = run(pk_init, "Ours", cfg)                       # kernel 0: the settled pose of this engine
            rec[name] = {"lin": lin_leg(ctx, lin, pose_of(res), args.rounds, args.calls),
                         "clean": run_leg(ctx, run, pk_init, cfg, pk_gt, args.rounds)}
        dirty, n_moved = contaminate(src)
        ctx.set_source(dirty)
        ctx.keep_source_normals(k5)
        rec["moved_points"] = n_moved
        for name, run, _ in engines(ctx, prm):
            rec[name]["dirty"] = run_leg(ctx, run, pk_init, cfg, pk_gt, args.rounds)
        out["c3_pk01_200k_x_8k"] = rec
        ctx.close()
    if "c4" not in skip:
        tgt = scenes.scene_corridor(1_000_000, seed=0)
        src = (tgt + np.random.default_rng(1000).normal(0, 0.01, tgt.shape)).astype(np.float32)
        cfg = api.default_config(search_radius=1.0, max_iterations=30, use_weight_derivative=1, gt_matrix=np.eye(4).reshape(-1))
        prm = api.default_lin_params(1.0, 1)
        ctx = context(tgt, src, 1.0)
        rec = {"map_points": int(len(tgt)), "frame_points": int(len(src))}
        for name, run, lin in engines(ctx, prm):
            res, _ = run(small, "Ours", cfg)
            rec[name] = {"lin": lin_leg(ctx, lin, pose_of(res), max(args.rounds // 2, 3), max(args.calls // 2, 5))}
        out["c4_corridor_1m"] = rec
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
