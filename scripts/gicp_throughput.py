"""The third engine (dcreg_icp_run_gicp: plane-to-plane rows from the map's kept normals and the source's own) beside the second
(dcreg_icp_run_normals) and the first (dcreg_icp_run) on the device.  A host clock around calls that end in a synchronise, after
warm-up; medians.  For each pair - the parking lot with a 200 k map and an 8 k frame (c3), the same with a 200 k frame, the 1 M x 1 M
corridor (c4) -
  keep_target_ms / keep_source_ms   dcreg_target_normals_keep and dcreg_source_normals_keep (k = 5, unbounded)
  gicp / normals / plane            one registration with "Ours", thresholds on, from the pair's start pose, all three in the same loop on
                                    the same box: run_ms, iterations, ms per iteration, the time of one linearisation call (host clock:
                                    alternating between the start pose and the final one, and repeated at the final pose), and the final
                                    pose errors against the truth
and, once, the cost of dcreg_source_normals_keep for an 8 k and a 131 k frame.  Prints one JSON line.

usage: python scripts/gicp_throughput.py [--repeats 7] [--skip c4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def pairs(skip):
    small = scenes.pose6d_matrix(0.05, -0.08, 0.03, scenes.deg2rad(0.2), scenes.deg2rad(-0.1), scenes.deg2rad(0.5))
    pk_gt, pk_init = scenes.pose6d_matrix(**scenes.PK01_GT), scenes.pose6d_matrix(**scenes.PK01_INIT)
    if "c3" not in skip:
        tgt, src = scenes.scene_parkinglot()
        yield "c3_pk01_200k_x_8k", tgt, src, pk_gt, pk_init, 0.5, 0
    if "c3full" not in skip:
        tgt, src = scenes.scene_parkinglot(n_map=200_000, n_frame=200_000, frame_range=100.0)
        yield "c3_pk01_200k_x_200k", tgt, src, pk_gt, pk_init, 0.5, 0
    if "c4" not in skip:
        tgt = scenes.scene_corridor(1_000_000, seed=0)
        src = (tgt + np.random.default_rng(1000).normal(0, 0.01, tgt.shape)).astype(np.float32)
        yield "c4_corridor_1m", tgt, src, np.eye(4), small, 1.0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip", default="")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    out = {}
    k5 = api.normal_params(k=5)
    for name, tgt, src, gt, init, radius, wd in pairs(skip):
        ctx = api.Context(0)
        ctx.set_target(tgt, radius)
        ctx.set_source(src)
        cfg = api.default_config(search_radius=radius, max_iterations=30, use_weight_derivative=wd, gt_matrix=gt.reshape(-1))
        rec = {"map_points": int(len(tgt)), "frame_points": int(len(src))}
        rec["keep_target_ms"] = timed(lambda: ctx.keep_target_normals(k5), max(args.repeats // 2, 1), warmup=1)
        info = ctx.keep_source_normals(k5)
        rec["keep_source_ms"] = timed(lambda: ctx.keep_source_normals(k5), max(args.repeats // 2, 1), warmup=0)
        rec["source_normals_sparse"] = info["n_sparse"]
        prm = api.default_lin_params(radius, wd)
        for engine, run, lin in (("gicp", ctx.icp_run_gicp, lambda T: ctx.linearize_gicp(T, prm)),
                                 ("normals", ctx.icp_run_normals, lambda T: ctx.linearize_normals(T, prm)),
                                 ("plane", ctx.icp_run, lambda T: ctx.linearize(T[:3, :3], T[:3, 3], prm))):
            res, logs = run(init, "Ours", cfg)
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = np.array(res.R[:]).reshape(3, 3), res.t[:]
            te, re_ = api.pose_error(gt, T)
            ms = timed(lambda: run(init, "Ours", cfg, log_capacity=0), args.repeats)
            e = {"run_ms": ms, "iterations": int(res.iterations), "converged": int(res.converged), "status": int(res.status),
                 "ms_per_iteration": ms / max(res.iterations, 1), "trans_err_m": te, "rot_err_deg": re_,
                 "n_eff_last": int(logs[-1].effective_points) if logs else 0}
            lin(init)
            e["lin_first_ms"] = timed(lambda: (lin(init), lin(T)), args.repeats, warmup=1) / 2.0      # a jump and back: searches from far bounds
            lin(T)
            e["lin_settled_ms"] = timed(lambda: lin(T), args.repeats * 3)                              # the same pose again: warm
            rec[engine] = e
        rec["gicp_over_normals_settled"] = rec["gicp"]["lin_settled_ms"] / rec["normals"]["lin_settled_ms"]
        out[name] = rec
        ctx.close()
    if "keep" not in skip:
        ctx = api.Context(0)
        for n, rng_ in ((8_192, 30.0), (131_072, 100.0)):
            _, src = scenes.scene_parkinglot(n_map=200_000, n_frame=n, frame_range=rng_)      # (a frame is drawn from the map's points)
            ctx.set_source(src)
            out["keep_source_%d" % len(src)] = {"frame_points": int(len(src)),
                                                "keep_source_ms": timed(lambda: ctx.keep_source_normals(k5), args.repeats, warmup=1)}
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
