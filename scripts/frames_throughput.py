"""Many frames against one resident map: the serial loop (dcreg_set_source + dcreg_icp_run per frame) against dcreg_register_frames at
16 / 64 / 256 slots, 256 frames of 8 k points cut out of the 200 k-point parking lot (--prior-map: also out of the 50 M-point prior map).
Upload included on both sides; a host clock around calls that end in a synchronise; one warm-up pass of each first; seeded inputs.  Also
checks that every frame's record is bitwise the serial loop's.  Prints one JSON line.

usage: python scripts/frames_throughput.py [--frames 256] [--points 8000] [--prior-map] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402


def frame_poses(n, seed, step):
    rng = np.random.default_rng(seed)
    gt = scenes.pose6d_matrix(**scenes.PK01_GT)
    T, T0 = [], []
    for _ in range(n):
        Tk = gt @ scenes.pose6d_matrix(rng.uniform(-step, step), rng.uniform(-step, step), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-20, 20)))
        T.append(Tk)
        T0.append(Tk @ scenes.pose6d_matrix(*rng.uniform(-0.15, 0.15, 3), *np.deg2rad(rng.uniform(-0.5, 0.5, 3))))
    return gt, T, T0


def record(r):
    return (r.iterations, r.converged, r.status, tuple(r.final_transform[:]), r.final_rmse, r.final_fitness, r.corr_num, tuple(r.H_upper[:]),
            tuple(r.degenerate_mask[:]))


def serial(ctx, frames, T0, cfg):
    out = []
    for f, T in zip(frames, T0):
        ctx.set_source(f)
        res, logs = ctx.icp_run(T, "Ours", cfg)
        last = logs[-1] if logs else None
        Tf = np.eye(4)
        Tf[:3, :3] = np.array(res.R[:]).reshape(3, 3)
        Tf[:3, 3] = res.t[:]
        out.append((res.iterations, res.converged, res.status, tuple(Tf.reshape(16)), last.rmse if last else 0.0, last.fitness if last else 0.0,
                    last.effective_points if last else 0, tuple(last.H_upper[:]) if last else (0.0,) * 21,
                    tuple(last.analysis.degenerate_mask[:]) if last else (0,) * 6))
    return out


def leg(name, tgt, frames, T0, cfg, repeats):
    ctx = api.Context(0)
    try:
        ctx.set_target(tgt, 0.5)
        ref = serial(ctx, frames, T0, cfg)                      # warm-up of the serial loop
        best = None
        for _ in range(repeats):
            t = time.perf_counter()
            got = serial(ctx, frames, T0, cfg)                 # (icp_run returns its result: the stream has drained)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        assert got == ref
        iters = sum(r[0] for r in ref)
        line = {"serial": {"frames_per_s": len(frames) / best, "it_per_s": iters / best, "ms": 1e3 * best}}
        bitwise = True
        for slots in (16, 64, 256):
            recs = ctx.register_frames(frames, T0, "Ours", cfg, slots=slots)         # warm-up
            bitwise &= [record(r) for r in recs] == ref
            best = None
            for _ in range(repeats):
                t = time.perf_counter()
                recs = ctx.register_frames(frames, T0, "Ours", cfg, slots=slots)     # (returns after the last result has been waited for)
                dt = time.perf_counter() - t
                best = dt if best is None else min(best, dt)
                bitwise &= [record(r) for r in recs] == ref
            line["slots_%d" % slots] = {"frames_per_s": len(frames) / best, "it_per_s": iters / best, "ms": 1e3 * best,
                                        "x_serial": line["serial"]["ms"] / (1e3 * best)}
        line.update(iterations=iters, converged=sum(r[1] for r in ref), bitwise_equal_to_serial=bool(bitwise))
        return line
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--prior-map", action="store_true", help="also the 50 M-point prior map (600 MB of map, ~1 min to build)")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"frames": a.frames, "points": a.points}
    tgt, _ = scenes.scene_parkinglot()
    gt, T, T0 = frame_poses(a.frames, 5, 6.0)
    frames = scenes.map_frames(tgt, T, a.points, seed=3)
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1, gt_matrix=gt.reshape(16))
    out["parkinglot_200k"] = leg("parkinglot_200k", tgt, frames, T0, cfg, a.repeats)
    if a.prior_map:
        tgt, _ = scenes.scene_prior_map(50_000_000)
        frames = scenes.map_frames(tgt, T, a.points, seed=3)
        out["prior_map_50m"] = leg("prior_map_50m", tgt, frames, T0, cfg, a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
