"""Many scan pairs, each against its own target: the serial loop on one context (dcreg_set_target + dcreg_set_source + dcreg_icp_run per
pair), dcreg_icp_run_many over 8 contexts (8 pairs at a time, each context given its pair's clouds first), and dcreg_register_pairs at
16 / 64 / 256 slots.  Uploads and index builds are included everywhere.  Two workloads out of the 200 k-point parking lot: 256 frames of
8 k points against 100 k-point submap crops (loop-closure verification), and 512 scan-to-scan pairs of 8 k-point frames (odometry of a
recorded drive).  Also reported: the batched build alone (register_pairs with max_iterations = 0: sources loaded, targets indexed, nothing
run) and dcreg_set_target of all targets as ONE cloud.  A host clock around calls that end in a synchronise; one warm-up pass of each
first; seeded inputs.  Checks that every register_pairs record is bitwise the serial loop's.  Prints one JSON line.

usage: python scripts/pairs_throughput.py [--pairs 256] [--scan-pairs 512] [--points 8000] [--submap 100000] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402


def record(r):
    return (r.iterations, r.converged, r.status, tuple(r.final_transform[:]), r.final_rmse, r.final_fitness, r.corr_num, tuple(r.H_upper[:]),
            tuple(r.degenerate_mask[:]))


def pose_of(res):
    T = np.eye(4)
    T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
    T[:3, 3] = res.t[:]
    return T


def serial(ctx, srcs, tgts, T0, cfg):
    out = []
    for s, t, T in zip(srcs, tgts, T0):
        ctx.set_target(t, cfg.search_radius)
        ctx.set_source(s)
        res, logs = ctx.icp_run(T, "Ours", cfg)
        last = logs[-1] if logs else None
        out.append((res.iterations, res.converged, res.status, tuple(pose_of(res).reshape(16)), last.rmse if last else 0.0,
                    last.fitness if last else 0.0, last.effective_points if last else 0, tuple(last.H_upper[:]) if last else (0.0,) * 21,
                    tuple(last.analysis.degenerate_mask[:]) if last else (0,) * 6))
    return out


def many(ctxs, srcs, tgts, T0, cfg):
    out = []
    k = len(ctxs)
    for i in range(0, len(srcs), k):
        part = list(range(i, min(i + k, len(srcs))))
        for c, p in zip(ctxs, part):
            c.set_target(tgts[p], cfg.search_radius)
            c.set_source(srcs[p])
        for res in api.icp_run_many(ctxs[:len(part)], [T0[p] for p in part], "Ours", cfg):
            out.append((res.iterations, res.converged, res.status, tuple(pose_of(res).reshape(16))))
    return out


def best_of(fn, repeats):
    best, got = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        got = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best, got


def leg(srcs, tgts, T0, cfg, repeats):
    n = len(srcs)
    ctx = api.Context(0)
    ctxs = [api.Context(0) for _ in range(8)]
    try:
        ref = serial(ctx, srcs, tgts, T0, cfg)                      # warm-up
        dt, got = best_of(lambda: serial(ctx, srcs, tgts, T0, cfg), repeats)
        assert got == ref
        iters = sum(r[0] for r in ref)
        line = {"serial": {"pairs_per_s": n / dt, "ms": 1e3 * dt}}
        m = many(ctxs, srcs, tgts, T0, cfg)
        dt, m = best_of(lambda: many(ctxs, srcs, tgts, T0, cfg), repeats)
        line["icp_run_many_8"] = {"pairs_per_s": n / dt, "ms": 1e3 * dt, "x_serial": line["serial"]["ms"] / (1e3 * dt),
                                  "equal_to_serial": m == [r[:4] for r in ref]}
        bitwise = True
        for slots in (16, 64, 256):
            recs = ctx.register_pairs(srcs, tgts, T0, "Ours", cfg, slots=slots)        # warm-up
            bitwise &= [record(r) for r in recs] == ref
            dt, recs = best_of(lambda: ctx.register_pairs(srcs, tgts, T0, "Ours", cfg, slots=slots), repeats)
            bitwise &= [record(r) for r in recs] == ref
            line["slots_%d" % slots] = {"pairs_per_s": n / dt, "ms": 1e3 * dt, "x_serial": line["serial"]["ms"] / (1e3 * dt),
                                        "x_icp_run_many_8": line["icp_run_many_8"]["ms"] / (1e3 * dt)}
        # the batched build alone: no iteration runs
        build_cfg = api.default_config(search_radius=cfg.search_radius, max_iterations=0)
        ctx.register_pairs(srcs, tgts, T0, "Ours", build_cfg)
        dt, _ = best_of(lambda: ctx.register_pairs(srcs, tgts, T0, "Ours", build_cfg), repeats)
        line["build_ms"] = 1e3 * dt
        whole = np.concatenate(tgts, 0)
        ctx.set_target(whole, cfg.search_radius)
        dt, _ = best_of(lambda: ctx.set_target(whole, cfg.search_radius), repeats)
        line["set_target_all_as_one_ms"] = 1e3 * dt
        line["set_target_all_as_one_points"] = int(len(whole))
        line.update(pairs=n, iterations=iters, converged=sum(r[1] for r in ref), bitwise_equal_to_serial=bool(bitwise))
        return line
    finally:
        ctx.close()
        for c in ctxs:
            c.close()


def drive(n, seed, step):
    """n sensor poses along a drive through the lot: ~step metres and a few degrees of heading apart"""
    rng = np.random.default_rng(seed)
    gt = scenes.pose6d_matrix(**scenes.PK01_GT)
    T = [gt @ scenes.pose6d_matrix(-25.0, -25.0, 0.0, 0.0, 0.0, 0.0)]
    for _ in range(n - 1):
        T.append(T[-1] @ scenes.pose6d_matrix(step * (0.5 + rng.random()), 0.0, 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-4, 4))))
        T[-1][:2, 3] = gt[:2, 3] + np.clip(T[-1][:2, 3] - gt[:2, 3], -30.0, 30.0)
    return gt, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--scan-pairs", type=int, default=512)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--submap", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"points": a.points}
    tgt, _ = scenes.scene_parkinglot()
    rng = np.random.default_rng(5)
    gt = scenes.pose6d_matrix(**scenes.PK01_GT)
    poses = [gt @ scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-20, 20)))
             for _ in range(a.pairs)]
    srcs, tgts, Tt = scenes.scan_pairs(tgt, poses, a.points, seed=3, mode="submap", n_submap=a.submap, submap_radius=45.0)
    T0 = [T @ scenes.pose6d_matrix(*rng.uniform(-0.15, 0.15, 3), *np.deg2rad(rng.uniform(-0.5, 0.5, 3))) for T in Tt]
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1)
    out["submap"] = leg(srcs, tgts, T0, cfg, a.repeats)
    out["submap"]["target_points"] = int(np.mean([len(t) for t in tgts]))
    _, drv = drive(a.scan_pairs + 1, 9, 1.0)
    srcs, tgts, Tt = scenes.scan_pairs(tgt, drv, a.points, seed=6, mode="scan")
    T0 = [T @ scenes.pose6d_matrix(*rng.uniform(-0.1, 0.1, 3), *np.deg2rad(rng.uniform(-0.5, 0.5, 3))) for T in Tt]
    out["scan_to_scan"] = leg(srcs, tgts, T0, cfg, a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
