"""Many scan pairs through all three engines: per engine the serial loop its pairs call promises on one context (dcreg_set_target
[+ dcreg_target_normals_keep] + dcreg_set_source [+ dcreg_source_normals_keep] + dcreg_icp_run / _normals / _gicp per pair) and the pairs
call itself (dcreg_register_pairs, dcreg_register_pairs_normals, dcreg_register_pairs_gicp) at 64 and 256 slots.  Uploads, index builds and
normal estimation are included everywhere.  The two workloads of scripts/pairs_throughput.py out of the 200 k-point parking lot: 256
frames of 8 k points against 100 k-point submap crops (loop-closure verification), and 512 scan-to-scan pairs of 8 k-point frames.  The
map's normals are bounded at the search radius, the frames' own are k = 5 unbounded.  A host clock around calls that end in a
synchronise; one warm-up pass of each first; seeded inputs; all in one process.  Checks that every pairs record is bitwise the serial
loop's.  Prints one JSON line.

usage: python scripts/pairs_engines_throughput.py [--pairs 256] [--scan-pairs 512] [--points 8000] [--submap 100000] [--repeats 3]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402
from pairs_throughput import best_of, drive, pose_of, record  # noqa: E402

ENGINES = ("planes", "normals", "gicp")


def serial(ctx, engine, srcs, tgts, T0, cfg, tn, sn):
    out = []
    for s, t, T in zip(srcs, tgts, T0):
        ctx.set_target(t, cfg.search_radius)
        if engine != "planes":
            ctx.keep_target_normals(tn)
        ctx.set_source(s)
        if engine == "gicp":
            ctx.keep_source_normals(sn)
        run = {"planes": ctx.icp_run, "normals": ctx.icp_run_normals, "gicp": ctx.icp_run_gicp}[engine]
        res, logs = run(T, "Ours", cfg)
        last = logs[-1] if logs else None
        out.append((res.iterations, res.converged, res.status, tuple(pose_of(res).reshape(16)), last.rmse if last else 0.0,
                    last.fitness if last else 0.0, last.effective_points if last else 0, tuple(last.H_upper[:]) if last else (0.0,) * 21,
                    tuple(last.analysis.degenerate_mask[:]) if last else (0,) * 6))
    return out


def batched(ctx, engine, srcs, tgts, T0, cfg, tn, sn, slots):
    if engine == "planes":
        return ctx.register_pairs(srcs, tgts, T0, "Ours", cfg, slots=slots)
    if engine == "normals":
        return ctx.register_pairs_normals(srcs, tgts, T0, "Ours", cfg, tn, slots=slots)
    return ctx.register_pairs_gicp(srcs, tgts, T0, "Ours", cfg, tn, sn, slots=slots)


def leg(srcs, tgts, T0, cfg, repeats):
    n = len(srcs)
    tn, sn = api.normal_params(k=5, search_radius=cfg.search_radius), api.normal_params(k=5)
    ctx = api.Context(0)
    line = {"pairs": n}
    try:
        for engine in ENGINES:
            ref = serial(ctx, engine, srcs, tgts, T0, cfg, tn, sn)                      # warm-up
            dt, got = best_of(lambda: serial(ctx, engine, srcs, tgts, T0, cfg, tn, sn), repeats)
            assert got == ref
            e = {"serial": {"pairs_per_s": n / dt, "ms": 1e3 * dt}, "iterations": sum(r[0] for r in ref), "converged": sum(r[1] for r in ref)}
            bitwise = True
            for slots in (64, 256):
                recs = batched(ctx, engine, srcs, tgts, T0, cfg, tn, sn, slots)          # warm-up
                bitwise &= [record(r) for r in recs] == ref
                dt, recs = best_of(lambda: batched(ctx, engine, srcs, tgts, T0, cfg, tn, sn, slots), repeats)
                bitwise &= [record(r) for r in recs] == ref
                e["slots_%d" % slots] = {"pairs_per_s": n / dt, "ms": 1e3 * dt, "x_serial": e["serial"]["ms"] / (1e3 * dt)}
            # the batched build alone (sources loaded, targets indexed, normals estimated, nothing run)
            build_cfg = api.default_config(search_radius=cfg.search_radius, max_iterations=0)
            batched(ctx, engine, srcs, tgts, T0, build_cfg, tn, sn, 0)
            dt, _ = best_of(lambda: batched(ctx, engine, srcs, tgts, T0, build_cfg, tn, sn, 0), repeats)
            e["build_ms"] = 1e3 * dt
            e["bitwise_equal_to_serial"] = bool(bitwise)
            line[engine] = e
        return line
    finally:
        ctx.close()


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
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1)
    if a.pairs > 0:
        poses = [gt @ scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-20, 20)))
                 for _ in range(a.pairs)]
        srcs, tgts, Tt = scenes.scan_pairs(tgt, poses, a.points, seed=3, mode="submap", n_submap=a.submap, submap_radius=45.0)
        T0 = [T @ scenes.pose6d_matrix(*rng.uniform(-0.15, 0.15, 3), *np.deg2rad(rng.uniform(-0.5, 0.5, 3))) for T in Tt]
        out["submap"] = leg(srcs, tgts, T0, cfg, a.repeats)
        out["submap"]["target_points"] = int(np.mean([len(t) for t in tgts]))
    if a.scan_pairs > 0:
        _, drv = drive(a.scan_pairs + 1, 9, 1.0)
        srcs, tgts, Tt = scenes.scan_pairs(tgt, drv, a.points, seed=6, mode="scan")
        T0 = [T @ scenes.pose6d_matrix(*rng.uniform(-0.1, 0.1, 3), *np.deg2rad(rng.uniform(-0.5, 0.5, 3))) for T in Tt]
        out["scan_to_scan"] = leg(srcs, tgts, T0, cfg, a.repeats)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
