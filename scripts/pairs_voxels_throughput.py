"""Many scan pairs through the fourth engine (rows against per-voxel Gaussians), a voxel map per target: the two workloads of
scripts/pairs_engines_throughput.py out of the 200 k-point parking lot - 256 frames of 8 k points against 100 k-point submap crops
(loop-closure verification) and 512 scan-to-scan pairs of 8 k-point frames - method "Ours", thresholds on, uploads and builds included on
all sides.  For leaf 1.0 and 0.5 and "voxels_source_cov" 0 and 1 the legs are timed in the SAME loop of one process - every repeat runs
all legs of all configurations, one after the other, each under its own synchronise, a host clock, one warm-up pass of each first:
  (a) serial           the loop dcreg_set_target + dcreg_target_voxels_keep + dcreg_set_source [+ dcreg_source_normals_keep in mode 1] +
                       dcreg_icp_run_voxels per pair: the only way before the pairs call
  (b) voxels_<slots>   dcreg_register_pairs_voxels at 256 / 64 / 16 slots
  (c) normals, gicp    dcreg_register_pairs_normals / dcreg_register_pairs_gicp on the same pairs at 64 slots (once per repeat)
and per leg the minimum and the maximum over the repeats (their difference is the spread a ratio is judged against).  Asserts that every
record of (b) is bitwise the serial loop's (a target that keeps no voxel: status 3).  "build_ms" is a call with max_iterations = 0: the
sources' load, in mode 1 their normals, and every batch's voxel maps, nothing stepped.  The engine's own per-step timing line
(DCREG_TRIALS_TIMING) is printed for one 64-slot call of every configuration, on stderr.  One more leg starts the submap pairs OUTSIDE the
0.5 m search radius of the 1-NN engines - 1 to 2 m and up to 3 degrees per axis off - and reports converged pairs and final errors for the
voxel form (all four configurations) and for the two 1-NN forms.  Prints one JSON line.

usage: python scripts/pairs_voxels_throughput.py [--pairs 256] [--scan-pairs 512] [--points 8000] [--submap 100000] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402
from frames_normals_throughput import errors  # noqa: E402
from pairs_throughput import drive, pose_of, record  # noqa: E402

SLOTS = (256, 64, 16)
CONFIGS = [(leaf, mode) for leaf in (1.0, 0.5) for mode in (0, 1)]
NOTHING = (0, 0, 3, (0.0,) * 16, 0.0, 0.0, 0, (0.0,) * 21, (0,) * 6)       # the call's record for a target that keeps no voxel


def serial(ctx, srcs, tgts, T0, cfg, vp, sn, mode):
    out = []
    for s, t, T in zip(srcs, tgts, T0):
        ctx.set_target(t, cfg.search_radius)
        if ctx.keep_target_voxels(vp)["n_kept"] == 0:
            out.append(NOTHING)
            continue
        ctx.set_source(s)
        if mode:
            ctx.keep_source_normals(sn)
        res, logs = ctx.icp_run_voxels(T, "Ours", cfg)
        last = logs[-1] if logs else None
        out.append((res.iterations, res.converged, res.status, tuple(pose_of(res).reshape(16)), last.rmse if last else 0.0,
                    last.fitness if last else 0.0, last.effective_points if last else 0, tuple(last.H_upper[:]) if last else (0.0,) * 21,
                    tuple(last.analysis.degenerate_mask[:]) if last else (0,) * 6))
    return out


def stage(recs, truth):
    """mean iterations, converged pairs and the final errors of the pairs that ran (status 3: nothing ran, the record has no pose)"""
    n = len(recs)
    it = [r[0] if isinstance(r, tuple) else r.iterations for r in recs]
    cv = [r[1] if isinstance(r, tuple) else r.converged for r in recs]
    ran = [(r, T) for r, T in zip(recs, truth) if (r[2] if isinstance(r, tuple) else r.status) != 3]
    err = errors([r for r, _ in ran], [T for _, T in ran]) if ran else {}
    return dict(mean_iterations=sum(it) / n, converged=int(sum(cv)), **err)


def workload(ctx, srcs, tgts, T0, truth, cfg, repeats):
    n = len(srcs)
    sn, tn = api.normal_params(k=5), api.normal_params(k=5, search_radius=cfg.search_radius)
    build_cfg = api.default_config(search_radius=cfg.search_radius, max_iterations=0)

    def batched(leaf, mode, slots, c=cfg, starts=T0):
        ctx.set_option("voxels_source_cov", mode)
        return ctx.register_pairs_voxels(srcs, tgts, starts, "Ours", c, api.voxel_map_params(leaf), sn if mode else None, slots=slots)

    def one_nn(engine, starts=T0):
        if engine == "normals":
            return ctx.register_pairs_normals(srcs, tgts, starts, "Ours", cfg, tn, slots=64)
        return ctx.register_pairs_gicp(srcs, tgts, starts, "Ours", cfg, tn, sn, slots=64)

    # ---- warm-up of every leg, and the bitwise check
    ref = {}
    for leaf, mode in CONFIGS:
        ctx.set_option("voxels_source_cov", mode)
        ref[(leaf, mode)] = serial(ctx, srcs, tgts, T0, cfg, api.voxel_map_params(leaf), sn, mode)
        for s in SLOTS:
            assert [record(r) for r in batched(leaf, mode, s)] == ref[(leaf, mode)], "register_pairs_voxels at %d slots is not the serial loop" % s
        batched(leaf, mode, 0, build_cfg)
    nn = {e: one_nn(e) for e in ("normals", "gicp")}
    # ---- the timed loop: every leg of every configuration in every repeat
    times = {}

    def timed(key, fn):
        t = time.perf_counter()
        got = fn()
        times.setdefault(key, []).append(time.perf_counter() - t)
        return got

    for _ in range(repeats):
        for leaf, mode in CONFIGS:
            ctx.set_option("voxels_source_cov", mode)
            timed((leaf, mode, "serial"), lambda: serial(ctx, srcs, tgts, T0, cfg, api.voxel_map_params(leaf), sn, mode))
            for s in SLOTS:
                got = timed((leaf, mode, "voxels_%d" % s), lambda: batched(leaf, mode, s))
                assert [record(r) for r in got] == ref[(leaf, mode)], "voxels_%d is not the serial loop" % s
            timed((leaf, mode, "build"), lambda: batched(leaf, mode, 0, build_cfg))
        for e in ("normals", "gicp"):
            timed(e, lambda: one_nn(e))
    os.environ["DCREG_TRIALS_TIMING"] = "1"
    for leaf, mode in CONFIGS:
        sys.stderr.write("%d pairs, leaf %.1f mode %d, 64 slots: " % (n, leaf, mode))
        sys.stderr.flush()
        batched(leaf, mode, 64)
    del os.environ["DCREG_TRIALS_TIMING"]
    out = {"pairs": n, "target_points": int(np.mean([len(t) for t in tgts])), "bitwise_equal_to_serial": True, "configs": []}
    for leaf, mode in CONFIGS:
        r = ref[(leaf, mode)]
        row = {"leaf": leaf, "mode": mode, "status_1": sum(x[2] == 1 for x in r), "status_3": sum(x[2] == 3 for x in r), **stage(r, truth)}
        ts = times[(leaf, mode, "serial")]
        for name in ["serial"] + ["voxels_%d" % s for s in SLOTS] + ["build"]:
            t = times[(leaf, mode, name)]
            row[name] = {"ms_min": 1e3 * min(t), "ms_max": 1e3 * max(t), "x_serial": min(ts) / min(t)}
        b = times[(leaf, mode, "voxels_64")]
        # the condition of the change: at 64 slots faster than the serial loop by more than the larger spread of either leg
        row["gain_64_ms"] = 1e3 * (min(ts) - min(b))
        row["spread_ms"] = 1e3 * max(max(ts) - min(ts), max(b) - min(b))
        row["faster_beyond_spread"] = bool(row["gain_64_ms"] > row["spread_ms"])
        out["configs"].append(row)
    for e in ("normals", "gicp"):
        out["pairs_" + e] = {"ms_min": 1e3 * min(times[e]), "ms_max": 1e3 * max(times[e]), **stage(nn[e], truth)}
    return out, batched, one_nn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--scan-pairs", type=int, default=512)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--submap", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    out = {"points": a.points, "repeats": a.repeats}
    tgt, _ = scenes.scene_parkinglot()
    rng = np.random.default_rng(5)
    gt = scenes.pose6d_matrix(**scenes.PK01_GT)
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1)
    ctx = api.Context(0)
    try:
        if a.pairs > 0:
            poses = [gt @ scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-20, 20)))
                     for _ in range(a.pairs)]
            srcs, tgts, Tt = scenes.scan_pairs(tgt, poses, a.points, seed=3, mode="submap", n_submap=a.submap, submap_radius=45.0)
            T0 = [T @ scenes.pose6d_matrix(*rng.uniform(-0.15, 0.15, 3), *np.deg2rad(rng.uniform(-0.5, 0.5, 3))) for T in Tt]
            out["submap"], batched, one_nn = workload(ctx, srcs, tgts, T0, Tt, cfg, a.repeats)
            # ---- outside the basin of the 1-NN engines: 1 to 2 m off in a random direction, up to 3 degrees per axis
            far = []
            for T in Tt:
                d = rng.normal(size=3)
                d *= rng.uniform(1.0, 2.0) / np.linalg.norm(d)
                far.append(T @ scenes.pose6d_matrix(*d, *np.deg2rad(rng.uniform(-3.0, 3.0, 3))))
            legs = [{"leg": "voxels", "leaf": leaf, "mode": mode, **stage(batched(leaf, mode, 64, starts=far), Tt)} for leaf, mode in CONFIGS]
            legs += [{"leg": e, **stage(one_nn(e, starts=far), Tt)} for e in ("normals", "gicp")]
            out["submap_outside_the_basin"] = legs
        if a.scan_pairs > 0:
            _, drv = drive(a.scan_pairs + 1, 9, 1.0)
            srcs, tgts, Tt = scenes.scan_pairs(tgt, drv, a.points, seed=6, mode="scan")
            T0 = [T @ scenes.pose6d_matrix(*rng.uniform(-0.1, 0.1, 3), *np.deg2rad(rng.uniform(-0.5, 0.5, 3))) for T in Tt]
            out["scan_to_scan"], _, _ = workload(ctx, srcs, tgts, T0, Tt, cfg, a.repeats)
        print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
