"""Many frames against one resident map with the fourth engine (rows against the map's kept voxel distributions): 256 frames of 8 k points
cut out of the 200 k-point parking lot (the frames and start poses of scripts/frames_throughput.py), thresholds on, method "Ours", upload
included on all sides.  For leaf 1.0 and 0.5 and "voxels_source_cov" 0 and 1, four legs timed in the SAME loop of one process - every
repeat runs all legs of all configurations, one after the other, each under its own synchronise (every call returns after its last
result has been waited for), a host clock, one warm-up pass of each first:
  (a) serial           the loop dcreg_set_source [+ dcreg_source_normals_keep in mode 1] + dcreg_icp_run_voxels per frame: the only way
                       before the batched call
  (b) voxels_<slots>   dcreg_register_frames_voxels at 256 / 64 / 16 slots (mode 1: the frames' normals in one batched pass inside the call)
and per leg the minimum and the maximum over the repeats (their difference is the spread a ratio is judged against).  A second table has
the chain dcreg_register_frames_voxels -> dcreg_register_frames_gicp started from the poses reached against dcreg_register_frames_gicp
alone from the same starts: time, mean iterations, converged frames, mean final error against the frames' true poses.  Asserts that every
record of (b) is bitwise the serial loop's.  The engine's own per-step timing line (DCREG_TRIALS_TIMING) is printed for one 64-slot call
of every configuration, on stderr.  Prints one JSON line.

usage: python scripts/frames_voxels_throughput.py [--frames 256] [--points 8000] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402
from frames_normals_throughput import errors  # noqa: E402
from frames_throughput import frame_poses, record  # noqa: E402

SLOTS = (256, 64, 16)
CONFIGS = [(leaf, mode) for leaf in (1.0, 0.5) for mode in (0, 1)]


def serial(ctx, frames, T0, cfg, prm, mode):
    out = []
    for f, T in zip(frames, T0):
        ctx.set_source(f)
        if mode:
            ctx.keep_source_normals(prm)
        res, logs = ctx.icp_run_voxels(T, "Ours", cfg)
        last = logs[-1] if logs else None
        Tf = np.eye(4)
        Tf[:3, :3] = np.array(res.R[:]).reshape(3, 3)
        Tf[:3, 3] = res.t[:]
        out.append((res.iterations, res.converged, res.status, tuple(Tf.reshape(16)), last.rmse if last else 0.0, last.fitness if last else 0.0,
                    last.effective_points if last else 0, tuple(last.H_upper[:]) if last else (0.0,) * 21,
                    tuple(last.analysis.degenerate_mask[:]) if last else (0,) * 6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    tgt, _ = scenes.scene_parkinglot()
    gt, T, T0 = frame_poses(a.frames, 5, 6.0)
    frames = scenes.map_frames(tgt, T, a.points, seed=3)
    prm = api.normal_params(k=5)
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1, gt_matrix=gt.reshape(16))
    ctx = api.Context(0)
    try:
        ctx.set_target(tgt, 0.5)
        ctx.keep_target_normals(prm)                                      # for the chain's second stage; the fourth engine does not read them

        def select(leaf, mode):
            ctx.set_option("voxels_source_cov", mode)
            return ctx.keep_target_voxels(api.voxel_map_params(leaf))

        def batched(mode, slots):
            return ctx.register_frames_voxels(frames, T0, "Ours", cfg, prm if mode else None, slots=slots)

        # ---- warm-up of every leg, and the bitwise check
        ref, kept = {}, {}
        for leaf, mode in CONFIGS:
            kept[(leaf, mode)] = select(leaf, mode)["n_kept"]
            ref[(leaf, mode)] = serial(ctx, frames, T0, cfg, prm, mode)
            for s in SLOTS:
                assert [record(r) for r in batched(mode, s)] == ref[(leaf, mode)], "register_frames_voxels at %d slots is not the serial loop" % s
        # ---- the timed loop: every leg of every configuration in every repeat
        times = {}
        for _ in range(a.repeats):
            for leaf, mode in CONFIGS:
                select(leaf, mode)
                legs = [("serial", lambda: serial(ctx, frames, T0, cfg, prm, mode))] + [("voxels_%d" % s, lambda s=s: batched(mode, s)) for s in SLOTS]
                for name, fn in legs:
                    t = time.perf_counter()
                    got = fn()
                    times.setdefault((leaf, mode, name), []).append(time.perf_counter() - t)
                    if name != "serial":
                        assert [record(r) for r in got] == ref[(leaf, mode)], "%s is not the serial loop" % name
        # ---- the upload's share, and the engine's own timing line for one 64-slot call of every configuration
        load = []
        for _ in range(a.repeats + 1):
            t = time.perf_counter()
            ctx.frames_load(frames)
            load.append(time.perf_counter() - t)
        os.environ["DCREG_TRIALS_TIMING"] = "1"
        for leaf, mode in CONFIGS:
            select(leaf, mode)
            sys.stderr.write("leaf %.1f mode %d, 64 slots: " % (leaf, mode))
            sys.stderr.flush()
            batched(mode, 64)
        del os.environ["DCREG_TRIALS_TIMING"]
        out = {"frames": a.frames, "points": a.points, "map_points": int(len(tgt)), "repeats": a.repeats, "bitwise_equal_to_serial": True,
               "frames_load_ms": 1e3 * min(load[1:]), "configs": []}
        for leaf, mode in CONFIGS:
            r = ref[(leaf, mode)]
            iters = sum(x[0] for x in r)
            row = {"leaf": leaf, "mode": mode, "kept_voxels": int(kept[(leaf, mode)]), "mean_iterations": iters / a.frames,
                   "converged": sum(x[1] for x in r), "status_1": sum(x[2] == 1 for x in r), **errors(r, T)}
            ts = times[(leaf, mode, "serial")]
            for name in ["serial"] + ["voxels_%d" % s for s in SLOTS]:
                t = times[(leaf, mode, name)]
                row[name] = {"ms_min": 1e3 * min(t), "ms_max": 1e3 * max(t), "frames_per_s": a.frames / min(t), "it_per_s": iters / min(t),
                             "x_serial": min(ts) / min(t)}
            b = times[(leaf, mode, "voxels_64")]
            # the condition of the change: at 64 slots faster than the serial loop by more than the spread of either leg
            row["gain_64_ms"] = 1e3 * (min(ts) - min(b))
            row["spread_ms"] = 1e3 * max(max(ts) - min(ts), max(b) - min(b))
            row["faster_beyond_spread"] = bool(row["gain_64_ms"] > row["spread_ms"])
            out["configs"].append(row)
        # ---- the chain: the fourth engine first, the third from the poses it reached, against the third alone
        chain = {}
        alone = ctx.register_frames_gicp(frames, T0, "Ours", cfg, prm)                      # warm-up
        for _ in range(a.repeats):
            t = time.perf_counter()
            alone = ctx.register_frames_gicp(frames, T0, "Ours", cfg, prm)
            chain.setdefault("gicp_alone", []).append(time.perf_counter() - t)
            for leaf, mode in CONFIGS:
                select(leaf, mode)                                                          # (the map is kept once per map: not part of a call)
                t = time.perf_counter()
                first = batched(mode, 0)
                reached = [np.array(r.final_transform[:]).reshape(4, 4) for r in first]
                second = ctx.register_frames_gicp(frames, reached, "Ours", cfg, prm)
                chain.setdefault((leaf, mode), []).append((time.perf_counter() - t, first, second))

        def stage(recs):
            return dict(mean_iterations=sum(r.iterations for r in recs) / a.frames, converged=sum(r.converged for r in recs), **errors(recs, T))

        out["chain"] = [{"leg": "gicp_alone", "ms_min": 1e3 * min(chain["gicp_alone"]), "ms_max": 1e3 * max(chain["gicp_alone"]), **stage(alone)}]
        for leaf, mode in CONFIGS:
            runs = chain[(leaf, mode)]
            _, first, second = runs[-1]
            out["chain"].append({"leg": "voxels_then_gicp", "leaf": leaf, "mode": mode, "ms_min": 1e3 * min(r[0] for r in runs),
                                 "ms_max": 1e3 * max(r[0] for r in runs), "voxels": stage(first), "gicp": stage(second)})
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
