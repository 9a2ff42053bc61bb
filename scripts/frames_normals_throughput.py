"""Many frames against one resident map with the second engine (the map's kept normals, k = 5): 256 frames of 8 k points cut out of the
200 k-point parking lot (the frames and start poses of scripts/frames_throughput.py), thresholds on, method "Ours".  Three legs, timed in
the SAME loop of one process - every repeat runs all of them, one after the other, each under its own synchronise (every call returns
after its last result has been waited for) - upload included on all sides, a host clock, one warm-up pass of each first, the best repeat:
  (a) serial          the loop dcreg_set_source + dcreg_icp_run_normals per frame: the only way to do this before the batched call
  (b) normals_<slots> dcreg_register_frames_normals at 16 / 64 / 256 slots
  (c) plane_<slots>   dcreg_register_frames (the first engine) at the same slots: a second reference
and for each engine the mean iterations per frame, the converged frames and the final pose errors against the frames' true poses.
Also checks that every record of (b) is bitwise the serial loop's.  DCREG_TRIALS_TIMING=1 adds the engines' per-step timing on stderr.
Prints one JSON line.

usage: python scripts/frames_normals_throughput.py [--frames 256] [--points 8000] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402
from frames_throughput import frame_poses, record  # noqa: E402

SLOTS = (16, 64, 256)


def serial(ctx, frames, T0, cfg):
    out = []
    for f, T in zip(frames, T0):
        ctx.set_source(f)
        res, logs = ctx.icp_run_normals(T, "Ours", cfg)
        last = logs[-1] if logs else None
        Tf = np.eye(4)
        Tf[:3, :3] = np.array(res.R[:]).reshape(3, 3)
        Tf[:3, 3] = res.t[:]
        out.append((res.iterations, res.converged, res.status, tuple(Tf.reshape(16)), last.rmse if last else 0.0, last.fitness if last else 0.0,
                    last.effective_points if last else 0, tuple(last.H_upper[:]) if last else (0.0,) * 21,
                    tuple(last.analysis.degenerate_mask[:]) if last else (0,) * 6))
    return out


def errors(recs, truth):
    """mean / max pose error of the records' final transforms against the frames' true poses"""
    te, re_ = [], []
    for r, T in zip(recs, truth):
        a, b = api.pose_error(T, np.array(r[3] if isinstance(r, tuple) else r.final_transform[:]).reshape(4, 4))
        te.append(a); re_.append(b)
    return {"trans_err_m_mean": float(np.mean(te)), "trans_err_m_max": float(np.max(te)), "rot_err_deg_mean": float(np.mean(re_)),
            "rot_err_deg_max": float(np.max(re_))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    tgt, _ = scenes.scene_parkinglot()
    gt, T, T0 = frame_poses(a.frames, 5, 6.0)
    frames = scenes.map_frames(tgt, T, a.points, seed=3)
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1, gt_matrix=gt.reshape(16))
    ctx = api.Context(0)
    try:
        ctx.set_target(tgt, 0.5)
        t = time.perf_counter()
        ctx.keep_target_normals(api.normal_params(k=5))
        keep_ms = 1e3 * (time.perf_counter() - t)
        legs = {"serial": lambda: serial(ctx, frames, T0, cfg)}
        for s in SLOTS:
            legs["normals_%d" % s] = lambda s=s: ctx.register_frames_normals(frames, T0, "Ours", cfg, slots=s)
            legs["plane_%d" % s] = lambda s=s: ctx.register_frames(frames, T0, "Ours", cfg, slots=s)
        first = {name: fn() for name, fn in legs.items()}                 # warm-up of every leg
        ref = first["serial"]
        bitwise = all([record(r) for r in first["normals_%d" % s]] == ref for s in SLOTS)
        best = {}
        for _ in range(a.repeats):
            for name, fn in legs.items():
                t = time.perf_counter()
                got = fn()
                dt = time.perf_counter() - t
                best[name] = min(best.get(name, dt), dt)
                if name.startswith("normals_"):
                    bitwise &= [record(r) for r in got] == ref
        iters = {"normals": sum(r[0] for r in ref), "plane": sum(r.iterations for r in first["plane_256"])}
        out = {"frames": a.frames, "points": a.points, "map_points": int(len(tgt)), "keep_normals_ms": keep_ms, "bitwise_equal_to_serial": bool(bitwise)}
        for name in legs:
            engine = "plane" if name.startswith("plane_") else "normals"
            out[name] = {"ms": 1e3 * best[name], "frames_per_s": a.frames / best[name], "it_per_s": iters[engine] / best[name],
                         "x_serial": best["serial"] / best[name]}
        out["normals"] = dict(mean_iterations=iters["normals"] / a.frames, converged=sum(r[1] for r in ref), **errors(ref, T))
        out["plane"] = dict(mean_iterations=iters["plane"] / a.frames, converged=sum(r.converged for r in first["plane_256"]),
                            **errors(first["plane_256"], T))
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
