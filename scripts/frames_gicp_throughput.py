"""Many frames against one resident map with the third engine (plane-to-plane rows from the map's kept normals and every frame's own,
k = 5): 256 frames of 8 k points cut out of the 200 k-point parking lot (the frames and start poses of scripts/frames_throughput.py),
thresholds on, method "Ours".  Four legs, timed in the SAME loop of one process - every repeat runs all of them, one after the other, each
under its own synchronise (every call returns after its last result has been waited for) - upload included on all sides, a host clock, one
warm-up pass of each first, the best repeat:
  (a) serial          the loop dcreg_set_source + dcreg_source_normals_keep + dcreg_icp_run_gicp per frame: the only way before the
                      batched call
  (b) gicp_<slots>    dcreg_register_frames_gicp at 16 / 64 / 256 slots (the frames' normals: one batched pass inside the call)
  (c) normals_<slots> dcreg_register_frames_normals (the second engine) at the same slots: a second reference
  (d) clouds / loop   dcreg_normals_clouds of the 256 frames against the loop of dcreg_normals over them
and for each engine the mean iterations per frame, the converged frames and the final pose errors against the frames' true poses.
Asserts that every record of (b) is bitwise the serial loop's and every value of (d) the loop's.  DCREG_TRIALS_TIMING=1 adds the
engines' per-step timing on stderr.  Prints one JSON line.

usage: python scripts/frames_gicp_throughput.py [--frames 256] [--points 8000] [--repeats 3]"""
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

SLOTS = (16, 64, 256)


def serial(ctx, frames, T0, cfg, prm):
    out = []
    for f, T in zip(frames, T0):
        ctx.set_source(f)
        ctx.keep_source_normals(prm)
        res, logs = ctx.icp_run_gicp(T, "Ours", cfg)
        last = logs[-1] if logs else None
        Tf = np.eye(4)
        Tf[:3, :3] = np.array(res.R[:]).reshape(3, 3)
        Tf[:3, 3] = res.t[:]
        out.append((res.iterations, res.converged, res.status, tuple(Tf.reshape(16)), last.rmse if last else 0.0, last.fitness if last else 0.0,
                    last.effective_points if last else 0, tuple(last.H_upper[:]) if last else (0.0,) * 21,
                    tuple(last.analysis.degenerate_mask[:]) if last else (0,) * 6))
    return out


def same(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--repeats", type=int, default=3)
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
        ctx.keep_target_normals(prm)

        def normals_loop():
            return [ctx.normals(f, prm)[:2] for f in frames]

        legs = {"serial": lambda: serial(ctx, frames, T0, cfg, prm)}
        for s in SLOTS:
            legs["gicp_%d" % s] = lambda s=s: ctx.register_frames_gicp(frames, T0, "Ours", cfg, prm, slots=s)
            legs["normals_%d" % s] = lambda s=s: ctx.register_frames_normals(frames, T0, "Ours", cfg, slots=s)
        legs["normals_loop"] = normals_loop
        legs["normals_clouds"] = lambda: ctx.normals_clouds(frames, prm)
        first = {name: fn() for name, fn in legs.items()}                 # warm-up of every leg
        ref = first["serial"]
        for s in SLOTS:
            assert [record(r) for r in first["gicp_%d" % s]] == ref, "register_frames_gicp at %d slots is not the serial loop" % s
        nrm, cur, off, _ = first["normals_clouds"]
        for k, (wn, wc) in enumerate(first["normals_loop"]):
            assert same(nrm[off[k]:off[k + 1]], wn) and same(cur[off[k]:off[k + 1]], wc), "normals_clouds differs from normals at cloud %d" % k
        best = {}
        for _ in range(a.repeats):
            for name, fn in legs.items():
                t = time.perf_counter()
                got = fn()
                dt = time.perf_counter() - t
                best[name] = min(best.get(name, dt), dt)
                if name.startswith("gicp_"):
                    assert [record(r) for r in got] == ref, "%s is not the serial loop" % name
        # the frames' normals alone, as the engine takes them: the load and the batched pass behind it
        keep = []
        for _ in range(a.repeats + 1):
            ctx.frames_load(frames)
            t = time.perf_counter()
            ctx.frames_normals_keep(prm)
            keep.append(time.perf_counter() - t)
        iters = {"gicp": sum(r[0] for r in ref), "normals": sum(r.iterations for r in first["normals_256"])}
        out = {"frames": a.frames, "points": a.points, "map_points": int(len(tgt)), "bitwise_equal_to_serial": True,
               "frames_normals_keep_ms": 1e3 * min(keep[1:])}
        for name in legs:
            if name.startswith("normals_c") or name.startswith("normals_l"):
                continue
            engine = "normals" if name.startswith("normals_") else "gicp"
            out[name] = {"ms": 1e3 * best[name], "frames_per_s": a.frames / best[name], "it_per_s": iters[engine] / best[name],
                         "x_serial": best["serial"] / best[name]}
        out["normals_loop_ms"] = 1e3 * best["normals_loop"]
        out["normals_clouds_ms"] = 1e3 * best["normals_clouds"]
        out["normals_clouds_x_loop"] = best["normals_loop"] / best["normals_clouds"]
        out["gicp"] = dict(mean_iterations=iters["gicp"] / a.frames, converged=sum(r[1] for r in ref), **errors(ref, T))
        out["normals"] = dict(mean_iterations=iters["normals"] / a.frames, converged=sum(r.converged for r in first["normals_256"]),
                              **errors(first["normals_256"], T))
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
