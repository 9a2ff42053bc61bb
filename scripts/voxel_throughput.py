"""Voxel-grid downsampling on the device against the host.  A host clock around calls that end in a synchronise, after warm-up; medians.
  (a) one 131 k-point organised sweep (scenes.lidar_sweep over the 200 k-point parking-lot map, NaN where a beam has no return):
      set_source_voxel + icp_run, against the numpy reference downsample (the header's rules, vectorised) + set_source + icp_run;
  (b) --sweeps sweeps through ONE batched voxel_downsample, then register_frames of its output;
  (c) set_target_voxel of a --map-points prior map (scenes.scene_prior_map), against set_target of the same map downsampled beforehand.
Checks that (a) gives bitwise the same pose both ways and that (c)'s maps are bitwise the same.  Prints one JSON line.

usage: python scripts/voxel_throughput.py [--leaf 0.2] [--map-leaf 0.1] [--sweeps 256] [--map-points 50000000] [--repeats 10] [--skip c]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402


def voxel_reference(xyz, leaf):
    """the centroid rule of include/dcreg.h in numpy: finite points, floor((double)p / leaf), (z, y, x) order, sequential double sums"""
    p = np.asarray(xyz, np.float32)[:, :3]
    idx = np.flatnonzero(np.all(np.isfinite(p), 1))
    v = np.floor(p[idx].astype(np.float64) / leaf).astype(np.int64)
    order = np.lexsort((idx, v[:, 0], v[:, 1], v[:, 2]))
    vs, ids = v[order], idx[order]
    starts = np.flatnonzero(np.r_[True, np.any(vs[1:] != vs[:-1], 1)])
    counts = np.diff(np.r_[starts, len(ids)])
    s = p[ids[starts]].astype(np.float64)
    for k in range(1, int(counts.max())):
        m = counts > k
        s[m] += p[ids[starts[m] + k]].astype(np.float64)
    return (s / counts[:, None]).astype(np.float32)


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaf", type=float, default=0.2)
    ap.add_argument("--map-leaf", type=float, default=0.1)
    ap.add_argument("--sweeps", type=int, default=256)
    ap.add_argument("--map-points", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip", default="")
    ap.add_argument("--only-a", action="store_true", help="run (a) alone, a few times (the profiled run)")
    a = ap.parse_args()
    out = {"leaf": a.leaf}
    tgt, _ = scenes.scene_parkinglot()
    gt, T0 = scenes.pose6d_matrix(**scenes.PK01_GT), scenes.pose6d_matrix(**scenes.PK01_INIT)
    cfg = api.default_config(search_radius=1.0, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, use_weight_derivative=1,
                             always_compute_schur=1)
    ctx = api.Context(0)
    ctx.set_target(tgt, 1.0)
    sweep = scenes.lidar_sweep(tgt, gt, seed=1)
    out["sweep_points"], out["sweep_returns"] = len(sweep), int(np.isfinite(sweep[:, 0]).sum())
    if "a" not in a.skip:
        def dev():
            ctx.set_source_voxel(sweep, a.leaf)
            return ctx.icp_run(T0, "Ours", cfg)[0]

        def host():
            ctx.set_source(voxel_reference(sweep, a.leaf))
            return ctx.icp_run(T0, "Ours", cfg)[0]
        rd, rh = dev(), host()
        assert tuple(rd.R[:]) == tuple(rh.R[:]) and tuple(rd.t[:]) == tuple(rh.t[:]) and rd.iterations == rh.iterations
        out["a_voxel_points"] = ctx.index_info().n_source
        out["a_iterations"] = rd.iterations
        out["a_device_ms"] = timed(dev, a.repeats)
        out["a_host_ms"] = timed(host, a.repeats)
        out["a_voxel_only_device_ms"] = timed(lambda: ctx.set_source_voxel(sweep, a.leaf), a.repeats)
        out["a_numpy_downsample_ms"] = timed(lambda: voxel_reference(sweep, a.leaf), a.repeats)
        out["a_icp_only_ms"] = timed(lambda: ctx.icp_run(T0, "Ours", cfg), a.repeats)
        if a.only_a:
            print(json.dumps(out), flush=True)
            return
    if "b" not in a.skip:
        rng = np.random.default_rng(2)
        poses, starts = [], []
        for k in range(a.sweeps):
            Tk = gt @ scenes.pose6d_matrix(rng.uniform(-4, 4), rng.uniform(-4, 4), 0.0, 0.0, 0.0, np.radians(rng.uniform(-20, 20)))
            poses.append(Tk)
            starts.append(Tk @ scenes.pose6d_matrix(*rng.uniform(-0.1, 0.1, 3), *np.radians(rng.uniform(-0.5, 0.5, 3))))
        # 256 sweeps of 131 k points: 32 distinct sweeps repeated (generating each is host work that is not measured)
        base = [scenes.lidar_sweep(tgt, poses[k], seed=k) for k in range(min(32, a.sweeps))]
        sweeps = [base[k % len(base)] for k in range(a.sweeps)]
        xyz = np.concatenate(sweeps)
        off = np.r_[0, np.cumsum([len(s) for s in sweeps])]
        res = {}

        def batch():
            res["v"] = ctx.voxel_downsample((xyz, off), a.leaf)
        out["b_points_in"] = int(len(xyz))
        out["b_voxel_ms"] = timed(batch, max(3, a.repeats // 3), warmup=1)
        (vx, voff), info = res["v"]
        out["b_points_out"] = int(info["n_out"])
        T0s = np.stack([starts[k % len(base)] for k in range(a.sweeps)])
        out["b_register_frames_ms"] = timed(lambda: ctx.register_frames((vx, voff), T0s, "Ours", cfg), max(3, a.repeats // 3), warmup=1)
        out["b_total_ms"] = out["b_voxel_ms"] + out["b_register_frames_ms"]
    if "c" not in a.skip:
        big, _ = scenes.scene_prior_map(a.map_points)
        (pre, _), info = ctx.voxel_downsample((big, [0, len(big)]), a.map_leaf)
        out["c_map_points"], out["c_map_out"] = len(big), int(info["n_out"])
        c2 = api.Context(0)
        r = max(3, a.repeats // 3)
        out["c_set_target_voxel_ms"] = timed(lambda: ctx.set_target_voxel(big, 1.0, a.map_leaf), r, warmup=1)
        out["c_set_target_predownsampled_ms"] = timed(lambda: c2.set_target(pre, 1.0), r, warmup=1)
        out["c_voxel_downsample_only_ms"] = timed(lambda: ctx.voxel_downsample((big, [0, len(big)]), a.map_leaf), r, warmup=1)
        got = ctx.target_points()
        want = c2.target_points()
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        c2.close()
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
