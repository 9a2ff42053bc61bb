"""Outlier removal on the device against the host.  A host clock around calls that end in a synchronise, after warm-up; medians.
  (a) one 131 k-point organised sweep (scenes.lidar_sweep over the 200 k-point parking-lot map): set_source_outliers with a voxel block
      (voxel -> statistical filter -> source), beside set_source_voxel alone;
  (b) the statistical filter on --cloud-points clouds (scenes.scene_prior_map) at k = 8 and 16, unbounded and with --search-radius, and the
      radius filter on the same clouds;
  (c) remove_outliers on --map-points maps beside crop's time (a crop that drops a comparable number of points);
  (d) the CPU comparison: the same rule with scipy.spatial.cKDTree (k + 1 neighbours, workers = -1) plus the upload (set_target of the result).
Checks that (a) leaves the source bitwise as set_source of the filter's output.  Prints one JSON line.

usage: python scripts/outliers_throughput.py [--cloud-points 1000000,10000000] [--map-points 1000000,10000000,50000000] [--repeats 5]
                                             [--search-radius 1.0] [--radius 0.5] [--skip d]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def scipy_statistical(pts, k, std_mul):
    from scipy.spatial import cKDTree
    p = pts.astype(np.float64)
    d, _ = cKDTree(p).query(p, k + 1, workers=-1)
    m = d[:, 1:].mean(axis=1)
    return pts[m <= m.mean() + std_mul * m.std(ddof=1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud-points", default="1000000,10000000")
    ap.add_argument("--map-points", default="1000000,10000000,50000000")
    ap.add_argument("--leaf", type=float, default=0.2)
    ap.add_argument("--search-radius", type=float, default=1.0)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    out = {}
    ctx = api.Context(0)
    if "a" not in a.skip:
        tgt, _ = scenes.scene_parkinglot()
        gt = scenes.pose6d_matrix(**scenes.PK01_GT)
        sweep = scenes.lidar_sweep(tgt, gt, seed=1)
        p = api.outlier_params(k=8, std_mul=2.0)
        ctx.set_target(tgt, 1.0)
        info, vinfo = ctx.set_source_outliers(sweep, p, leaf=a.leaf)
        prm = api.default_lin_params(1.0, 1)
        got = ctx.linearize(gt[:3, :3], gt[:3, 3], prm)
        ctx.set_source(ctx.outlier_filter(ctx.voxel_downsample([sweep], a.leaf)[0][0], p)[0])
        want = ctx.linearize(gt[:3, :3], gt[:3, 3], prm)
        assert np.array_equal(got["H_upper"], want["H_upper"]) and got["n_eff"] == want["n_eff"]
        out.update(a_sweep_points=len(sweep), a_voxel_points=int(vinfo["n_out"]), a_kept=int(info["n_out"]))
        out["a_voxel_filter_source_ms"] = timed(lambda: ctx.set_source_outliers(sweep, p, leaf=a.leaf), a.repeats * 2, warmup=2)
        out["a_voxel_source_ms"] = timed(lambda: ctx.set_source_voxel(sweep, a.leaf), a.repeats * 2, warmup=2)
    if "b" not in a.skip:
        for n in [int(x) for x in a.cloud_points.split(",") if x]:
            cloud, _ = scenes.scene_prior_map(n, extent=350.0 * (n / 50e6) ** 0.5)      # (the density of the 50 M-point map)
            tag = "b_%dM" % (n // 1_000_000) if n >= 1_000_000 else "b_%d" % n
            for k in (8, 16):
                for sr in (0.0, a.search_radius):
                    p = api.outlier_params(k=k, std_mul=2.0, search_radius=sr)
                    res = {}

                    def run():
                        res["i"] = ctx.outlier_filter(cloud, p, want_mask=False, want_scores=False)[3]
                    out["%s_k%d_%s_ms" % (tag, k, "bounded" if sr else "unbounded")] = timed(run, a.repeats)
                    out["%s_k%d_%s_removed" % (tag, k, "bounded" if sr else "unbounded")] = int(res["i"]["n_in"] - res["i"]["n_out"])
            p = api.outlier_params("radius", radius=a.radius, min_neighbors=3)
            out["%s_radius_ms" % tag] = timed(lambda: ctx.outlier_filter(cloud, p, want_mask=False, want_scores=False), a.repeats)
            if "d" not in a.skip and n <= 10_000_000:
                c2 = api.Context(0)
                out["%s_scipy_k8_plus_upload_ms" % tag] = timed(lambda: c2.set_target(scipy_statistical(cloud, 8, 2.0), 1.0), 1, warmup=0)
                c2.close()
    if "c" not in a.skip:
        for n in [int(x) for x in a.map_points.split(",") if x]:
            big, _ = scenes.scene_prior_map(n, extent=350.0 * (n / 50e6) ** 0.5)
            tag = "c_%dM" % (n // 1_000_000) if n >= 1_000_000 else "c_%d" % n
            p = api.outlier_params(k=8, std_mul=2.0, search_radius=a.search_radius)
            ts, tc, removed = [], [], 0
            lo, hi = big.min(0).astype(np.float64), big.max(0).astype(np.float64)
            for _ in range(max(2, a.repeats // 2)):
                ctx.set_target(big, 1.0)
                t0 = time.perf_counter()
                info = ctx.remove_outliers(p)
                ts.append((time.perf_counter() - t0) * 1e3)
                removed = int(info["n_in"] - info["n_out"])
                ctx.set_target(big, 1.0)
                cut = lo + (hi - lo) * [0.02, 0.0, 0.0]
                t0 = time.perf_counter()
                ctx.crop(cut, hi)
                tc.append((time.perf_counter() - t0) * 1e3)
            out["%s_remove_outliers_ms" % tag], out["%s_removed" % tag], out["%s_crop_ms" % tag] = float(np.median(ts)), removed, float(np.median(tc))
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
