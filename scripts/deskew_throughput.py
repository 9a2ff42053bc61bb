"""Motion compensation (deskew) on the device against the host.  A host clock around calls that end in a synchronise, after warm-up; medians.
  (a) one 128 x 1024 moving sweep (scenes.lidar_sweep_moving over the 200 k-point parking-lot map, 10 m/s and 0.5 rad/s over 0.1 s, records
      x y z stamp): set_source_deskew with a --leaf voxel, against set_source_voxel of the same records (no deskew), and against the deskew
      in numpy (vectorised, the header's rule) + set_source_voxel;
  (b) --sweeps such sweeps through ONE deskew call with a voxel block, against voxel_downsample alone of the same records;
  (c) --pack-only: set_source_deskew without a voxel block and set_source of the same finite records, --repeats times each - run it under
      `rocprofv3 --kernel-trace --stats` to compare the kernel time of k_pack_deskew with k_pack on the same records.
Prints one JSON line.

usage: python scripts/deskew_throughput.py [--leaf 0.2] [--sweeps 256] [--repeats 20] [--pack-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402


def numpy_deskew(rec, M, span, ref):
    """the header's rule for f32 stamps in column 3, vectorised on the host -> [n, 3] float32 (NaN rows stay NaN)"""
    xi = api.se3_log(M)
    s = rec[:, 3].astype(np.float64)
    a = (s - span[0]) / (span[1] - span[0]) - ref
    R, t = scenes._se3_exp_many(np.outer(a, xi))
    return (np.einsum("nij,nj->ni", R, rec[:, :3].astype(np.float64)) + t).astype(np.float32)


def clock(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaf", type=float, default=0.2)
    ap.add_argument("--sweeps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--pack-only", action="store_true")
    a = ap.parse_args()
    tgt, _ = scenes.scene_parkinglot()
    gt = scenes.pose6d_matrix(**scenes.PK01_GT)
    period = 0.1
    M = api.se3_exp([0.0, 0.0, 0.5 * period, 10.0 * period, 0.0, 0.0])
    rec, _ = scenes.lidar_sweep_moving(tgt, gt, M, period, seed=1)
    f = api.time_field(3)
    m = api.sweep_motion(M[:3, :3], M[:3, 3], (0.0, period), 0.5)
    ctx = api.Context(0)
    out = {"points": len(rec), "leaf": a.leaf}
    if a.pack_only:
        fin = np.ascontiguousarray(rec[np.all(np.isfinite(rec[:, :3]), 1)])
        for _ in range(a.repeats):
            ctx.set_source_deskew(fin, f, m)
            ctx.set_source(fin)
        out.update(pack_only=True, finite_points=len(fin), record_bytes=16)
        print(json.dumps(out))
        return
    out["a_set_source_deskew_voxel_ms"] = clock(lambda: ctx.set_source_deskew(rec, f, m, a.leaf), a.repeats)
    out["a_set_source_voxel_ms"] = clock(lambda: ctx.set_source_voxel(rec, a.leaf), a.repeats)
    out["a_numpy_deskew_plus_set_source_voxel_ms"] = clock(lambda: ctx.set_source_voxel(
        np.ascontiguousarray(np.c_[numpy_deskew(rec, M, (0.0, period), 0.5), rec[:, 3:]]), a.leaf), max(3, a.repeats // 4))
    out["a_numpy_deskew_ms"] = clock(lambda: numpy_deskew(rec, M, (0.0, period), 0.5), max(3, a.repeats // 4))
    # the numpy path gives the device's points to an ulp: the thinned sources agree in size
    ctx.set_source_deskew(rec, f, m, a.leaf)
    n_dev = ctx.index_info().n_source
    ctx.set_source_voxel(np.ascontiguousarray(numpy_deskew(rec, M, (0.0, period), 0.5)), a.leaf)
    out["a_sources_points_device_numpy"] = [int(n_dev), int(ctx.index_info().n_source)]
    recs = [rec] * a.sweeps
    allr = np.ascontiguousarray(np.concatenate(recs))
    off = np.arange(a.sweeps + 1, dtype=np.int64) * len(rec)
    out["b_sweeps"] = a.sweeps
    out["b_deskew_voxel_ms"] = clock(lambda: ctx.deskew((allr, off), f, m, a.leaf), max(3, a.repeats // 4))
    out["b_voxel_downsample_ms"] = clock(lambda: ctx.voxel_downsample((allr, off), a.leaf), max(3, a.repeats // 4))
    out["b_overhead_pct"] = 100.0 * (out["b_deskew_voxel_ms"] / out["b_voxel_downsample_ms"] - 1.0)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
