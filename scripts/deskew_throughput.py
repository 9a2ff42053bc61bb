"""Motion compensation (deskew) on the device against the host.  A host clock around calls that end in a synchronise, after warm-up; medians.
  (a) one 128 x 1024 moving sweep (scenes.lidar_sweep_moving over the 200 k-point parking-lot map, 10 m/s and 0.5 rad/s over 0.1 s, records
      x y z stamp): set_source_deskew with a --leaf voxel, against set_source_voxel of the same records (no deskew), and against the deskew
      in numpy (vectorised, the header's rule) + set_source_voxel;
  (b) --sweeps such sweeps through ONE deskew call with a voxel block, against voxel_downsample alone of the same records;
  (c) --pack-only: set_source_deskew, set_source_deskew_path without a voxel block and set_source of the same finite records, --repeats times
      each - run it under `rocprofv3 --kernel-trace --stats` to compare the kernel times of k_pack_deskew, k_pack_deskew_path and k_pack on
      the same records.
Beside each constant-twist leg its path leg (set_source_deskew_path / deskew_path): the same sweeps, the same motion sampled at 400 Hz as a
41-knot table per sweep (and the --sweeps call once more with one table shared by all), the two forms clocked alternately in one loop.
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


def numpy_deskew_path(rec, st, P, t_ref):
    """the header's path rule (identity extrinsic) for f32 stamps in column 3, vectorised on the host: per point its segment, Exp(u xi_k),
    then G_k -> [n, 3] float32"""
    T = np.tile(np.eye(4), (len(st), 1, 1))
    T[:, :3, :3], T[:, :3, 3] = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    xi = np.array([api.se3_log(np.linalg.inv(T[k]) @ T[k + 1]) for k in range(len(st) - 1)])
    kr = int(np.clip(np.searchsorted(st, t_ref, side="right") - 1, 0, len(st) - 2))
    Bref = T[kr] @ api.se3_exp((t_ref - st[kr]) / (st[kr + 1] - st[kr]) * xi[kr])
    G = np.linalg.inv(Bref)[None] @ T[:-1]
    s = rec[:, 3].astype(np.float64)
    k = np.clip(np.searchsorted(st, s, side="right") - 1, 0, len(st) - 2)
    R, t = scenes._se3_exp_many(((s - st[k]) / (st[k + 1] - st[k]))[:, None] * xi[k])
    q = np.einsum("nij,nj->ni", R, rec[:, :3].astype(np.float64)) + t
    return (np.einsum("nij,nj->ni", G[k, :3, :3], q) + G[k, :3, 3]).astype(np.float32)


def clock_pair(fa, fb, repeats):
    """the two calls alternately in one loop, after a warm-up of each -> their medians in ms"""
    fa()
    fb()
    ta, tb = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fa()
        t1 = time.perf_counter()
        fb()
        ta.append(t1 - t0)
        tb.append(time.perf_counter() - t1)
    return float(np.median(ta)) * 1e3, float(np.median(tb)) * 1e3


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
    xi = api.se3_log(M)
    st = np.arange(41) / 400.0                                 # the same motion as a table: the sensor's own poses at 400 Hz
    P = np.array([np.r_[T[:3, :3].reshape(9), T[:3, 3]] for T in (gt @ api.se3_exp(k / 40.0 * xi) for k in range(41))])
    path = api.sweep_path(0, 41, 0.5 * period)
    ctx = api.Context(0)
    out = {"points": len(rec), "leaf": a.leaf}
    if a.pack_only:
        fin = np.ascontiguousarray(rec[np.all(np.isfinite(rec[:, :3]), 1)])
        for _ in range(a.repeats):
            ctx.set_source_deskew(fin, f, m)
            ctx.set_source_deskew_path(fin, f, st, P, path)
            ctx.set_source(fin)
        out.update(pack_only=True, finite_points=len(fin), record_bytes=16)
        print(json.dumps(out))
        return
    out["a_set_source_deskew_voxel_ms"] = clock(lambda: ctx.set_source_deskew(rec, f, m, a.leaf), a.repeats)
    out["a_pair_set_source_deskew_voxel_ms"], out["a_pair_set_source_deskew_path_voxel_ms"] = clock_pair(
        lambda: ctx.set_source_deskew(rec, f, m, a.leaf), lambda: ctx.set_source_deskew_path(rec, f, st, P, path, a.leaf), a.repeats)
    # host only: what the binding spends checking its arguments before the library is reached (one motion; a 41-knot table and its block)
    out["a_binding_checks_motion_ms"] = clock(lambda: api._motions(m, 1, "checks"), a.repeats)
    out["a_binding_checks_path_ms"] = clock(lambda: api._paths(path, 1, *api._knot_table(st, P, "checks"), "checks"), a.repeats)
    out["a_numpy_deskew_path_plus_set_source_voxel_ms"] = clock(lambda: ctx.set_source_voxel(
        np.ascontiguousarray(np.c_[numpy_deskew_path(rec, st, P, 0.5 * period), rec[:, 3:]]), a.leaf), max(3, a.repeats // 4))
    ctx.set_source_deskew_path(rec, f, st, P, path, a.leaf)
    n_dev = ctx.index_info().n_source
    ctx.set_source_voxel(np.ascontiguousarray(numpy_deskew_path(rec, st, P, 0.5 * period)), a.leaf)
    out["a_path_sources_points_device_numpy"] = [int(n_dev), int(ctx.index_info().n_source)]
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
    st_all, P_all = np.tile(st, a.sweeps), np.tile(P, (a.sweeps, 1))                 # a table per sweep, and one shared by all
    own = [api.sweep_path(41 * k, 41, 0.5 * period) for k in range(a.sweeps)]
    out["b_pair_deskew_voxel_ms"], out["b_pair_deskew_path_voxel_ms"] = clock_pair(
        lambda: ctx.deskew((allr, off), f, m, a.leaf), lambda: ctx.deskew_path((allr, off), f, st_all, P_all, own, a.leaf), max(3, a.repeats // 4))
    out["b_deskew_path_shared_table_voxel_ms"] = clock(lambda: ctx.deskew_path((allr, off), f, st, P, path, a.leaf), max(3, a.repeats // 4))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
