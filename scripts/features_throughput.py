"""FPFH descriptors and feature-space matching on the device against the host.  A host clock around calls that end in a synchronise, after
warm-up; medians.  Every device leg runs beside its CPU comparison in the same loop on the same box: scipy.spatial.cKDTree for the
neighbours (workers = -1) and for the search in feature space, the pair features and histograms in numpy - PCL's definition in double,
not this library's rounding.
  (a) descriptors, normals given: an 8 k-point frame, a 131 k-point organised sweep (scenes.lidar_sweep over the 200 k-point parking-lot
      map) and the 200 k-point map as a cloud, k = 16; and target_fpfh() of the map from its kept normals (no upload, no build);
  (b) descriptors with the normals estimated inside the call (normal k = 10) for the same three clouds;
  (c) matching: 8 k x 8 k and 8 k x 200 k rows, with the second-best and the mutual flags; the comparison is cKDTree.query(k = 2) in 33
      dimensions and a second query the other way round for the mutual flags;
  (d) the far-started pairs of DESIGN.md section 24 (submap pairs, frames of --points points against submaps of --submap): descriptors of
      both sides, the source matched against the target, and the share of the mutual matches whose target point lies within 0.5 m of the
      source point moved by the true pose - for the clouds as they are (k = 16) and for both sides thinned by the voxel grid at --leaf
      first (k = 32: equal density on both sides).  Normals of both sides are oriented upwards (a viewpoint 1 km above the cloud).
Prints one JSON line.

usage: python scripts/features_throughput.py [--repeats 5] [--pairs 16] [--points 8000] [--submap 50000] [--leaf 0.5] [--skip d]"""
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


def scipy_fpfh(pts, nrm, k, chunk=1 << 16):
    """PCL's FPFHEstimation with a k search, vectorised: -> [n, 33] float32"""
    from scipy.spatial import cKDTree
    p, n = pts.astype(np.float64), nrm.astype(np.float64)
    dist, idx = cKDTree(p).query(p, k, workers=-1)
    spfh = np.zeros((len(p), 33))
    for s in range(0, len(p), chunk):
        j = idx[s:s + chunk, 1:]
        d = p[j] - p[s:s + chunk, None, :]
        f4 = np.maximum(np.linalg.norm(d, axis=2), 1e-300)
        npp = np.broadcast_to(n[s:s + chunk, None, :], d.shape)
        nq = n[j]
        a1, a2 = np.sum(npp * d, axis=2) / f4, np.sum(nq * d, axis=2) / f4
        sw = np.abs(a1) < np.abs(a2)
        n1, n2 = np.where(sw[..., None], nq, npp), np.where(sw[..., None], npp, nq)
        d = np.where(sw[..., None], -d, d)
        phi = np.where(sw, -a2, a1)
        v = np.cross(d, n1)
        v /= np.maximum(np.linalg.norm(v, axis=2, keepdims=True), 1e-300)
        w = np.cross(n1, v)
        alpha = np.sum(v * n2, axis=2)
        theta = np.arctan2(np.sum(w * n2, axis=2), np.sum(n1 * n2, axis=2))
        rows = np.broadcast_to(np.arange(s, s + len(j))[:, None], j.shape)
        for blk, x in enumerate(((theta + np.pi) / (2 * np.pi), (alpha + 1) * 0.5, (phi + 1) * 0.5)):
            np.add.at(spfh, (rows, 11 * blk + np.clip(np.floor(11 * x), 0, 10).astype(np.int64)), 100.0 / (k - 1))
    out = np.zeros((len(p), 33))
    wgt = 1.0 / np.maximum(dist[:, 1:] ** 2, 1e-300)
    for s in range(0, len(p), chunk):
        out[s:s + chunk] = np.einsum("nk,nkb->nb", wgt[s:s + chunk], spfh[idx[s:s + chunk, 1:]])
    blocks = out.reshape(-1, 3, 11)
    blocks *= 100.0 / np.maximum(blocks.sum(axis=2, keepdims=True), 1e-300)
    return out.astype(np.float32)


def scipy_match(a, b):
    """-> (idx, idx2, mutual) by two cKDTree queries in 33 dimensions"""
    from scipy.spatial import cKDTree
    _, ij = cKDTree(b).query(a, 2, workers=-1)
    _, back = cKDTree(a).query(b, 1, workers=-1)
    return ij[:, 0], ij[:, 1], back[ij[:, 0]] == np.arange(len(a))


def up(cloud):
    c = cloud[np.isfinite(cloud).all(axis=1)].mean(axis=0)
    return (float(c[0]), float(c[1]), float(c[2]) + 1000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--points", type=int, default=8000)
    ap.add_argument("--submap", type=int, default=50000)
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    out = {}
    ctx = api.Context(0)
    tgt, frame = scenes.scene_parkinglot()
    gt = scenes.pose6d_matrix(**scenes.PK01_GT)
    sweep = scenes.lidar_sweep(tgt, gt, seed=1)
    sweep = np.ascontiguousarray(sweep[np.isfinite(sweep[:, :3]).all(axis=1), :3])
    clouds = {"frame_8k": frame, "sweep_131k": sweep, "map_200k": tgt}
    p, npar = api.fpfh_params(k=16), api.normal_params(k=10)
    desc = {}
    for tag, cloud in clouds.items():
        out["%s_points" % tag] = len(cloud)
        nrm = ctx.normals(cloud, npar)[0]
        if "a" not in a.skip:
            res = {}

            def run():
                res["f"], _, res["i"] = ctx.fpfh(cloud, nrm, params=p)
            out["a_%s_fpfh_ms" % tag] = timed(run, a.repeats, warmup=2)
            out["a_%s_n_out" % tag] = int(res["i"]["n_out"])
            desc[tag] = res["f"]
            host = {}

            def cpu():
                host["f"] = scipy_fpfh(cloud, nrm, 16)
            out["a_%s_scipy_numpy_ms" % tag] = timed(cpu, 1, warmup=0)
            ok = ~np.isnan(res["f"][:, 0])
            out["a_%s_max_diff_to_scipy" % tag] = float(np.abs(res["f"][ok] - host["f"][ok]).max())
        if "b" not in a.skip:
            out["b_%s_fpfh_with_normals_ms" % tag] = timed(lambda: ctx.fpfh(cloud, None, npar, p), a.repeats, warmup=2)
    if "a" not in a.skip:
        ctx.set_target(tgt, 0.5)
        ctx.keep_target_normals(npar)
        out["a_map_200k_target_fpfh_ms"] = timed(lambda: ctx.target_fpfh(p), a.repeats, warmup=2)
    if "c" not in a.skip and desc:
        fa, fm = desc["frame_8k"], desc["map_200k"]
        fa, fm = np.ascontiguousarray(fa[~np.isnan(fa[:, 0])]), np.ascontiguousarray(fm[~np.isnan(fm[:, 0])])
        rng = np.random.default_rng(2)
        fb = np.ascontiguousarray(fm[rng.choice(len(fm), len(fa), replace=False)])
        for tag, b in (("8k_x_8k", fb), ("8k_x_200k", fm)):
            res, host = {}, {}

            def run():
                res["m"] = ctx.feature_match(fa, b)

            def cpu():
                host["m"] = scipy_match(fa, b)
            out["c_%s_match_ms" % tag] = timed(run, a.repeats, warmup=2)
            out["c_%s_match_no_mutual_ms" % tag] = timed(lambda: ctx.feature_match(fa, b, want_mutual=False), a.repeats, warmup=1)
            out["c_%s_scipy_ms" % tag] = timed(cpu, 1, warmup=0)
            out["c_%s_pairs" % tag] = int(len(fa)) * int(len(b))
            out["c_%s_same_best_as_scipy" % tag] = float(np.mean(res["m"]["idx"] == host["m"][0]))      # (ties: scipy's choice among equal rows is its own)
            out["c_%s_mutual" % tag] = int(res["m"]["n_mutual"])
    if "d" not in a.skip:
        rng = np.random.default_rng(5)
        poses = [gt @ scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.0, 0.0, 0.0, np.deg2rad(rng.uniform(-20, 20))) for _ in range(a.pairs)]
        srcs, tgts, Tt = scenes.scan_pairs(tgt, poses, a.points, seed=3, mode="submap", n_submap=a.submap, submap_radius=45.0)
        # raw: the clouds as they are, k = 16 - a frame of 8 k points and a submap several times as dense, so the k nearest points span
        # different supports on the two sides; thinned: both sides through the voxel grid at --leaf first, k = 32 - equal density, the
        # usual preparation for FPFH
        for tag, leaf, kk in (("raw", 0.0, 16), ("thinned", a.leaf, 32)):
            shares, mutuals, ms, sizes = [], [], [], []
            pk = api.fpfh_params(k=kk)
            for s, t, T in zip(srcs, tgts, Tt):
                t0 = time.perf_counter()
                if leaf > 0.0:
                    (s, t), _ = ctx.voxel_downsample([s, t], leaf)
                fs = ctx.fpfh(s, None, api.normal_params(k=10, viewpoint=up(s)), pk)[0]
                ft = ctx.fpfh(t, None, api.normal_params(k=10, viewpoint=up(t)), pk)[0]
                m = ctx.feature_match(fs, ft)
                ms.append((time.perf_counter() - t0) * 1e3)
                mu = np.flatnonzero(m["mutual"])
                moved = s[mu].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
                err = np.linalg.norm(moved - t[m["idx"][mu]].astype(np.float64), axis=1)
                shares.append(float(np.mean(err < 0.5)) if len(mu) else 0.0)
                mutuals.append(int(len(mu)))
                sizes.append([len(s), len(t)])
            out["d_%s_k" % tag] = kk
            out["d_%s_points_median" % tag] = [float(x) for x in np.median(np.array(sizes), axis=0)]
            out["d_%s_ms_per_pair_median" % tag] = float(np.median(ms))
            out["d_%s_mutual_matches_median" % tag] = float(np.median(mutuals))
            out["d_%s_share_within_0.5m_median" % tag] = float(np.median(shares))
            out["d_%s_share_within_0.5m_min_max" % tag] = [float(np.min(shares)), float(np.max(shares))]
        out["d_pairs"] = a.pairs
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
