"""Surface normals on the device against the host.  A host clock around calls that end in a synchronise, after warm-up; medians.
  (a) one 131 k-point organised sweep (scenes.lidar_sweep over the 200 k-point parking-lot map): normals() at k = 5 and 16;
  (b) normals() of --cloud-points clouds (scenes.scene_prior_map) at k = 5 and 16, unbounded and with --search-radius;
  (c) target_normals() of --map-points maps at k = 5 and 16 (the map's own index: no upload, no build);
  (d) the CPU comparison in the same loop on the same box: scipy.spatial.cKDTree (k neighbours, workers = -1), the covariances in numpy,
      batched numpy.linalg.eigh - PCL's definition in double, not this library's rounding - for (a), and for (b) up to 10 M points.
Checks on (a) that the device's normals lie within 1e-5 rad of the comparison's wherever the two smallest eigenvalues are apart.
Prints one JSON line.

usage: python scripts/normals_throughput.py [--cloud-points 1000000,10000000] [--map-points 50000000] [--repeats 5] [--search-radius 1.0]
                                            [--skip d]"""
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


def scipy_normals(pts, k, chunk=1 << 20):
    """-> (normals [n, 3] float64 towards the origin, eigenvalues [n, 3] ascending)"""
    from scipy.spatial import cKDTree
    p = pts.astype(np.float64)
    _, idx = cKDTree(p).query(p, k, workers=-1)
    nrm, lam = np.empty((len(p), 3)), np.empty((len(p), 3))
    for s in range(0, len(p), chunk):
        q = p[idx[s:s + chunk]]
        d = q - q.mean(axis=1, keepdims=True)
        w, v = np.linalg.eigh(np.einsum("nka,nkb->nab", d, d) / k)
        n0 = v[:, :, 0]
        flip = np.sum(-p[s:s + chunk] * n0, axis=1) < 0.0
        nrm[s:s + chunk] = np.where(flip[:, None], -n0, n0)
        lam[s:s + chunk] = w
    return nrm, lam


def tag_of(prefix, n):
    return "%s_%dM" % (prefix, n // 1_000_000) if n >= 1_000_000 else "%s_%d" % (prefix, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud-points", default="1000000,10000000")
    ap.add_argument("--map-points", default="50000000")
    ap.add_argument("--search-radius", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    out = {}
    ctx = api.Context(0)
    if "a" not in a.skip:
        tgt, _ = scenes.scene_parkinglot()
        gt = scenes.pose6d_matrix(**scenes.PK01_GT)
        sweep = scenes.lidar_sweep(tgt, gt, seed=1)
        sweep = np.ascontiguousarray(sweep[np.isfinite(sweep[:, :3]).all(axis=1), :3])
        out["a_sweep_points"] = len(sweep)
        for k in (5, 16):
            p = api.normal_params(k=k)
            out["a_k%d_ms" % k] = timed(lambda: ctx.normals(sweep, p), a.repeats * 2, warmup=2)
            if "d" not in a.skip:
                res = {}

                def host():
                    res["n"], res["w"] = scipy_normals(sweep, k)
                out["a_k%d_scipy_eigh_ms" % k] = timed(host, 1, warmup=0)
                nrm, _, _, info = ctx.normals(sweep, p)
                apart = (res["w"][:, 1] - res["w"][:, 0]) / res["w"][:, 2] > 1e-3
                cosang = np.abs(np.sum(nrm.astype(np.float64) * res["n"], axis=1))[apart]
                assert info["n_out"] == len(sweep) and np.all(np.arccos(np.minimum(cosang, 1.0)) < 1e-5)
    if "b" not in a.skip:
        for n in [int(x) for x in a.cloud_points.split(",") if x]:
            cloud, _ = scenes.scene_prior_map(n, extent=350.0 * (n / 50e6) ** 0.5)      # (the density of the 50 M-point map)
            tag = tag_of("b", n)
            for k in (5, 16):
                for sr in (0.0, a.search_radius):
                    p = api.normal_params(k=k, search_radius=sr)
                    res = {}

                    def run():
                        res["i"] = ctx.normals(cloud, p)[3]
                    out["%s_k%d_%s_ms" % (tag, k, "bounded" if sr else "unbounded")] = timed(run, a.repeats)
                    out["%s_k%d_%s_sparse" % (tag, k, "bounded" if sr else "unbounded")] = int(res["i"]["n_sparse"])
                if "d" not in a.skip and n <= 10_000_000:
                    out["%s_k%d_scipy_eigh_ms" % (tag, k)] = timed(lambda: scipy_normals(cloud, k), 1, warmup=0)
    if "c" not in a.skip:
        for n in [int(x) for x in a.map_points.split(",") if x]:
            big, _ = scenes.scene_prior_map(n, extent=350.0 * (n / 50e6) ** 0.5)
            tag = tag_of("c", n)
            ctx.set_target(big, 1.0)
            for k in (5, 16):
                p = api.normal_params(k=k)
                out["%s_k%d_target_normals_ms" % (tag, k)] = timed(lambda: ctx.target_normals(p), max(2, a.repeats // 2))
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
