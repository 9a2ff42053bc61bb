"""FPFH descriptors over a radius support on the device (dcreg_fpfh_radius*).  A host clock around calls that end in a synchronise, after
warm-up; medians of --repeats.  Every leg runs the k = 16 form of dcreg_fpfh beside it in the same loop on the same box.
  (a) the 200 k-point parking-lot map thinned by the voxel grid at --leaf (normals given, k = 16 oriented upwards) at the radii of
      --radii, each with its mean m (m_sum / n_used) and m_max; an 8 k-point frame at the first radius; target_fpfh_radius() of the
      thinned lot as the resident map from its kept normals (no upload, no build of an index);
  (b) the second end-to-end leg of scripts/align_throughput.py - the full map moved first and thinned afterwards, so that no point has
      its twin -: descriptors over the whole thinned clouds, the cut to the non-planar points (surface variation above --curvature),
      mutual matches, align_correspondences with the best 8, icp_run_trials_normals from those 8 poses; once with the descriptors at the
      last radius of --radii and once with the k = 16 ones.  Reported per side: the mutual pairs, the share of them within one leaf of the
      truth, the inliers of the hypotheses, the errors of the poses before and after the refinement.
Prints one JSON line.

usage: python scripts/features_radius_throughput.py [--repeats 5] [--leaf 0.5] [--radii 1.0,1.5,2.5] [--curvature 0.02] [--skip b]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def up(cloud):
    c = cloud.mean(axis=0)
    return (float(c[0]), float(c[1]), float(c[2]) + 1000.0)


def centre_error(T, X, c0):
    """the distance between the images of the cloud's centre under the two poses, and the angle between their rotations"""
    dR = X[:3, :3] @ T[:3, :3].T
    return [float(np.linalg.norm((X[:3, :3] @ c0 + X[:3, 3]) - (T[:3, :3] @ c0 + T[:3, 3]))),
            float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) * 0.5, -1.0, 1.0))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--radii", default="1.0,1.5,2.5")
    ap.add_argument("--curvature", type=float, default=0.02)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    radii = [float(x) for x in a.radii.split(",")]
    out = {}
    ctx = api.Context(0)
    tgt, frame = scenes.scene_parkinglot()
    (thin,), _ = ctx.voxel_downsample([tgt], a.leaf)
    pk = api.fpfh_params(k=16)
    if "a" not in a.skip:
        for tag, cloud, rs in (("lot_thinned", thin, radii), ("frame_8k", frame, radii[:1])):
            nrm = ctx.normals(cloud, api.normal_params(k=16, viewpoint=up(cloud)))[0]
            out["a_%s_points" % tag] = len(cloud)
            for r in rs:
                p = api.fpfh_radius_params(r)
                res = {}

                def run():
                    res["i"] = ctx.fpfh_radius(cloud, nrm, params=p)[2]
                key = "a_%s_r%g_" % (tag, r)
                out[key + "ms"] = timed(run, a.repeats)
                out[key + "k16_ms"] = timed(lambda: ctx.fpfh(cloud, nrm, params=pk), a.repeats)
                i = res["i"]
                out[key + "mean_m"] = i["m_sum"] / max(i["n_used"], 1)
                out[key + "m_max"] = i["m_max"]
                out[key + "n_out_of_used"] = [i["n_out"], i["n_used"]]
        ctx.set_target(thin, 0.5)
        ctx.keep_target_normals(api.normal_params(k=16, viewpoint=up(thin)))
        for r in radii:
            p = api.fpfh_radius_params(r)
            out["a_map_r%g_target_fpfh_radius_ms" % r] = timed(lambda: ctx.target_fpfh_radius(p), a.repeats)
        out["a_map_k16_target_fpfh_ms"] = timed(lambda: ctx.target_fpfh(pk), a.repeats)
    if "b" not in a.skip:
        rng = np.random.default_rng(4)
        c0 = tgt.mean(axis=0).astype(np.float64)
        M = scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.5, np.deg2rad(2.0), np.deg2rad(-3.0), np.deg2rad(rng.uniform(-60, 60)))
        T = np.eye(4)                                    # the motion turns the lot about its own centre, then shifts it
        T[:3, :3] = M[:3, :3]
        T[:3, 3] = c0 - M[:3, :3] @ c0 + M[:3, 3]
        moved = (tgt.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        (other,), _ = ctx.voxel_downsample([moved], a.leaf)
        prm = api.align_params(n_hypotheses=100000, seed=1, inlier_distance=a.leaf, edge_similarity=0.9, n_best=8, refine_iterations=3)
        cfg = api.default_config(search_radius=1.0, max_iterations=30, gt_matrix=T.reshape(-1))
        sides = []
        for cloud in (thin, other):
            nrm, cur, _, _ = ctx.normals(cloud, api.normal_params(k=16, viewpoint=up(cloud)))
            sides.append((cloud, nrm, cur))
        pr = api.fpfh_radius_params(radii[-1])
        for tag, describe in (("r%g" % radii[-1], lambda c, n: ctx.fpfh_radius(c, n, params=pr)[0]), ("k16", lambda c, n: ctx.fpfh(c, n, params=pk)[0])):
            t0 = time.perf_counter()
            cut = []
            for cloud, nrm, cur in sides:
                f = describe(cloud, nrm)
                keep = np.isfinite(cur) & (cur > a.curvature) & np.isfinite(f[:, 0])
                cut.append((np.ascontiguousarray(cloud[keep]), np.ascontiguousarray(f[keep])))
            (sa, fa), (sb, fb) = cut
            t1 = time.perf_counter()
            match = ctx.feature_match(fa, fb)
            ca, cb = api.correspondences_from_match(match, mutual_only=True)
            al = ctx.align_correspondences(sa, sb, ca, cb, prm)
            trials = []
            if al["records"]:
                ctx.set_target(other, 1.0)
                ctx.keep_target_normals(api.normal_params(k=10))
                ctx.set_source(thin)
                trials = ctx.icp_run_trials_normals([r["T"] for r in al["records"]], "Ours", cfg)
            t2 = time.perf_counter()
            key = "b_%s_" % tag
            out[key + "ms_describe_and_cut__match_align_refine"] = [(t1 - t0) * 1e3, (t2 - t1) * 1e3]
            out[key + "thinned_points"] = [len(thin), len(other)]
            out[key + "non_planar_points"] = [len(sa), len(sb)]
            out[key + "mutual_pairs"] = int(len(ca))
            if len(ca):
                moved_a = sa[ca].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
                true_in = np.linalg.norm(moved_a - sb[cb].astype(np.float64), axis=1) <= a.leaf
                out[key + "pairs_within_leaf_of_truth"] = int(true_in.sum())
                out[key + "share_of_pairs_within_leaf_of_truth"] = float(true_in.mean())
            if al["records"]:
                out[key + "inliers"] = [int(r["n_inliers"]) for r in al["records"]]
                out[key + "align_error_m_deg"] = [centre_error(T, r["T"], c0) for r in al["records"]]
                out[key + "refined_error_m_deg_converged"] = [centre_error(T, np.array(t.final_transform).reshape(4, 4), c0) + [int(t.converged)]
                                                              for t in trials]
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
