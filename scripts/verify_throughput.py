"""Candidate poses scored against the map (Context.verify_poses) beside what a caller did before the call existed.  A host clock
around calls that end in a synchronise, after warm-up; medians of --repeats and spreads (max - min); uploads and downloads included.
All legs of a setting alternate in ONE loop on one box.
  (a) the 8 k frame of the parking lot against its 200 k map, P = 32 and P = 1 024 seeded perturbations of the truth, d = 0.3, point
      stride 1 and 4 - the resident form and the cloud form;
  (b) the lot thinned at --leaf against itself, 64 poses, stride 1 and 4;
  beside each, in the same loop (P = 1 024: on the first 32 poses, scaled figures are not reported):
      knn_loop   a loop of Context.knn(transformed cloud, 1, d) with the count taken in numpy - what the call replaces;
      p2p_loop   a loop of Context.p2p_error(T, d), which also makes a backward pass over the map.
  (c) the end-to-end leg of consensus_throughput.py ("rethinned": descriptors over a radius, mutual matches, the consensus call with
      n_best = 8) with the new stage: where the records whose refined pose ends within 0.05 m of the truth stand in the verified rank.
Every verify result is compared with the knn loop's counts.  Prints one JSON line.

usage: python scripts/verify_throughput.py [--repeats 5] [--leaf 0.5] [--radius 2.5] [--curvature 0.02] [--skip c]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dcreg_amd import api, scenes  # noqa: E402


def perturbed(G, P, seed):
    rng = np.random.default_rng(seed)
    Ts = [np.array(G)]
    for k in range(1, P):
        a = 3.0 * k / max(P - 1, 1)
        M = scenes.pose6d_matrix(0.0, 0.0, 0.0, 0.0, 0.0, rng.normal(0.0, 0.01 + 0.1 * a))
        T = np.array(G)
        T[:3, :3] = M[:3, :3] @ T[:3, :3]
        T[:3, 3] += rng.normal(0.0, 0.02 + a, 3) * [1.0, 1.0, 0.1]
        Ts.append(T)
    return np.stack(Ts)


def transform(T, p):
    q = np.empty((len(p), 3), np.float32)
    P = p[:, :3].astype(np.float64)
    for a in range(3):
        q[:, a] = (((T[a, 0] * P[:, 0] + T[a, 1] * P[:, 1]) + T[a, 2] * P[:, 2]) + T[a, 3]).astype(np.float32)
    return q


def alternating(legs, repeats, warmup=2):
    """legs: name -> callable; every round runs each leg once, in turn -> name -> [median ms, spread ms]"""
    ts = {k: [] for k in legs}
    for r in range(warmup + repeats):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: [float(np.median(v)), float(np.max(v) - np.min(v))] for k, v in ts.items()}


def setting(ctx, out, tag, src, Ts, d, repeats):
    """the resident source is src; the loops run on at most the first 32 poses"""
    few = Ts[:32]
    res = {}

    def knn_loop():
        cnt = []
        dd = np.float64(d) * np.float64(d)
        for T in few:
            idx, d2 = ctx.knn(transform(T, src), 1, d)
            cnt.append(int(((idx[:, 0] >= 0) & (d2[:, 0].astype(np.float64) < dd)).sum()))
        res["knn"] = cnt

    def p2p_loop():
        res["p2p"] = [ctx.p2p_error(T, d)[3] for T in few]

    legs = {}
    for stride in (1, 4):
        p = api.verify_params(inlier_distance=d, point_stride=stride)
        legs["verify_P%d_stride%d" % (len(Ts), stride)] = lambda p=p, stride=stride: res.__setitem__(("v", stride), ctx.verify_poses(Ts, p))
        legs["verify_cloud_P%d_stride%d" % (len(Ts), stride)] = lambda p=p, stride=stride: res.__setitem__(("c", stride), ctx.verify_poses(Ts, p, cloud=src))
    legs["knn_loop_P%d" % len(few)] = knn_loop
    legs["p2p_loop_P%d_with_backward_pass" % len(few)] = p2p_loop
    for k, v in alternating(legs, repeats).items():
        out["%s_%s_ms_spread" % (tag, k)] = v
    by_pose = {r["pose"]: r["count"] for r in res[("v", 1)]["records"]}
    out[tag + "_counts_equal_knn_loop"] = bool([by_pose[k] for k in range(len(few))] == res["knn"])
    out[tag + "_cloud_form_equal"] = bool(res[("v", 1)]["records"] == res[("c", 1)]["records"] and res[("v", 4)]["records"] == res[("c", 4)]["records"])
    out[tag + "_n_scored_stride_1_4"] = [res[("v", 1)]["info"]["n_scored"], res[("v", 4)]["info"]["n_scored"]]
    out[tag + "_best_pose_stride_1_4"] = [res[("v", 1)]["info"]["best_pose"], res[("v", 4)]["info"]["best_pose"]]


def centre_error(T, X, c0):
    dR = X[:3, :3] @ T[:3, :3].T
    return [float(np.linalg.norm((X[:3, :3] @ c0 + X[:3, 3]) - (T[:3, :3] @ c0 + T[:3, 3]))),
            float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) * 0.5, -1.0, 1.0))))]


def up(cloud):
    c = cloud.mean(axis=0)
    return (float(c[0]), float(c[1]), float(c[2]) + 1000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--radius", type=float, default=2.5)
    ap.add_argument("--curvature", type=float, default=0.02)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    out = {}
    ctx = api.Context(0)
    tgt, frame = scenes.scene_parkinglot()
    G = scenes.pose6d_matrix(**scenes.PK01_GT)
    if "a" not in a.skip:
        ctx.set_target(tgt, 0.5)
        ctx.set_source(frame)
        out["a_points_map_frame"] = [len(tgt), len(frame)]
        for P in (32, 1024):
            setting(ctx, out, "a_P%d" % P, frame, perturbed(G, P, P), 0.3, a.repeats)
    (thin,), _ = ctx.voxel_downsample([tgt], a.leaf)
    if "b" not in a.skip:
        ctx.set_target(thin, a.leaf)
        ctx.set_source(thin)
        out["b_points"] = len(thin)
        setting(ctx, out, "b_P64", thin, perturbed(np.eye(4), 64, 64), 0.3, a.repeats)
    if "c" not in a.skip:
        rng = np.random.default_rng(4)
        c0 = tgt.mean(axis=0).astype(np.float64)
        M = scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.5, np.deg2rad(2.0), np.deg2rad(-3.0), np.deg2rad(rng.uniform(-60, 60)))
        T = np.eye(4)                                    # the motion turns the lot about its own centre, then shifts it
        T[:3, :3] = M[:3, :3]
        T[:3, 3] = c0 - M[:3, :3] @ c0 + M[:3, 3]
        moved = (tgt.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        (other,), _ = ctx.voxel_downsample([moved], a.leaf)
        pr = api.fpfh_radius_params(a.radius)
        cut = []
        for cloud in (thin, other):
            n, c, _, _ = ctx.normals(cloud, api.normal_params(k=16, viewpoint=up(cloud)))
            f = ctx.fpfh_radius(cloud, n, params=pr)[0]
            keep = np.isfinite(c) & (c > a.curvature) & np.isfinite(f[:, 0])
            cut.append((np.ascontiguousarray(cloud[keep]), np.ascontiguousarray(f[keep])))
        (sa, fa), (sb, fb) = cut
        ca, cb = api.correspondences_from_match(ctx.feature_match(fa, fb), mutual_only=True)
        lot = api.consensus_params(compat_distance=a.leaf, min_length=2.0, inlier_distance=a.leaf, n_seeds=64, consensus_size=16, n_best=8,
                                   refine_iterations=3)
        r = ctx.consensus_correspondences(sa, sb, ca, cb, lot)
        out["c_mutual_pairs"] = int(len(ca))
        out["c_consensus_records"] = len(r["records"])
        if r["records"]:
            cfg = api.default_config(search_radius=1.0, max_iterations=30, gt_matrix=T.reshape(-1))
            ctx.set_target(other, 1.0)
            ctx.keep_target_normals(api.normal_params(k=10))
            ctx.set_source(thin)
            Ts = np.stack([x["T"] for x in r["records"]])
            res = {}
            for d in (a.leaf, 0.3):
                for rank_by in (0, 1):
                    p = api.verify_params(inlier_distance=d, rank_by=rank_by)
                    t = alternating({"v": lambda: res.__setitem__("v", ctx.verify_poses(Ts, p))}, a.repeats)["v"]
                    key = "c_d%g_rank%d_" % (d, rank_by)
                    out[key + "verify_ms_spread"] = t
                    out[key + "order"] = res["v"]["order"]
                    out[key + "counts_in_consensus_order"] = [x["count"] for x in sorted(res["v"]["records"], key=lambda x: x["pose"])]
            trials = ctx.icp_run_trials_normals(list(Ts), "Ours", cfg)
            err = [centre_error(T, np.array(t.final_transform).reshape(4, 4), c0) for t in trials]
            out["c_consensus_error_m_deg"] = [centre_error(T, x, c0) for x in Ts]
            out["c_refined_error_m_deg"] = err
            out["c_records_refined_within_5cm"] = [k for k, e in enumerate(err) if e[0] < 0.05]
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
