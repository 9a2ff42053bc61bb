"""The consensus pose on the device (Context.consensus_correspondences) beside the three-pair sampler (Context.align_correspondences).
A host clock around calls that end in a synchronise, after warm-up; medians and spreads (max - min); uploads and downloads included.
Every leg runs beside its comparisons in the same loop on the same box.
  (a) align_throughput.py's sixteen synthetic settings - M = 2 000 and 8 000 pairs at 10 % and 30 % inliers (2 cm noise, d = 0.10), the
      sampler with H = 10^5 and 10^6, s = 0.9 and 0 - and the consensus call on the same pairs (compatibility 0.10 m, minimum length
      1.0 m, 64 seeds, sets of at most 16);
  (b) the low shares: 2 000 pairs at 1 % and 0.5 %, 8 000 at 1 %, the sampler at H = 10^5 and 10^6 (s = 0.9) beside the call, and for the
      2 000-pair scenes the numpy reference of tests/consensus_ref.py;
  (c) dense graphs, every pair true and exact: the worst case of k_cons_weights;
  (d) align_throughput.py's two end-to-end legs on the parking lot - "copy" and "rethinned" - with the descriptors over a radius of
      --radius, through the consensus call and, in the same loop, through the sampler; nothing is promised of the second leg, the
      inliers found and the pose errors are reported as they come out.
Prints one JSON line.

usage: python scripts/consensus_throughput.py [--repeats 5] [--leaf 0.5] [--radius 2.5] [--curvature 0.02] [--skip d]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dcreg_amd import api, scenes  # noqa: E402

SYN = dict(compat_distance=0.10, min_length=1.0, inlier_distance=0.10, n_seeds=64, consensus_size=16, n_best=1, refine_iterations=3)


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(ts)), float(np.max(ts) - np.min(ts))]


def synthetic(m, share, noise, seed):
    rng = np.random.default_rng(seed)
    T = scenes.pose6d_matrix(*rng.uniform(-10, 10, 3), *rng.uniform(-np.pi / 2, np.pi / 2, 3))
    R, t = T[:3, :3], T[:3, 3]
    a = rng.uniform([-20, -20, -5], [20, 20, 5], (m, 3))
    b = rng.uniform([-20, -20, -5], [20, 20, 5], (m, 3)) @ R.T + t
    who = rng.permutation(m)[:int(round(share * m))]
    b[who] = a[who] @ R.T + t + rng.normal(scale=noise, size=(len(who), 3))
    idx = np.arange(m, dtype=np.int32)
    return a.astype(np.float32), b.astype(np.float32), idx, idx, T, who


def pose_error(T, X):
    dR = X[:3, :3] @ T[:3, :3].T
    return [float(np.linalg.norm(X[:3, 3] - T[:3, 3])), float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) * 0.5, -1.0, 1.0))))]


def centre_error(T, X, c0):
    """the distance between the images of the cloud's centre under the two poses, and the angle between their rotations"""
    dR = X[:3, :3] @ T[:3, :3].T
    return [float(np.linalg.norm((X[:3, :3] @ c0 + X[:3, 3]) - (T[:3, :3] @ c0 + T[:3, 3]))),
            float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) * 0.5, -1.0, 1.0))))]


def true_found(res, who):
    """how many of the true pairs the first record's mask holds, and how many pairs it holds"""
    mask = res["mask"] != 0
    return [int(mask[who].sum()), int(mask.sum())]


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
    cp = api.consensus_params(**SYN)

    def sampler(n_hyp, s):
        return api.align_params(n_hypotheses=n_hyp, seed=1, inlier_distance=0.10, edge_similarity=s, n_best=1, refine_iterations=3)

    def leg(tag, pa, pb, ca, cb, T, who, samplers):
        res = {}

        def cons():
            res["c"] = ctx.consensus_correspondences(pa, pb, ca, cb, cp)
        out[tag + "_consensus_ms_spread"] = timed(cons, a.repeats)
        c = res["c"]
        out[tag + "_consensus_info"] = c["info"]
        out[tag + "_consensus_true_found_of_%d__mask" % len(who)] = true_found(c, who)
        out[tag + "_consensus_pose_error_m_deg"] = pose_error(T, c["records"][0]["T"]) if c["records"] else None
        for n_hyp, s in samplers:
            def ransac():
                res["r"] = ctx.align_correspondences(pa, pb, ca, cb, sampler(n_hyp, s))
            key = "%s_sampler_H%d_s%s" % (tag, n_hyp, "09" if s else "0")
            out[key + "_ms_spread"] = timed(ransac, a.repeats)
            r = res["r"]
            out[key + "_true_found__mask"] = true_found(r, who)
            out[key + "_pose_error_m_deg"] = pose_error(T, r["records"][0]["T"]) if r["records"] else None

    if "a" not in a.skip:
        for m in (2000, 8000):
            for share in (0.1, 0.3):
                pa, pb, ca, cb, T, who = synthetic(m, share, 0.02, m + int(100 * share))
                leg("a_M%d_in%d" % (m, int(100 * share)), pa, pb, ca, cb, T, who, [(100000, 0.9), (100000, 0.0), (1000000, 0.9), (1000000, 0.0)])
    if "b" not in a.skip:
        import consensus_ref
        for m, share in ((2000, 0.01), (2000, 0.005), (8000, 0.01)):
            pa, pb, ca, cb, T, who = synthetic(m, share, 0.02, m + int(10000 * share))
            tag = "b_M%d_in%gpct" % (m, 100 * share)
            leg(tag, pa, pb, ca, cb, T, who, [(100000, 0.9), (1000000, 0.9)])
            if m <= 2000:
                out[tag + "_numpy_reference_ms_spread"] = timed(lambda: consensus_ref.consensus(pa, pb, ca, cb, **SYN), min(a.repeats, 3), warmup=1)
    if "c" not in a.skip:
        for m in (2000, 4000, 8000):
            pa, _, ca, cb, T, who = synthetic(m, 1.0, 0.0, m)
            pb = (pa.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
            leg("c_dense_M%d" % m, pa, pb, ca, cb, T, who, [])
    if "d" not in a.skip:
        tgt, _ = scenes.scene_parkinglot()
        rng = np.random.default_rng(4)
        c0 = tgt.mean(axis=0).astype(np.float64)
        M = scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.5, np.deg2rad(2.0), np.deg2rad(-3.0), np.deg2rad(rng.uniform(-60, 60)))
        T = np.eye(4)                                    # the motion turns the lot about its own centre, then shifts it
        T[:3, :3] = M[:3, :3]
        T[:3, 3] = c0 - M[:3, :3] @ c0 + M[:3, 3]
        moved = (tgt.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        (thin,), _ = ctx.voxel_downsample([tgt], a.leaf)
        pr = api.fpfh_radius_params(a.radius)
        lot = api.consensus_params(compat_distance=a.leaf, min_length=2.0, inlier_distance=a.leaf, n_seeds=64, consensus_size=16, n_best=8,
                                   refine_iterations=3)
        ransac = api.align_params(n_hypotheses=100000, seed=1, inlier_distance=a.leaf, edge_similarity=0.9, n_best=8, refine_iterations=3)
        cfg = api.default_config(search_radius=1.0, max_iterations=30, gt_matrix=T.reshape(-1))
        nrm, cur, _, _ = ctx.normals(thin, api.normal_params(k=16, viewpoint=up(thin)))
        for tag in ("copy", "rethinned"):
            if tag == "copy":
                other = (thin.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
                nrm_b, cur_b = (nrm.astype(np.float64) @ T[:3, :3].T).astype(np.float32), cur
            else:
                (other,), _ = ctx.voxel_downsample([moved], a.leaf)
                nrm_b, cur_b, _, _ = ctx.normals(other, api.normal_params(k=16, viewpoint=up(other)))
            cut = []
            for cloud, n, c in ((thin, nrm, cur), (other, nrm_b, cur_b)):
                f = ctx.fpfh_radius(cloud, n, params=pr)[0]
                keep = np.isfinite(c) & (c > a.curvature) & np.isfinite(f[:, 0])
                cut.append((np.ascontiguousarray(cloud[keep]), np.ascontiguousarray(f[keep])))
            (sa, fa), (sb, fb) = cut
            ca, cb = api.correspondences_from_match(ctx.feature_match(fa, fb), mutual_only=True)
            key = "d_%s_" % tag
            out[key + "thinned_points"] = [len(thin), len(other)]
            out[key + "non_planar_points"] = [len(sa), len(sb)]
            out[key + "mutual_pairs"] = int(len(ca))
            moved_a = sa[ca].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            true_in = np.linalg.norm(moved_a - sb[cb].astype(np.float64), axis=1) <= a.leaf
            out[key + "pairs_within_leaf_of_truth"] = int(true_in.sum())
            res = {}
            for name, call in (("consensus", lambda: ctx.consensus_correspondences(sa, sb, ca, cb, lot, want_weights=True)),
                               ("sampler", lambda: ctx.align_correspondences(sa, sb, ca, cb, ransac))):
                def run():
                    res[name] = call()
                out[key + name + "_ms_spread"] = timed(run, a.repeats)
                r = res[name]
                out[key + name + "_info"] = r["info"]
                if not r["records"]:
                    continue
                ctx.set_target(other, 1.0)
                ctx.keep_target_normals(api.normal_params(k=10))
                ctx.set_source(thin)
                trials = ctx.icp_run_trials_normals([x["T"] for x in r["records"]], "Ours", cfg)
                out[key + name + "_inliers"] = [int(x["n_inliers"]) for x in r["records"]]
                out[key + name + "_true_pairs_in_mask__mask"] = [int(((r["mask"] != 0) & true_in).sum()), int((r["mask"] != 0).sum())]
                out[key + name + "_error_m_deg"] = [centre_error(T, x["T"], c0) for x in r["records"]]
                out[key + name + "_refined_error_m_deg_converged"] = [centre_error(T, np.array(t.final_transform).reshape(4, 4), c0) + [int(t.converged)]
                                                                      for t in trials]
            w = res["consensus"]["weight"]
            out[key + "pairs_with_weight__true_among_them"] = [int((w > 0).sum()), int(((w > 0) & true_in).sum())]
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
