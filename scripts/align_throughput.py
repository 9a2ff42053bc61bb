"""A pose from correspondences on the device (Context.align_correspondences) against a vectorised float64 numpy RANSAC.  A host clock
around calls that end in a synchronise, after warm-up; medians; uploads and downloads included.  Every device leg runs beside its numpy
comparison in the same loop on the same box.  The numpy RANSAC is the same algorithm - seeded three-pair draws, edge-length
pre-rejection, a pose per hypothesis, inlier counts over all pairs, a least-squares refit of the winner - written with whole-array
operations, not this library's rounding.  It scores at most --numpy-budget residuals per leg: where H hypotheses would need more, it
runs fewer and the line says how many ("numpy_hypotheses"), so its time is to be scaled by the reader, not by the script.
  (a) synthetic pairs with a known motion: M = 2 000 and 8 000 pairs at 10 % and 30 % inliers (2 cm noise, d = 0.10), each with H = 10^5
      and 10^6 hypotheses, each with s = 0.9 (the cost sits in k_align_hypotheses: few survive) and s = 0 (every hypothesis is scored:
      the cost sits in k_align_score);
  (b) end to end on the parking lot: the 200 k-point map thinned by the voxel grid at --leaf, descriptors over the whole thinned cloud,
      the cut to its non-planar points (surface variation above --curvature), matching, correspondences_from_match (mutual),
      align_correspondences with the best 8, icp_run_trials_normals of the thinned clouds from those 8 poses.  Two other sides:
      "copy" - the thinned map moved point for point by a known pose, normals turned with it (the same points on both sides);
      "rethinned" - the full map moved first and thinned afterwards, so the grid cuts it differently and no point has its twin.
      Pose errors are given at the lot's centre.
Prints one JSON line.

usage: python scripts/align_throughput.py [--repeats 5] [--leaf 0.5] [--curvature 0.02] [--numpy-budget 5e7] [--skip b]"""
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
    return float(np.median(ts)), float(np.max(ts) - np.min(ts))


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


def kabsch(p, q):
    cp, cq = p.mean(axis=0), q.mean(axis=0)
    U, _, Vt = np.linalg.svd((p - cp).T @ (q - cq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cq - R @ cp


def frames(x0, x1, x2):
    u, v = x1 - x0, x2 - x0
    w = np.cross(u, v)
    ok = np.einsum("ij,ij->i", w, w) > 1e-4 * np.einsum("ij,ij->i", u, u) * np.einsum("ij,ij->i", v, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        e1 = u / np.linalg.norm(u, axis=1, keepdims=True)
        e3 = w / np.linalg.norm(w, axis=1, keepdims=True)
    return ok, np.stack([e1, np.cross(e3, e1), e3], axis=1)


def numpy_ransac(p, q, n_hyp, d, s, rng, budget):
    """-> (R, t, inliers of the refit pose, hypotheses drawn, hypotheses scored)"""
    m = len(p)
    best = (-1, None, None)
    drawn = scored = 0
    spent = 0.0
    batch = 1 << 16
    while drawn < n_hyp and spent < budget:
        n = min(batch, n_hyp - drawn)
        u = rng.integers(0, m, (n, 3))
        drawn += n
        keep = (u[:, 0] != u[:, 1]) & (u[:, 1] != u[:, 2]) & (u[:, 2] != u[:, 0])
        P, Q = p[u], q[u]
        if s > 0.0:
            for i, j in ((0, 1), (1, 2), (2, 0)):
                la, lb = np.linalg.norm(P[:, i] - P[:, j], axis=1), np.linalg.norm(Q[:, i] - Q[:, j], axis=1)
                keep &= (la >= s * lb) & (lb >= s * la)
        P, Q = P[keep], Q[keep]
        ok_p, E = frames(P[:, 0], P[:, 1], P[:, 2])
        ok_q, F = frames(Q[:, 0], Q[:, 1], Q[:, 2])
        ok = ok_p & ok_q
        E, F, P, Q = E[ok], F[ok], P[ok], Q[ok]
        R = np.einsum("nkr,nkc->nrc", F, E)
        t = Q.mean(axis=1) - np.einsum("nrc,nc->nr", R, P.mean(axis=1))
        step = max(1, (1 << 22) // m)
        for s0 in range(0, len(R), step):
            if spent >= budget:
                break
            r = np.einsum("nrc,mc->nmr", R[s0:s0 + step], p) + t[s0:s0 + step, None, :] - q[None]
            cnt = (np.einsum("nmr,nmr->nm", r, r) <= d * d).sum(axis=1)
            k = int(np.argmax(cnt))
            if cnt[k] > best[0]:
                best = (int(cnt[k]), R[s0 + k], t[s0 + k])
            scored += len(cnt)
            spent += float(len(cnt)) * m
    _, R, t = best
    inl = np.zeros(m, bool)
    for _ in range(3):
        if R is None:
            break
        r = p @ R.T + t - q
        inl = np.einsum("ij,ij->i", r, r) <= d * d
        if inl.sum() < 3:
            break
        R, t = kabsch(p[inl], q[inl])
    return R, t, int(inl.sum()), drawn, scored


def pose_error(T, R, t):
    if R is None:
        return [float("nan"), float("nan")]
    dR = R @ T[:3, :3].T
    return [float(np.linalg.norm(t - T[:3, 3])), float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) * 0.5, -1.0, 1.0))))]


def described(ctx, cloud, nrm, fp, curvature, cur=None):
    """descriptors over the WHOLE cloud (a point's support is the surface around it, ground included), then the cut to the non-planar
    points: surface variation above `curvature`.  nrm None: normals (k = 16, oriented upwards) and curvature are estimated first.
    -> (points, descriptors, normals of the whole cloud, keep mask)"""
    if nrm is None:
        c = cloud.mean(axis=0)
        nrm, cur, _, _ = ctx.normals(cloud, api.normal_params(k=16, viewpoint=(float(c[0]), float(c[1]), float(c[2]) + 1000.0)))
    f = ctx.fpfh(cloud, nrm, params=fp)[0]
    keep = np.isfinite(cur) & (cur > curvature) & np.isfinite(f[:, 0])
    return np.ascontiguousarray(cloud[keep]), np.ascontiguousarray(f[keep]), nrm, cur, keep


def centre_error(T, X, c0):
    """the distance between the images of the cloud's centre under the two poses, and the angle between their rotations"""
    dR = X[:3, :3] @ T[:3, :3].T
    return [float(np.linalg.norm((X[:3, :3] @ c0 + X[:3, 3]) - (T[:3, :3] @ c0 + T[:3, 3]))),
            float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) * 0.5, -1.0, 1.0))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leaf", type=float, default=0.5)
    ap.add_argument("--curvature", type=float, default=0.02)
    ap.add_argument("--numpy-budget", type=float, default=5e7)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    out = {}
    ctx = api.Context(0)
    if "a" not in a.skip:
        for m in (2000, 8000):
            for share in (0.1, 0.3):
                pa, pb, ca, cb, T, who = synthetic(m, share, 0.02, m + int(100 * share))
                p64, q64 = pa.astype(np.float64), pb.astype(np.float64)
                for n_hyp in (100000, 1000000):
                    for s in (0.9, 0.0):
                        tag = "a_M%d_in%d_H%d_s%s" % (m, int(100 * share), n_hyp, "09" if s else "0")
                        prm = api.align_params(n_hypotheses=n_hyp, seed=1, inlier_distance=0.10, edge_similarity=s, n_best=1, refine_iterations=3)
                        res, host = {}, {}

                        def run():
                            res["r"] = ctx.align_correspondences(pa, pb, ca, cb, prm)

                        def cpu():
                            host["r"] = numpy_ransac(p64, q64, n_hyp, 0.10, s, np.random.default_rng(1), a.numpy_budget)
                        out[tag + "_ms"], out[tag + "_ms_spread"] = timed(run, a.repeats, warmup=2)
                        out[tag + "_numpy_ms"], _ = timed(cpu, 1, warmup=0)
                        r = res["r"]
                        out[tag + "_scored"] = int(r["info"]["n_scored"])
                        rec = r["records"][0] if r["records"] else None
                        out[tag + "_inliers_of_%d" % len(who)] = int(rec["n_inliers"]) if rec else 0
                        out[tag + "_pose_error_m_deg"] = pose_error(T, rec["T"][:3, :3], rec["T"][:3, 3]) if rec else None
                        out[tag + "_numpy_hypotheses"] = [host["r"][3], host["r"][4]]
                        out[tag + "_numpy_inliers"] = host["r"][2]
                        out[tag + "_numpy_pose_error_m_deg"] = pose_error(T, host["r"][0], host["r"][1])
    if "b" not in a.skip:
        tgt, _ = scenes.scene_parkinglot()
        rng = np.random.default_rng(4)
        c0 = tgt.mean(axis=0).astype(np.float64)
        M = scenes.pose6d_matrix(rng.uniform(-6, 6), rng.uniform(-6, 6), 0.5, np.deg2rad(2.0), np.deg2rad(-3.0), np.deg2rad(rng.uniform(-60, 60)))
        # the motion turns the lot about its own centre, then shifts it
        T = np.eye(4)
        T[:3, :3] = M[:3, :3]
        T[:3, 3] = c0 - M[:3, :3] @ c0 + M[:3, 3]
        moved = (tgt.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        fp = api.fpfh_params(k=16)
        prm = api.align_params(n_hypotheses=100000, seed=1, inlier_distance=a.leaf, edge_similarity=0.9, n_best=8, refine_iterations=3)
        cfg = api.default_config(search_radius=1.0, max_iterations=30, gt_matrix=T.reshape(-1))
        # "copy": the thinned map moved point for point (normals turned with it) - the same points on both sides, the tests' setting at size;
        # "rethinned": the full map moved FIRST and thinned afterwards - the voxel grid cuts it differently, no point has its twin
        for tag in ("copy", "rethinned"):
            res = {}

            def whole():
                t0 = time.perf_counter()
                (thin,), _ = ctx.voxel_downsample([tgt], a.leaf)
                sa, fa, nrm, cur, keep = described(ctx, thin, None, fp, a.curvature)
                if tag == "copy":
                    other = (thin.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
                    sb, fb = described(ctx, other, (nrm.astype(np.float64) @ T[:3, :3].T).astype(np.float32), fp, a.curvature, cur)[:2]
                else:
                    (other,), _ = ctx.voxel_downsample([moved], a.leaf)
                    sb, fb = described(ctx, other, None, fp, a.curvature)[:2]
                t1 = time.perf_counter()
                match = ctx.feature_match(fa, fb)
                ca, cb = api.correspondences_from_match(match, mutual_only=True)
                t2 = time.perf_counter()
                al = ctx.align_correspondences(sa, sb, ca, cb, prm)
                t3 = time.perf_counter()
                trials = []
                if al["records"]:
                    ctx.set_target(other, 1.0)
                    ctx.keep_target_normals(api.normal_params(k=10))
                    ctx.set_source(thin)
                    trials = ctx.icp_run_trials_normals([r["T"] for r in al["records"]], "Ours", cfg)
                t4 = time.perf_counter()
                res.update(n=[len(thin), len(other)], sa=sa, sb=sb, ca=ca, cb=cb, al=al, trials=trials,
                           ms=[(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3])
            whole()
            runs = []
            for _ in range(a.repeats):
                whole()
                runs.append(res["ms"])
            ms = np.median(np.array(runs), axis=0)
            key = "b_%s_" % tag
            out[key + "ms_thin_describe_filter__match__align__refine"] = [float(x) for x in ms]
            out[key + "thinned_points"] = [int(x) for x in res["n"]]
            out[key + "non_planar_points"] = [int(len(res["sa"])), int(len(res["sb"]))]
            out[key + "pairs"] = int(len(res["ca"]))
            al = res["al"]
            out[key + "info"] = al["info"]
            if len(res["ca"]):
                moved_a = res["sa"][res["ca"]].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
                true_in = np.linalg.norm(moved_a - res["sb"][res["cb"]].astype(np.float64), axis=1) <= a.leaf
                out[key + "share_of_pairs_within_leaf_of_truth"] = float(true_in.mean())
            if al["records"]:
                out[key + "inliers"] = [int(r["n_inliers"]) for r in al["records"]]
                out[key + "align_error_m_deg"] = [centre_error(T, r["T"], c0) for r in al["records"]]
                out[key + "refined_error_m_deg_converged"] = [centre_error(T, np.array(t.final_transform).reshape(4, 4), c0) + [int(t.converged)]
                                                              for t in res["trials"]]
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
