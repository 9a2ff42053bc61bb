"""Place recognition on the device against numpy.  A host clock around calls that end in a synchronise, after warm-up; medians.
  (a) descriptors: one 128 x 1024 sweep (scenes.lidar_sweep over the 200 k-point parking-lot map) through place_descriptors, and --sweeps such
      sweeps in one call, against the numpy rule (np.maximum.at over the bins) for the same clouds;
  (b) search: 1 and 64 queries against databases of 10 k and 100 k seeded random descriptors (k = 5), against the numpy rule evaluated in
      bulk on --numpy-entries entries and scaled to the database's size;
  (c) an end-to-end revisit: the keyframes of a 120-frame drive through a 4 M-point prior map added to the database, 24 revisit sweeps (random
      yaw, up to 1.5 m off the path) queried with k = 5, the five candidates of every query verified in ONE register_pairs call from
      place_guess, and per query the converged candidate with the lowest final rmse kept: how many revisits end within 10 cm and 0.5 deg of
      the truth, against how many do when registered against their own keyframe from the true pose.
Prints one JSON line.

usage: python scripts/places_throughput.py [--sweeps 256] [--repeats 20] [--numpy-entries 2000] [--skip-revisit]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402

TWO_PI = 2.0 * np.pi


def numpy_descriptor(cloud, p):
    """include/dcreg.h's rule for one cloud, vectorised on the host -> [n_rings, n_sectors] float32"""
    xyz = cloud[:, :3]
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        r2 = x * x + y * y
        used = np.isfinite(xyz).all(1) & (r2 >= p.min_range ** 2) & (r2 < p.max_range ** 2)
    r2, x, y = r2[used], x[used], y[used]
    ring = np.minimum(np.floor(np.sqrt(r2) * p.n_rings / p.max_range).astype(np.int64), p.n_rings - 1)
    th = np.arctan2(y, x)
    th = np.where(th < 0.0, th + TWO_PI, th)
    sector = np.minimum(np.floor(th * p.n_sectors / TWO_PI).astype(np.int64), p.n_sectors - 1)
    d = np.full(p.n_rings * p.n_sectors, -np.inf, np.float32)
    np.maximum.at(d, ring * p.n_sectors + sector, (xyz[used, 2].astype(np.float64) + p.z_offset).astype(np.float32))
    d[np.isneginf(d)] = 0.0
    return d.reshape(p.n_rings, p.n_sectors)


def numpy_search(qs, db, k):
    """the header's distance for every (query, entry, shift) in bulk and the k best entries per query -> (idx, shift, dist)"""
    S = qs.shape[2]
    q64, c64 = qs.astype(np.float64), db.astype(np.float64)
    qn, cn = np.sqrt((q64 * q64).sum(1)), np.sqrt((c64 * c64).sum(1))
    j = np.arange(S)
    col = (j[None, :] + j[:, None]) % S
    idx, shift, dist = [], [], []
    for qi in range(len(qs)):
        best, arg = np.empty(len(db)), np.empty(len(db), np.int64)
        for e0 in range(0, len(db), 256):
            dots = np.einsum("rj,erl->ejl", q64[qi], c64[e0:e0 + 256])
            den = qn[qi][None, :, None] * cn[e0:e0 + 256, None, :]
            ok = den > 0.0
            with np.errstate(invalid="ignore", divide="ignore"):
                term = np.where(ok, 1.0 - dots / den, 0.0)
            m = ok[:, j[None, :], col].sum(2)
            D = np.where(m > 0, term[:, j[None, :], col].sum(2) / np.maximum(m, 1), 1.0)
            best[e0:e0 + 256], arg[e0:e0 + 256] = D.min(1), D.argmin(1)
        order = np.lexsort((np.arange(len(db)), best))[:k]
        idx.append(order)
        shift.append(arg[order])
        dist.append(best[order])
    return np.array(idx), np.array(shift), np.array(dist)


def random_descriptors(n, p, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, 6.0, (n, p.n_rings, p.n_sectors)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.2] = 0.0
    return d


def clock(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def revisit(ctx, out):
    world, _ = scenes.scene_prior_map(n_map=4_000_000, extent=220.0)
    poses, frames = scenes.drive(world, 120, n_frame=8_000, seed=5)
    near, rev_poses, revs = scenes.revisits(world, poses, 24, 1.5, 8_000, seed=105)
    p = api.place_params(max_range=30.0)
    cfg = api.default_config(search_radius=1.0, max_iterations=30)
    ctx.places_reset(p)
    t0 = time.perf_counter()
    ctx.places_add_clouds(frames)
    t1 = time.perf_counter()
    idx, shift, dist, _ = ctx.places_query_clouds(revs, 5)
    t2 = time.perf_counter()
    src = [revs[q] for q in range(len(revs)) for _ in range(5)]
    tgt = [frames[e] for e in idx.reshape(-1)]
    T0 = [api.place_guess(s, p.n_sectors) for s in shift.reshape(-1)]
    recs = ctx.register_pairs(src, tgt, T0, "Ours", cfg)
    t3 = time.perf_counter()

    def good(rec, truth):
        t_err, r_err = api.pose_error(truth, np.array(rec.final_transform[:]).reshape(4, 4))
        return bool(rec.converged) and t_err <= 0.10 and r_err <= 0.5

    found = 0
    for q in range(len(revs)):
        cand = [(recs[5 * q + s].final_rmse, s) for s in range(5) if recs[5 * q + s].converged]
        if cand:
            s = min(cand)[1]
            found += good(recs[5 * q + s], np.linalg.inv(poses[idx[q, s]]) @ rev_poses[q])
    truths = [np.linalg.inv(poses[kf]) @ T for kf, T in zip(near, rev_poses)]
    base = ctx.register_pairs(revs, [frames[kf] for kf in near], truths, "Ours", cfg)
    out.update(c_keyframes=len(frames), c_revisits=len(revs), c_add_clouds_ms=(t1 - t0) * 1e3, c_query_clouds_k5_ms=(t2 - t1) * 1e3,
               c_register_pairs_120_ms=(t3 - t2) * 1e3, c_top1_within_one_keyframe=int((np.abs(idx[:, 0] - near) <= 1).sum()),
               c_within_10cm_half_degree=int(found), c_within_from_true_pose=int(sum(good(r, T) for r, T in zip(base, truths))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--numpy-entries", type=int, default=2000)
    ap.add_argument("--skip-revisit", action="store_true")
    a = ap.parse_args()
    ctx = api.Context(0)
    p = api.place_params()
    tgt, _ = scenes.scene_parkinglot()
    sweep = scenes.lidar_sweep(tgt, scenes.pose6d_matrix(**scenes.PK01_GT))
    out = {"points_per_sweep": len(sweep), "finite_per_sweep": int(np.isfinite(sweep).all(1).sum()), "rings_x_sectors": [p.n_rings, p.n_sectors]}
    # (a) descriptors
    out["a_descriptor_1_sweep_ms"] = clock(lambda: ctx.place_descriptors([sweep], p), a.repeats)
    out["a_numpy_descriptor_1_sweep_ms"] = clock(lambda: numpy_descriptor(sweep, p), max(3, a.repeats // 4))
    allr = np.ascontiguousarray(np.tile(sweep, (a.sweeps, 1)))
    off = np.arange(a.sweeps + 1, dtype=np.int64) * len(sweep)
    out["a_sweeps"] = a.sweeps
    out["a_descriptor_sweeps_ms"] = clock(lambda: ctx.place_descriptors((allr, off), p), max(3, a.repeats // 4))
    out["a_numpy_descriptor_sweeps_ms"] = out["a_numpy_descriptor_1_sweep_ms"] * a.sweeps
    assert np.array_equal(ctx.place_descriptors([sweep], p)[0][0], numpy_descriptor(sweep, p))
    del allr
    # (b) search
    db = random_descriptors(100_000, p, seed=1)
    qs = random_descriptors(64, p, seed=2)
    small = db[:a.numpy_entries]
    t0 = time.perf_counter()
    ref = numpy_search(qs[:2], small, 5)
    per_pair_ms = (time.perf_counter() - t0) * 1e3 / (2 * len(small))
    out["b_numpy_entries"] = len(small)
    out["b_numpy_ms_per_pair"] = per_pair_ms
    for n in (10_000, 100_000):
        ctx.places_reset(p)
        ctx.places_add(db[:n])
        for nq in (1, 64):
            key = "b_query_%dk_entries_%d_queries" % (n // 1000, nq)
            out[key + "_ms"] = clock(lambda: ctx.places_query(qs[:nq], 5), max(3, a.repeats // 4))
            out[key + "_numpy_scaled_ms"] = per_pair_ms * n * nq
    ctx.places_reset(p)
    ctx.places_add(small)
    got = ctx.places_query(qs[:2], 5)
    out["b_device_equals_numpy_top5"] = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.abs(got[2] - ref[2]).max() <= 1e-12)
    if not a.skip_revisit:
        revisit(ctx, out)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
