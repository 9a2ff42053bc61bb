"""numpy reference of the verification call (include/dcreg.h, "Verification of candidate poses against the map"): the rule, literally.

For the poses T_k, a cloud, d = inlier_distance, s = point_stride:
  1. row i of the cloud is used when its three coordinates are finite and selected when i % s == 0; n_scored = the selected used rows;
  2. q = normal_icp_ref.transform(R_k, t_k, p): double, every operation rounded once, float32 store; a non-finite q is no inlier;
  3. (j, d2) = normal_icp_ref.nearest(map, q): the first map point in (d2, index) order, d2 in float32;
  4. inlier iff (double)d2 < d * d; e = floor(((double)d2 / (d * d)) * 2^20) as an integer;
  5. count = the inliers, cost = the sum of e, score = cost + (n_scored - count) * 2^20 - Python integers;
  6. fitness = count / n_scored (0.0 for n_scored == 0), rmse = sqrt(((cost / 2^20) * dd) / count) (0.0 for count == 0), in double;
  7. rank_by 0: (count descending, cost ascending, k ascending); rank_by 1: (score ascending, count descending, k ascending);
  8. detail of pose k: mask [n] uint8 and nn [n] int32 in the cloud's original order (0 / -1 at every row that is no inlier).
"""
import math

import numpy as np

import normal_icp_ref as nref

UNIT = 1048576


def selected(cloud, point_stride=1):
    """the original indices of the rows that are scored: selected (i % s == 0) and used (finite)"""
    xyz = np.asarray(cloud, np.float32)[:, :3]
    i = np.arange(len(xyz))
    return np.flatnonzero((i % int(point_stride) == 0) & np.isfinite(xyz).all(axis=1))


def score_pose(map_xyz, cloud, T, d, point_stride=1):
    """one pose -> dict count, cost, score, n_scored (Python ints), fitness, rmse (floats), mask [n] uint8, nn [n] int32, d2 [n] float32
    (the nearest map point's float d2 of every scored row, +inf elsewhere: ungated, what the tests' preconditions look at)"""
    map_xyz = np.ascontiguousarray(np.asarray(map_xyz, np.float32)[:, :3])
    xyz = np.asarray(cloud, np.float32)[:, :3]
    T = np.asarray(T, np.float64).reshape(4, 4)
    n = len(xyz)
    sel = selected(xyz, point_stride)
    mask, nn, d2_all = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, np.inf, np.float32)
    dd = np.float64(d) * np.float64(d)
    count, cost = 0, 0
    if len(sel):
        with np.errstate(over="ignore", invalid="ignore"):
            q = nref.transform(T[:3, :3], T[:3, 3], xyz[sel])
        ok = np.isfinite(q).all(axis=1)
        j = np.zeros(len(sel), np.int64)
        d2 = np.full(len(sel), np.inf, np.float32)
        if ok.any():
            j[ok], d2[ok] = nref.nearest(map_xyz, q[ok])
        inl = ok & (d2.astype(np.float64) < dd)
        e = np.floor((d2[inl].astype(np.float64) / dd) * np.float64(UNIT))
        count, cost = int(inl.sum()), sum(int(v) for v in e)
        mask[sel[inl]] = 1
        nn[sel[inl]] = j[inl]
        d2_all[sel] = d2
    n_scored = len(sel)
    fitness = float(np.float64(count) / np.float64(n_scored)) if n_scored else 0.0
    rmse = float(np.sqrt(((np.float64(cost) / np.float64(UNIT)) * dd) / np.float64(count))) if count else 0.0
    return dict(count=count, cost=cost, score=cost + (n_scored - count) * UNIT, n_scored=n_scored, fitness=fitness, rmse=rmse, mask=mask, nn=nn,
                d2=d2_all)


def rank(scores, rank_by=0):
    """the input indices, best first"""
    if rank_by == 0:
        key = lambda k: (-scores[k]["count"], scores[k]["cost"], k)
    else:
        key = lambda k: (scores[k]["score"], -scores[k]["count"], k)
    return sorted(range(len(scores)), key=key)


def verify(map_xyz, cloud, Ts, d=0.5, point_stride=1, rank_by=0):
    """-> dict scores (per input pose, score_pose's dicts), order (ranked input indices), records (the ranked dicts with `pose` added),
    n_scored"""
    Ts = np.asarray(Ts, np.float64).reshape(-1, 4, 4)
    scores = [score_pose(map_xyz, cloud, T, d, point_stride) for T in Ts]
    order = rank(scores, rank_by)
    recs = [dict(scores[k], pose=k) for k in order]
    return dict(scores=scores, order=order, records=recs, n_scored=len(selected(cloud, point_stride)))


def record_key(r):
    """what a record is compared by, derived values as bit patterns"""
    return (int(r["pose"]), int(r["count"]), int(r["cost"]), int(r["score"]), np.float64(r["fitness"]).tobytes(), np.float64(r["rmse"]).tobytes())


def assert_records(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for a, b in zip(got, want):
        assert record_key(a) == record_key(b), (what, {k: a[k] for k in ("pose", "count", "cost", "score", "fitness", "rmse")},
                                                {k: b[k] for k in ("pose", "count", "cost", "score", "fitness", "rmse")})


LOT_OFFSETS = ((0.05, 0.2), (0.2, 1.0), (0.5, 3.0), (2.0, 10.0), (30.0, 90.0))      # (metres along x, degrees of yaw about the own position)


def lot_poses():
    """the lot's ground truth and its five competitors (normal_icp_scenes.offset: moved along x, turned about the pose's own position)"""
    import normal_icp_scenes as sc
    G = sc.lot()["GT"]
    return np.stack([np.array(G)] + [sc.offset(G, dx=m, yaw=math.radians(a)) for m, a in LOT_OFFSETS])
