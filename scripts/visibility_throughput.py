"""The visibility votes against the only other route to the same bits: the numpy reference of tests/visibility_ref.py on the host.  A host
clock around calls that end in a synchronise, after warm-up; medians; both routes in the same loop on the same box.
  (a) the range images of --images keyframes of 20 k points: keyframe_range_images (to host memory) and keyframe_range_images_device
      against range_image per keyframe;
  (b) remove_dynamic of a map of --map-keyframes x 20 k points (50 -> 1 M, 500 -> 10 M; rebuilt from the store before every timed call)
      against --members members, voting in cell order and in index order ("visibility_order"); the reference votes on --sample map points
      (all of them would take minutes), must agree with visibility_filter on those bit for bit, and its time is scaled to the whole map;
  (c) a local clean: a 500 k-point map of the nearest 25 keyframes, voted on by those 25.
The frames are cut from the parking-lot scene along a drive (--distinct distinct frames, reused along the path at their own poses).
Prints one JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` (k_vis_image, k_vis_vote, k_vis_keep).

usage: python scripts/visibility_throughput.py [--images 100] [--map-keyframes 50,500] [--members 100,1000] [--sample 20000] [--repeats 3] [--skip bc]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import visibility_ref as vr  # noqa: E402
from dcreg_amd import api, scenes  # noqa: E402

RADIUS = 0.5


def timed(fn, repeats, warmup=1, before=None):
    ts = []
    for k in range(warmup + repeats):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def keyframes(world, n, n_frame, distinct, seed):
    poses, _ = scenes.drive(world, n, step=1.5, n_frame=1, seed=seed)
    frames = scenes.map_frames(world, poses[:distinct], n_frame, seed=seed)
    return [np.asarray(p, np.float64) for p in poses], [frames[k % distinct] for k in range(n)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def nearest(poses, k, n):
    xy = np.array([T[:2, 3] for T in poses])
    return [int(i) for i in np.argsort(np.linalg.norm(xy - xy[k], axis=1), kind="stable")[:n]]


def votes_leg(ctx, frames, poses, map_ids, member_ids, p, sample, repeats, rng):
    """remove_dynamic of the map of map_ids against member_ids, both orders; the reference on a sample of the map"""
    build = [(i, poses[i]) for i in map_ids]
    members = (np.asarray(member_ids), np.stack([poses[i] for i in member_ids]))
    ctx.set_target_keyframes(build, RADIUS)
    cloud = ctx.target_points()
    rec = {"map_points": len(cloud), "members": len(member_ids)}
    for order, name in ((1, "cell_order"), (0, "index_order")):
        ctx.set_option("visibility_order", order)
        infos = []
        rec["remove_dynamic_%s_ms" % name] = timed(lambda: infos.append(ctx.remove_dynamic(members, p)), repeats,
                                                   before=lambda: ctx.set_target_keyframes(build, RADIUS))
        assert all(i == infos[0] for i in infos)
        rec.setdefault("info", infos[0])
        assert rec["info"] == infos[0]
    ctx.set_option("visibility_order", 1)
    pick = np.sort(rng.choice(len(cloud), min(sample, len(cloud)), replace=False))
    q = np.ascontiguousarray(cloud[pick])
    mlist = [(i, poses[i]) for i in member_ids]
    images = {}
    t0 = time.perf_counter()
    for i in set(member_ids):
        images[i] = vr.range_image(frames[i], p)
    t_img = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = vr.filter_ref(q, frames, mlist, p, images)
    t_vote = (time.perf_counter() - t0) * 1e3
    got = ctx.visibility_filter(q, members, p)
    rec["ambiguous_in_sample"] = vr.ambiguous([], p, q, mlist)
    rec["sample_same_bits"] = bool(np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]) and same(got[0], ref[0]))
    rec["numpy_images_ms"] = t_img
    rec["numpy_votes_scaled_to_map_ms"] = t_vote * len(cloud) / max(len(q), 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--map-keyframes", default="50,500")
    ap.add_argument("--members", default="100,1000")
    ap.add_argument("--distinct", type=int, default=40)
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    out = {}
    rng = np.random.default_rng(6)
    p = api.visibility_params()
    world, _ = scenes.scene_parkinglot(n_map=400_000)
    n_members = [int(v) for v in a.members.split(",")]
    n_kf = max(n_members + [a.images, 25] + [int(v) for v in a.map_keyframes.split(",")])
    poses, frames = keyframes(world, n_kf, 20000, a.distinct, seed=3)
    ctx = api.Context(0)
    ctx.keyframes_reset()
    for k in range(0, n_kf, 50):
        ctx.keyframes_add(frames[k:k + 50])
    if "a" not in a.skip:
        ids = list(range(a.images))
        got = ctx.keyframe_range_images(ids, p)
        t0 = time.perf_counter()
        ref = np.stack([vr.range_image(frames[i], p) for i in ids])
        out["a_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        out.update(a_images=a.images, a_same_bits=bool(same(got, ref)), a_ambiguous=vr.ambiguous([frames[i] for i in set(ids)], p))
        out["a_range_images_host_ms"] = timed(lambda: ctx.keyframe_range_images(ids, p), a.repeats)
        hip = C.CDLL("libamdhip64.so.7")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        buf = C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), 4 * a.images * p.rows * p.cols) == 0
        out["a_range_images_device_ms"] = timed(lambda: ctx.keyframe_range_images_device(ids, buf.value, p), a.repeats * 2, warmup=2)
        hip.hipFree(buf)
    if "b" not in a.skip:
        out["b"] = []
        for n_map in (int(v) for v in a.map_keyframes.split(",")):
            for m in n_members:
                out["b"].append(votes_leg(ctx, frames, poses, list(range(n_map)), list(range(m)), p, a.sample, a.repeats, rng))
    if "c" not in a.skip:
        near = nearest(poses, n_kf // 2, 25)
        out["c"] = votes_leg(ctx, frames, poses, near, near, p, a.sample, a.repeats, rng)
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
