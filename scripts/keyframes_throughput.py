"""The keyframe store against the only route without it: the caller keeps the clouds on the host, transforms and concatenates them with
numpy and hands the result to the voxel calls.  A host clock around calls that end in a synchronise, after warm-up; medians; both routes in
the same loop on the same box.
  (a) keyframes_add_source per keyframe of 8 k / 20 k points (the source is already on the device: the host route keeps a reference, 0 ms);
  (b) --submaps submaps of --members members x 8 k points with a leaf: keyframe_submaps against numpy transform + concatenate +
      voxel_downsample from host buffers;
  (c) a map rebuild after a pose-graph update: set_target_keyframes of --keyframes keyframes x 20 k points with a leaf against numpy
      transform + concatenate + set_target_voxel; the gather on its own as the raw device-output form of the same members (kernel, the
      upload of the member records and one synchronise);
  (d) a local map of the nearest --local keyframes at every keyframe, both routes.
The frames are cut from the parking-lot scene along a drive (--distinct distinct frames, reused along the path at their own poses).  Checks
that both routes of (b), (c) and (d) give the same bits.  Prints one JSON line.

usage: python scripts/keyframes_throughput.py [--keyframes 1000] [--submaps 64] [--members 11] [--local 25] [--leaf 0.2] [--repeats 5] [--skip cd]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dcreg_amd import api, scenes  # noqa: E402

RADIUS = 0.5


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def transform(xyz, T):
    """the member transform of include/dcreg.h in numpy"""
    p = xyz.astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    return np.stack([R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1] + R[a, 2] * p[:, 2] + t[a] for a in range(3)], 1).astype(np.float32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def keyframes(world, n, n_frame, distinct, seed):
    poses, _ = scenes.drive(world, n, step=1.5, n_frame=1, seed=seed)
    frames = scenes.map_frames(world, poses[:distinct], n_frame, seed=seed)
    return [np.asarray(p, np.float64) for p in poses], [frames[k % distinct] for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--submaps", type=int, default=64)
    ap.add_argument("--members", type=int, default=11)
    ap.add_argument("--local", type=int, default=25)
    ap.add_argument("--distinct", type=int, default=40)
    ap.add_argument("--leaf", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    out = {}
    world, _ = scenes.scene_parkinglot(n_map=400_000)
    ctx = api.Context(0)
    if "a" not in a.skip:
        for n_frame in (8000, 20000):
            poses, frames = keyframes(world, 24, n_frame, 24, seed=1)
            ctx.keyframes_reset()
            ts = []
            for f in frames:
                ctx.set_source(f)
                t0 = time.perf_counter()
                ctx.keyframes_add_source()
                ts.append((time.perf_counter() - t0) * 1e3)
            assert same(ctx.keyframes_get(23), frames[23])
            out["a_add_source_%dk_ms" % (n_frame // 1000)] = float(np.median(ts[4:]))
    if "b" not in a.skip:
        w = a.members // 2
        n = a.submaps + 2 * w
        poses, frames = keyframes(world, n, 8000, min(a.distinct, n), seed=2)
        ctx.keyframes_reset()
        ctx.keyframes_add(frames)
        # the candidates +- w keyframes, each submap in its candidate's own frame
        members = [[(i, np.linalg.inv(poses[g + w]) @ poses[i]) for i in range(g, g + 2 * w + 1)] for g in range(a.submaps)]

        def host():
            return ctx.voxel_downsample([np.concatenate([transform(frames[i], T) for i, T in sub]) for sub in members], a.leaf)

        got, info = ctx.keyframe_submaps(members, a.leaf)
        want, winfo = host()
        assert info == winfo and all(same(x, y) for x, y in zip(got, want))
        out.update(b_submaps=a.submaps, b_members=2 * w + 1, b_points_in=int(info["n_in"]), b_points_out=int(info["n_out"]))
        out["b_keyframe_submaps_ms"] = timed(lambda: ctx.keyframe_submaps(members, a.leaf), a.repeats)
        out["b_numpy_voxel_downsample_ms"] = timed(host, max(2, a.repeats // 2))
        out["b_raw_ms"] = timed(lambda: ctx.keyframe_submaps(members), a.repeats)
    if "c" not in a.skip or "d" not in a.skip:
        poses, frames = keyframes(world, a.keyframes, 20000, a.distinct, seed=3)
        ctx.keyframes_reset()
        t0 = time.perf_counter()
        for k in range(0, a.keyframes, 50):
            ctx.keyframes_add(frames[k:k + 50])
        out["c_store_fill_ms"] = (time.perf_counter() - t0) * 1e3
        rng = np.random.default_rng(4)
        moved = [T @ scenes.pose6d_matrix(*rng.uniform(-0.05, 0.05, 3), 0.0, 0.0, float(np.deg2rad(rng.uniform(-0.2, 0.2)))) for T in poses]
    if "c" not in a.skip:
        members = list(zip(range(a.keyframes), moved))

        def host():
            return ctx.set_target_voxel(np.concatenate([transform(frames[i], T) for i, T in members]), RADIUS, a.leaf)

        info = ctx.set_target_keyframes(members, RADIUS, a.leaf)
        got = ctx.target_points()
        winfo = host()
        assert info == winfo and same(got, ctx.target_points())
        out.update(c_keyframes=a.keyframes, c_points_in=int(info["n_in"]), c_points_out=int(info["n_out"]))
        out["c_set_target_keyframes_ms"] = timed(lambda: ctx.set_target_keyframes(members, RADIUS, a.leaf), a.repeats)
        out["c_numpy_set_target_voxel_ms"] = timed(host, max(2, a.repeats // 2), warmup=0)
        thinned = ctx.voxel_downsample([np.concatenate([transform(frames[i], T) for i, T in members])], a.leaf)[0][0]
        out["c_set_target_of_the_result_ms"] = timed(lambda: ctx.set_target(thinned, RADIUS), a.repeats)
        # the gather on its own: the raw form straight into device memory
        import ctypes as C
        hip = C.CDLL("libamdhip64.so.7")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        n_in = int(info["n_in"])
        buf = C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), 12 * n_in) == 0
        out["c_gather_raw_device_ms"] = timed(lambda: ctx.keyframe_submaps_device([members], buf.value, n_in), a.repeats * 2, warmup=2)
        hip.hipFree(buf)
    if "d" not in a.skip:
        xy = np.array([T[:2, 3] for T in poses])
        at = list(range(0, a.keyframes, max(1, a.keyframes // 20)))
        near = {k: np.argsort(np.linalg.norm(xy - xy[k], axis=1), kind="stable")[:a.local] for k in at}
        td, th = [], []
        for k in at:
            members = [(int(i), moved[i]) for i in near[k]]
            t0 = time.perf_counter()
            info = ctx.set_target_keyframes(members, RADIUS, a.leaf)
            td.append((time.perf_counter() - t0) * 1e3)
            got = ctx.target_points()
            t0 = time.perf_counter()
            winfo = ctx.set_target_voxel(np.concatenate([transform(frames[i], T) for i, T in members]), RADIUS, a.leaf)
            th.append((time.perf_counter() - t0) * 1e3)
            assert info == winfo and same(got, ctx.target_points())
        out.update(d_local=a.local, d_points_in=int(info["n_in"]), d_points_out=int(info["n_out"]))
        out["d_set_target_keyframes_ms"], out["d_numpy_set_target_voxel_ms"] = float(np.median(td[2:])), float(np.median(th[2:]))
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
