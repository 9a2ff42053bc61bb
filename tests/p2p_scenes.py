"""The scenes of the dcreg_p2p_error tests (test_p2p_reference.py pins the numpy reference against the oracle on them and asserts that
each still exercises its edge; test_gpu_p2p_error.py runs the device on them).  A scene is a dict: name, kind, src (body frame), tgt
(map frame), T (4x4) and thrs (the error thresholds it is run at).  Every cloud has at most 4000 points."""
import functools

import numpy as np

import helpers as h
import p2p_ref as pr


def axis_angle_pose(axis, angle, t):
    """Rodrigues' formula -> 4x4"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def _exact_pose():
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]     # 90 degrees about z
    T[:3, 3] = [8.0, -4.0, 0.5]
    return T


POSES = {
    "identity": np.eye(4),
    "near": h.pose6d_matrix(0.03, -0.02, 0.01, h.deg2rad(0.2), h.deg2rad(-0.1), h.deg2rad(0.4)),
    "exact": _exact_pose(),
    "large": axis_angle_pose((1.0, 2.0, 3.0), 2.5, (120.0, -340.0, 15.0)),
}

# (ns, nt) of the reduction scenes: kBlock is 256 and a wave is 64; every size appears once as ns and once as nt
REDUCTION_SIZES = (1, 2, 4, 63, 64, 65, 255, 256, 257, 513)
REDUCTION_SHAPES = ((1, 513), (513, 1), (256, 256), (2, 257), (257, 2), (4, 255), (255, 4), (63, 65), (65, 64), (64, 63))

TIE_DISTANCE = 0.125
TIE_DISTANCE_2 = 0.15625      # |(3, 4, 0)| / 32
TIE_OFFSETS = ((0.0, 0.0, 0.0), (0.125, 0.0, 0.0), (0.0, 0.125, 0.0), (0.0625, 0.0625, 0.0), (0.0, 0.0, 0.03125), (0.09375, 0.125, 0.0),
               (0.125, 0.125, 0.0), (0.125, 0.125, 0.125))
TIE_THRESHOLDS = (TIE_DISTANCE, float(np.nextafter(TIE_DISTANCE, np.inf)), float(np.nextafter(TIE_DISTANCE, -np.inf)),
                  TIE_DISTANCE_2, float(np.nextafter(TIE_DISTANCE_2, np.inf)), 0.0, -1.0, float("inf"))


def to_body(T, pts_map):
    """float32: T^-1 applied to map-frame points - a source whose aligned cloud lies where pts_map lies"""
    return pr.transform_exact(pr.rigid_inverse(T), np.asarray(pts_map, np.float32)).astype(np.float32)


def surface_target(n=3000, seed=21):
    """the noisy surface patch the asymmetric, degenerate and state scenes share as their map"""
    return h.scene_cylinder(n, seed=seed, noise=0.01)


def half_cover(tgt, n, n_off, seed, side=1.0):
    """map-frame points: n - n_off noisy copies of target points of the half x > 0 (side -1: x < 0), and n_off points well off the surface"""
    rng = np.random.default_rng(seed)
    half = np.flatnonzero(side * tgt[:, 0] > 0)
    on = tgt[rng.choice(half, n - n_off, replace=False)].astype(np.float64) + rng.normal(0, 0.02, (n - n_off, 3))
    off = tgt[rng.choice(half, n_off, replace=False)].astype(np.float64)
    off[:, :2] *= 0.8                                   # up to 8 m inside the wall
    off[:, 2] += 5.0                                    # and 5 m above the floor
    return np.concatenate([on, off]).astype(np.float32)


def asymmetric_pair(pose, swapped=False):
    T = POSES[pose]
    big = surface_target()
    small = half_cover(big, 700, 40, seed=22)
    src_map, tgt = (big, small) if swapped else (small, big)
    return dict(name="asym_%s%s" % (pose, "_swapped" if swapped else ""), kind="asym", pose=pose, src=to_body(T, src_map), tgt=tgt, T=T,
                thrs=(0.05,))


def tie_scene():
    T = POSES["exact"]
    g = np.arange(0, 12, dtype=np.float32) * 0.25
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(23)
    parts = []
    for k, off in enumerate(TIE_OFFSETS):
        parts.append(tgt[rng.choice(len(tgt), 30 + 3 * k, replace=False)] + np.asarray(off, np.float32))
    return dict(name="ties", kind="ties", pose="exact", src=to_body(T, np.concatenate(parts)), tgt=tgt, T=T, thrs=TIE_THRESHOLDS)


def reduction_scene(ns, nt):
    rng = np.random.default_rng(1000 * ns + nt)
    T = POSES["near"]
    return dict(name="reduce_%d_%d" % (ns, nt), kind="reduce", pose="near", src=rng.uniform(0, 2, (ns, 3)).astype(np.float32),
                tgt=rng.uniform(0, 2, (nt, 3)).astype(np.float32), T=T, thrs=(0.3,))


DEGENERATE = ("identical", "collinear", "coplanar", "single")


def degenerate_scene(what, pose):
    """sources whose auxiliary grid degenerates, built in the BODY frame around the body-frame image of a point of the map"""
    T = POSES[pose]
    tgt = surface_target()
    far = int(np.argmax(np.hypot(tgt[:, 0], tgt[:, 1])))            # a point of the wall, 40 m from the map's origin
    p0 = to_body(T, tgt[far:far + 1])[0]
    rng = np.random.default_rng(24)
    n = 300
    if what == "identical":
        src = np.repeat(p0[None, :], n, axis=0)
    elif what == "collinear":
        src = np.repeat(p0[None, :], n, axis=0)
        src[:, 0] += rng.uniform(0, 30, n).astype(np.float32)
    elif what == "coplanar":
        src = np.repeat(p0[None, :], n, axis=0)
        src[:, :2] += rng.uniform(-15, 15, (n, 2)).astype(np.float32)
    else:
        src = p0[None, :].copy()
    return dict(name="degenerate_%s_%s" % (what, pose), kind="degenerate", what=what, pose=pose, src=src.astype(np.float32), tgt=tgt, T=T,
                thrs=(2.0,))


@functools.lru_cache(maxsize=None)
def all_scenes():
    out = [asymmetric_pair(p, sw) for p in POSES for sw in (False, True)]
    out.append(tie_scene())
    out += [reduction_scene(ns, nt) for ns, nt in REDUCTION_SHAPES]
    out += [degenerate_scene(w, p) for w in DEGENERATE for p in ("near", "large")]
    for s in out:
        s["src"] = np.ascontiguousarray(s["src"], np.float32)
        s["tgt"] = np.ascontiguousarray(s["tgt"], np.float32)
        s["src"].setflags(write=False)
        s["tgt"].setflags(write=False)
        assert len(s["src"]) <= 4000 and len(s["tgt"]) <= 4000
    return tuple(out)


def scene_names():
    return [s["name"] for s in all_scenes()]


def scene(name):
    return next(s for s in all_scenes() if s["name"] == name)


def oracle_of(src, tgt, T, thrs):
    """the oracle (po.p2p_error) on a pair of clouds: per threshold (rmse, fitness, chamfer, valid), plus its forward and backward means
    taken from its own k-NN, as orc_p2p_error takes them"""
    from oracle import pyoracle as po
    aligned = pr.transform(T, src)
    tree = po.KdTree(tgt)
    per_thr = {thr: po.p2p_error(aligned, tree, thr) for thr in thrs}
    _, fd2 = tree.knn(aligned, k=1)
    _, bd2 = po.KdTree(aligned).knn(tgt, k=1)
    fwd = float(np.sum(np.sqrt(fd2.reshape(-1)).astype(np.float64)) / len(aligned))
    bwd = float(np.sum(np.sqrt(bd2.reshape(-1)).astype(np.float64)) / len(tgt))
    return dict(thr=per_thr, fwd_mean=fwd, bwd_mean=bwd)


def reference_of(src, tgt, T, thrs):
    """the numpy reference of a pair of clouds: per threshold the p2p_exact dict, plus the exact backward mean and the two bounds"""
    aligned = pr.transform(T, src)
    exact_bwd = pr.p2p_exact_rigid(src, T, tgt)
    bound_dev, bound_ref = pr.backward_bounds(src, T, tgt, exact_bwd)
    base = pr.p2p_exact(aligned, tgt, thrs[0])
    per_thr = {thr: pr.p2p_exact_thr(base, thr) for thr in thrs}       # (only the thresholded part changes)
    return dict(aligned=aligned, exact_bwd=exact_bwd, bound_dev=bound_dev, bound_ref=bound_ref, thr=per_thr)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """oracle_of a scene, computed once"""
    s = scene(name)
    return oracle_of(s["src"], s["tgt"], s["T"], s["thrs"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_of a scene, computed once"""
    s = scene(name)
    return reference_of(s["src"], s["tgt"], s["T"], s["thrs"])
