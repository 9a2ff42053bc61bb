"""The scenes the alignment tests share (test_align_reference.py on the CPU, test_gpu_align.py on the device): seeded synthetic point
pairs with a known rigid motion and a known inlier set, and the reference's result for each, computed once per process."""
import functools

import numpy as np

import align_ref

# (M, inlier share, H, scene seed, RANSAC seed): 2 cm noise, d = 0.10, s = 0.9 - the two recovery scenes
RECOVERY = {"m400": (400, 0.30, 4000, 11, 5), "m2000": (2000, 0.10, 50000, 12, 7)}
RECOVERY_D, RECOVERY_S, RECOVERY_NOISE = 0.10, 0.9, 0.02


def rigid(rng, max_angle=np.pi, max_shift=10.0):
    """a random rotation (axis-angle) and translation -> (R [3, 3], t [3]) float64"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    return R, rng.uniform(-max_shift, max_shift, 3)


@functools.lru_cache(maxsize=None)
def synthetic(m, share, noise, seed):
    """m pairs (a[i], b[i]) in a 40 x 40 x 10 m box: the first round(share m) places of a random order are b = R a + t + noise, the
    others unrelated points -> (a, b float32 [m, 3], corr_a, corr_b int32 [m] - the pairs in a shuffled order -, R, t, inlier [m] bool
    by correspondence number)"""
    rng = np.random.default_rng(seed)
    R, t = rigid(rng)
    a = rng.uniform([-20, -20, -5], [20, 20, 5], (m, 3))
    b = rng.uniform([-20, -20, -5], [20, 20, 5], (m, 3)) @ R.T + t
    n_in = int(round(share * m))
    who = rng.permutation(m)[:n_in]
    b[who] = a[who] @ R.T + t + rng.normal(scale=noise, size=(n_in, 3))
    order = rng.permutation(m).astype(np.int32)
    inlier = np.zeros(m, bool)
    inlier[who] = True
    a, b = a.astype(np.float32), b.astype(np.float32)
    for x in (a, b, order):
        x.setflags(write=False)
    return a, b, order, order.copy(), R, t, inlier[order]


@functools.lru_cache(maxsize=None)
def recovery(name):
    """-> (scene tuple of synthetic(), parameter dict, the reference's result)"""
    m, share, n_hyp, scene_seed, seed = RECOVERY[name]
    sc = synthetic(m, share, RECOVERY_NOISE, scene_seed)
    kw = dict(n_hypotheses=n_hyp, seed=seed, inlier_distance=RECOVERY_D, edge_similarity=RECOVERY_S, n_best=1, refine_iterations=3)
    return sc, kw, align_ref.align(sc[0], sc[1], sc[2], sc[3], **kw)


def lattice(n):
    """n distinct points of the 4 x 4 x 4 integer lattice in a seeded order, float32 (many triples are collinear: those hypotheses are
    degenerate, the others tie)"""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    return g[rng.permutation(len(g))[:n]].astype(np.float32)
