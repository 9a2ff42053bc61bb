"""The scenes the consensus tests share (test_consensus_reference.py on the CPU, test_gpu_consensus.py on the device): align_scenes'
synthetic pairs and lattice at the low inlier shares the graph is for, and the reference's result for each, computed once per process."""
import functools

import numpy as np

import align_ref as ar
import align_scenes as sc
import consensus_ref as cr

# 2 cm noise, compatibility 0.10 m, minimum length 1.0 m, 64 seeds, sets of at most 16, d = 0.10
NOISE = 0.02
SETTINGS = dict(compat_distance=0.10, min_length=1.0, inlier_distance=0.10, n_seeds=64, consensus_size=16, n_best=1, refine_iterations=3)
# (M, inlier share, scene seed)
RECOVERY = {"m1000": (1000, 0.01, 40), "m2000": (2000, 0.005, 43)}
# where align_ref.align at H = 10^5, s = 0.9 returns a record with one inlier, RANSAC seeds 7, 1 and 2
SAMPLER_FAILS = {"m2000": (2000, 0.01, 22), "m1000": (1000, 0.01, 31)}
SAMPLER_SEEDS = (7, 1, 2)


def scene(m, share, seed):
    return sc.synthetic(m, share, NOISE, seed)


@functools.lru_cache(maxsize=None)
def solved(kind, name):
    """kind "recovery" or "fails" -> (scene tuple of synthetic(), the settings, the reference's result)"""
    m, share, seed = (RECOVERY if kind == "recovery" else SAMPLER_FAILS)[name]
    s = scene(m, share, seed)
    return s, dict(SETTINGS), cr.consensus(s[0], s[1], s[2], s[3], **SETTINGS)


@functools.lru_cache(maxsize=None)
def dense(m, seed):
    """every pair true and exact: b = a @ R.T + t in float32 with no noise term -> (a, b, corr_a, corr_b)"""
    a, _, ca, cb, R, t, _ = sc.synthetic(m, 1.0, 0.0, seed)
    b = (a @ R.T + t).astype(np.float32)
    b.setflags(write=False)
    return a, b, ca, cb


@functools.lru_cache(maxsize=None)
def rotated_lattice(n, wrong):
    """the lattice points against a copy of themselves turned a quarter about z and shifted - exact in float32, many equal lengths -,
    the last `wrong` pairs matched to another point of the copy -> (a, b, corr_a, corr_b)"""
    g = sc.lattice(n)
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    b = (g @ Rz.T + np.array([5.0, -3.0, 2.0], np.float32)).astype(np.float32)
    ia, ib = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    if wrong:
        ib[-wrong:] = np.roll(ib[-wrong:], 3)
    return g, b, ia, ib


@functools.lru_cache(maxsize=None)
def hinge(k=4):
    """Two pairs s, v on an axis and k pairs x_i turned about that axis by different angles between a and b: every x_i keeps its lengths
    to s and v and none to another x_j, so the graph is K(2, k) plus the edge s - v.  S(s, v) = k and S(s, x_i) = 1: for k >= 3 the seeds
    s and v (w = 2 k) have one candidate and are skipped, the x_i (w = 2) have s and v and are scored.  In front of them five pairs far
    away that are shifted as one: a clique with w = 12 each, compatible with nothing else -> (a, b, corr_a, corr_b): the clique is pairs
    0 .. 4, s and v are 5 and 6, the x_i follow"""
    a = [[50.0, 0.0, 0.0], [53.0, 1.0, 0.0], [51.0, 4.0, 1.0], [55.0, -2.0, 2.0], [52.0, -3.0, -2.0]]
    b = [[x, y, z + 30.0] for x, y, z in a]
    a += [[0.0, 0.0, 0.0], [0.0, 0.0, 4.0]]
    b += [[0.0, 0.0, 0.0], [0.0, 0.0, 4.0]]
    for i in range(k):
        r, z, th = 3.0 + 0.7 * i, 0.5 + 0.9 * i, 1.3 * (i + 1)
        a.append([r, 0.0, z])
        b.append([r * np.cos(th), r * np.sin(th), z])
    idx = np.arange(k + 7, dtype=np.int32)
    return np.asarray(a, np.float32), np.asarray(b, np.float32), idx, idx.copy()


def seed_sets(a, b, corr_a, corr_b, compat_distance, min_length, n_seeds, consensus_size, **_):
    """steps 1 to 4 with the reference's own functions -> the number of members of every seed, by rank"""
    m_of_u, p, q = ar.used_pairs(a, b, corr_a, corr_b)
    ia, ib = np.asarray(corr_a, np.int64)[m_of_u], np.asarray(corr_b, np.int64)[m_of_u]
    C = cr.compatibility(p, q, ia, ib, float(compat_distance), float(min_length))
    S = cr.second_order(C)
    seeds = np.lexsort((np.arange(len(p)), -S.sum(axis=1)))[:min(n_seeds, len(p))]
    return [int(cr.members_of(C, S, s, consensus_size).size) for s in seeds.tolist()]


def pose_error(T, R, t):
    """-> (translation error in metres, rotation error in degrees) of the 4x4 T against (R, t)"""
    dR = T[:3, :3] @ R.T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(T[:3, 3] - t)), float(ang)
