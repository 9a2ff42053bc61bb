"""A scene of the second engine (dcreg_linearize_normals) whose 31 sums are EXACT in double whatever the order of the additions: every
row entry is a small multiple of 2^-9, every product a multiple of 2^-18, and the sum of the absolute values of a slot's products stays
below 2^53 * 2^-18.  No addition of such terms ever rounds, so wave sums, block rows, chunk sums and the result row must give
math.fsum's value bit for bit, at every size.

  map      the integer lattice 16 x 16 x 4, spacing 1;
  normals  components from {-1, -0.5, 0, 0.5, 1}, not all zero (seeded);
  pose     R a signed permutation of determinant +1 (ROTATIONS), t = (3, -2, 1);
  world    a seeded lattice point plus k/8 per axis, k in -3 .. 3: its nearest map point is that lattice point, without a tie;
  source   R^T (world - t), exact in float32;
  params   search_radius 1, weight_slope 0.5, weight_min 0.1, the weight derivative off and on.
Then e = k/8, r = n.e is a multiple of 1/16 with |r| <= 9/8, s = 1 - |r|/2 >= 7/16 a multiple of 1/32, w = s + r ds likewise,
m = R^T n in halves, p in eighths: w (p x m) is a multiple of 2^-9, and so is b = -(s r).  scene() asserts all of this on the CPU."""
import functools

import numpy as np

import normal_icp_ref as ref

ROTATIONS = {"rz90": [[0, -1, 0], [1, 0, 0], [0, 0, 1]], "cyclic": [[0, 0, 1], [1, 0, 0], [0, 1, 0]], "swap_xy": [[0, 1, 0], [1, 0, 0], [0, 0, -1]]}
T_VEC = (3.0, -2.0, 1.0)
RADIUS, SLOPE, W_MIN = 1.0, 0.5, 0.1
SIZES = [1, 64, 255, 257, 4099, 16385, 32769]


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def lattice_map():
    """-> (map [1024, 3] float32, normals [1024, 3] float32)"""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(2024)
    nrm = rng.integers(-2, 3, (len(g), 3))
    zero = ~nrm.any(axis=1)
    nrm[zero, 2] = 2
    assert nrm.any(axis=1).all() and (nrm == 0).any() and (np.abs(nrm) == 1).any()
    return frozen(g), frozen((nrm * 0.5).astype(np.float32))


def pose(rotation):
    T = np.eye(4)
    T[:3, :3] = np.array(ROTATIONS[rotation], np.float64)
    T[:3, 3] = T_VEC
    assert round(np.linalg.det(T[:3, :3])) == 1 and np.array_equal(np.abs(T[:3, :3]).sum(axis=0), [1, 1, 1])
    return frozen(T)


@functools.lru_cache(maxsize=None)
def scene(n, rotation, wd):
    """-> dict: tgt, normals, src [n, 3] float32, T, want (the reference linearisation: its sums are math.fsum's over exact products)"""
    tgt, nrm = lattice_map()
    T = pose(rotation)
    rng = np.random.default_rng(77 + n)
    at = rng.integers(0, len(tgt), n)
    q = tgt[at].astype(np.float64) + rng.integers(-3, 4, (n, 3)) / 8.0
    p64 = (q - T[:3, 3]) @ T[:3, :3]                    # R^T (q - t), row-wise
    src = p64.astype(np.float32)
    assert np.array_equal(src.astype(np.float64), p64)
    # the premises
    assert np.array_equal(ref.transform(T[:3, :3], T[:3, 3], src).astype(np.float64), q)                 # the world points come back exactly
    want = ref.linearize(tgt, nrm, src, T, RADIUS, weight_slope=SLOPE, weight_min=W_MIN, use_weight_derivative=wd)
    assert (want["flag"] == 1).all() and np.array_equal(want["nn_idx"], at) and want["n_eff"] == n == want["n_pt"]
    scaled = want["row"] * 512.0
    assert np.array_equal(scaled, np.rint(scaled)) and np.abs(scaled).max() < 2.0 ** 20                   # rows * 2^9 are integers
    rows = scaled.astype(np.int64)
    pairs = [(a, b) for a in range(6) for b in range(a, 6)] + [(a, 6) for a in range(6)] + [(7, 7), (6, 6)]
    worst = max(int(np.abs(rows[:, a] * rows[:, b]).sum()) for a, b in pairs)
    assert worst < 2 ** 53, worst                                                                         # no partial sum can round
    # ... so the exact integer sums, scaled back, are the reference's sums: a check of the yardstick itself
    ints = [int((rows[:, a] * rows[:, b]).sum()) for a, b in pairs]
    have = np.concatenate([want["H_upper"], want["g"], [want["sum_r2"], want["sum_b2"]]])
    assert np.array_equal(have, np.array([v / 2.0 ** 18 for v in ints]))
    if n >= 64:
        assert (want["r"] > 0.0).any() and (want["r"] < 0.0).any() and (want["r"] == 0.0).any()         # s < 1 and s == 1: both weight branches
    for v in want.values():
        if isinstance(v, np.ndarray):
            frozen(v)
    return dict(tgt=tgt, normals=nrm, src=frozen(src), T=T, want=want, worst_log2=float(np.log2(max(worst, 1))))
