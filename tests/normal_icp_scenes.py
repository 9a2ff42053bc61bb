"""Scenes of the second engine's tests (tests/test_normal_icp_reference.py, test_emul_nlin.py, test_gpu_normal_icp.py): the parking lot of
tests/test_gpu_normals.py with its normals, the planted cases, the pose walks, and the bitwise comparison of a dump with the reference's.
Everything is computed once per process and never modified."""
import functools

import numpy as np

import helpers as h
import normal_icp_ref as ref
import normals_ref as nr
from test_normals_reference import lattice

RADIUS = 0.5
DUMP_KEYS = ("nn_idx", "nn_d2", "flag", "normal", "r", "s", "row")
SUM_KEYS = ("H_upper", "g", "sum_r2", "sum_b2", "n_eff", "n_pt")


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def lot():
    """-> dict: tgt, src (523 points), GT, INIT, MID (halfway between them), n5 (k = 5 unbounded normals: every point has one), nb (bounded at
    0.5: 1065 points are sparse), cur5 / curb (the curvatures)"""
    tgt, src = h.scene_parkinglot(n_map=4000, n_frame=1500, extent=12.0, frame_range=5.0)
    mid = {k: 0.5 * (h.PK01_GT[k] + h.PK01_INIT[k]) for k in h.PK01_GT}
    a, b = nr.normals_reference(tgt, k=5), nr.normals_reference(tgt, k=5, search_radius=RADIUS)
    assert len(src) == 523 and a["n_sparse"] == 0 and b["n_sparse"] == 1065
    return dict(tgt=frozen(tgt), src=frozen(src), GT=frozen(h.pose6d_matrix(**h.PK01_GT)), INIT=frozen(h.pose6d_matrix(**h.PK01_INIT)),
                MID=frozen(h.pose6d_matrix(**mid)), n5=frozen(a["normals"]), nb=frozen(b["normals"]), cur5=frozen(a["curvature"]),
                curb=frozen(b["curvature"]))


def offset(T, dx=0.0, dy=0.0, dz=0.0, yaw=0.0):
    """the pose moved by (dx, dy, dz) and turned by yaw about its own position (not about the map's origin, 400 m away from the lot)"""
    out = np.array(T, np.float64)
    out[:3, :3] = h.pose6d_matrix(0.0, 0.0, 0.0, 0.0, 0.0, yaw)[:3, :3] @ out[:3, :3]
    out[:3, 3] += [dx, dy, dz]
    return out


@functools.lru_cache(maxsize=None)
def walk():
    """start, a small step, halfway to the truth, a jump of many cells, back to the start"""
    L = lot()
    return [L["INIT"], frozen(offset(L["INIT"], 0.004, -0.002, 0.001, 1e-4)), L["MID"], frozen(offset(L["INIT"], 3.0, -2.5, 0.2, 0.05)), L["INIT"]]


@functools.lru_cache(maxsize=None)
def sized_source(n):
    """n map points with noise, in the sensor frame of the truth: source sizes across wave and block boundaries"""
    L = lot()
    rng = np.random.default_rng(4100 + n)
    pick = rng.choice(len(L["tgt"]), n, replace=n > len(L["tgt"]))
    w = L["tgt"][pick].astype(np.float64) + rng.normal(0.0, 0.03, (n, 3))
    Ti = np.linalg.inv(L["GT"])
    return frozen((w @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32))


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return frozen((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def lattice_case():
    """a lattice map (spacing exact in float) and queries on its cell midpoints: eight corners tie, the index decides; identity pose"""
    m = lattice((8, 8, 4), 0.25)
    q = (m[(m[:, 0] < 1.75) & (m[:, 1] < 1.75) & (m[:, 2] < 0.75)] + np.float32(0.125)).astype(np.float32)
    return dict(tgt=frozen(m), normals=unit_normals(len(m), 11), src=frozen(q), T=frozen(np.eye(4)), radius=RADIUS)


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """a map most of whose points exist two or three times, queried at its own points and around them"""
    rng = np.random.default_rng(12)
    base = (rng.uniform(-2, 2, (300, 3)) * [1.0, 1.0, 0.3]).astype(np.float32)
    m = np.concatenate([base, base[:200], base[100:300], base[:50]])
    rng.shuffle(m)
    q = np.concatenate([base[::3], (base[1::3] + rng.normal(0, 0.05, base[1::3].shape)).astype(np.float32)])
    return dict(tgt=frozen(np.ascontiguousarray(m)), normals=unit_normals(len(m), 13), src=frozen(np.ascontiguousarray(q)), T=frozen(np.eye(4)),
                radius=RADIUS)


@functools.lru_cache(maxsize=None)
def outside_case():
    """queries inside, just outside and far outside the box of the map's grid"""
    rng = np.random.default_rng(14)
    m = (rng.uniform(-1, 1, (500, 3)) * [1.0, 1.0, 0.2]).astype(np.float32)
    q = (rng.uniform(-1.5, 1.5, (400, 3)) * [1.0, 1.0, 0.4]).astype(np.float32)
    far = np.array([[50.0, 0.0, 0.0], [-1.0e4, 3.0, 0.0], [0.0, 0.0, 1.0e6], [1.3, 1.3, 0.0], [-1.4, 0.0, 0.0]], np.float32)
    return dict(tgt=frozen(m), normals=unit_normals(len(m), 15), src=frozen(np.concatenate([q, far])), T=frozen(np.eye(4)), radius=RADIUS)


# The planted gates, with weight_slope = 2 and 3 (at the default 0.9 a residual inside R = 0.5 cannot reach the weight gate): per source point
# the flag the rule gives it at either slope.  Map point k sits at (10 k, 0, 0) with the normal (0, 0, 1); point 2 has none.
GATE_SLOPES = (2.0, 3.0)
GATE_MAP = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0], [40, 0, 0]], np.float32)
GATE_NORMALS = np.array([[0, 0, 1], [0, 0, 1], [np.nan, 0, 1], [0, 0, 1], [0, 0, 1]], np.float32)
GATE_SRC = np.array([[0.5, 0, 0],                # d2 == R*R exactly: stays out
                     [np.nextafter(np.float32(0.5), np.float32(0)), 0, 0],      # the float below: in, r = 0 (s = 1, no derivative)
                     [10, 0, 0.01],              # effective
                     [20.1, 0, 0],               # the nearest point has no normal
                     [30, 0, 0.475],             # s = 0.05 <= weight_min (slope 3: 1 - 1.425 is clamped at 0)
                     [30, 0, -0.49],             # a negative residual: s = 0.02 (slope 3: clamped at 0 as well)
                     [40, 0, 0.25],              # s = 0.5: effective, the derivative term is active
                     [100, 0, 0]], np.float32)   # nothing inside the radius
GATE_FLAGS = [0, 1, 1, 2, 4, 4, 1, 0]


def gate_case():
    return dict(tgt=GATE_MAP, normals=GATE_NORMALS, src=GATE_SRC, T=np.eye(4), radius=RADIUS)


def same_bits(a, b):
    """bitwise, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def assert_dump_bitwise(got, want, what=""):
    for k in DUMP_KEYS:
        assert same_bits(got[k], want[k]), (what, k)


def assert_sums_bitwise(a, b, what=""):
    for k in SUM_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])) and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def assert_sums_close(got, want, what=""):
    """the tolerances of tests/test_gpu_parity.py against the exactly rounded sums of the reference rows; the counts are exact"""
    assert got["n_eff"] == want["n_eff"] and got["n_pt"] == want["n_pt"], (what, got["n_eff"], want["n_eff"], got["n_pt"], want["n_pt"])
    if want["n_eff"] == 0:
        assert not np.any(got["H_upper"]) and not np.any(got["g"]) and got["sum_r2"] == 0.0 and got["sum_b2"] == 0.0, what
        return
    assert h.rel_err(got["H_upper"], want["H_upper"]) < 1e-9, what
    assert h.rel_err(got["g"], want["g"]) < 1e-8, what
    assert abs(got["sum_r2"] - want["sum_r2"]) <= 1e-10 * max(1.0, want["sum_r2"]), what
    assert abs(got["sum_b2"] - want["sum_b2"]) <= 1e-10 * max(1.0, want["sum_b2"]), what
