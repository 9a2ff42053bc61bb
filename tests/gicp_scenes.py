"""Scenes of the third engine's tests (tests/test_gicp_reference.py, test_emul_glin.py, test_gpu_gicp.py): the scenes of
tests/normal_icp_scenes.py with normals for their SOURCES, the planted flags, and the bitwise comparison of a dump with the reference's.
Everything is computed once per process and never modified."""
import functools

import numpy as np

import normal_icp_scenes as sc
import normals_ref as nr

RADIUS = sc.RADIUS
EPS = 1e-3
DUMP_KEYS = ("nn_idx", "nn_d2", "flag", "normal_map", "normal_src", "w", "r", "row")


@functools.lru_cache(maxsize=None)
def lot():
    """normal_icp_scenes.lot() with the frame's own normals: m5 (k = 5 unbounded: every point has one) and mb (bounded at 0.5: some
    points are sparse), mcur5 / mcurb (the curvatures)"""
    L = dict(sc.lot())
    a, b = nr.normals_reference(L["src"], k=5), nr.normals_reference(L["src"], k=5, search_radius=RADIUS)
    assert a["n_sparse"] == 0 and 0 < b["n_sparse"] < len(L["src"])
    L.update(m5=sc.frozen(a["normals"]), mb=sc.frozen(b["normals"]), mcur5=sc.frozen(a["curvature"]), mcurb=sc.frozen(b["curvature"]))
    return L


def _with_source_normals(case, seed):
    C = dict(case)
    C["src_normals"] = sc.unit_normals(len(C["src"]), seed)
    return C


@functools.lru_cache(maxsize=None)
def lattice_case():
    return _with_source_normals(sc.lattice_case(), 31)


@functools.lru_cache(maxsize=None)
def duplicate_case():
    return _with_source_normals(sc.duplicate_case(), 33)


@functools.lru_cache(maxsize=None)
def outside_case():
    return _with_source_normals(sc.outside_case(), 35)


@functools.lru_cache(maxsize=None)
def sized_source_normals(n):
    """unit normals for normal_icp_scenes.sized_source(n), every 7th point without one"""
    m = np.array(sc.unit_normals(n, 5100 + n))
    m[3::7, 1] = np.nan
    return sc.frozen(m)


# The planted flags on gate_case's map: map point k sits at (10 k, 0, 0) with the normal (0, 0, 1); point 2 has none, point 3 has a
# normal of length 2.  Per source point the flag the rule gives it.
PLANT_MAP = sc.GATE_MAP
PLANT_MAP_NORMALS = np.array([[0, 0, 1], [0, 0, 1], [np.nan, 0, 1], [0, 0, 2], [0, 0, 1]], np.float32)
PLANT_SRC = np.array([[0.5, 0, 0],                # d2 == R*R exactly: stays out
                      [np.nextafter(np.float32(0.5), np.float32(0)), 0, 0],      # the float below: in
                      [10, 0, 0.01],              # the source point has no normal
                      [20.1, 0, 0],               # the nearest map point has no normal
                      [30, 0, 0.1],               # normals of length 2 on both sides: S22 = 2 - 8 c < 0
                      [40, 0, 0.25],              # effective, the source normal tilted
                      [100, 0, 0],                # nothing inside the radius
                      [20.1, 0, 0.05]], np.float32)      # neither side has a normal: the map's is looked at first
PLANT_SRC_NORMALS = np.array([[0, 0, 1], [0, 0, 1], [0, np.inf, 1], [0, 0, 1], [0, 0, 2], [0, 0.6, 0.8], [0, 0, 1], [np.nan, 0, 0]], np.float32)
PLANT_FLAGS = [0, 1, 3, 2, 5, 1, 0, 2]


def plant_case():
    return dict(tgt=PLANT_MAP, normals=PLANT_MAP_NORMALS, src=PLANT_SRC, src_normals=PLANT_SRC_NORMALS, T=np.eye(4), radius=RADIUS)


def assert_dump_bitwise(got, want, what=""):
    for k in DUMP_KEYS:
        assert sc.same_bits(got[k], want[k]), (what, k)
