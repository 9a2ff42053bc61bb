"""Scenes of the robust kernels' tests (tests/test_robust_reference.py, test_emul_robust.py, test_gpu_robust.py,
test_gpu_robust_batched.py): the lot of tests/normal_icp_scenes.py with a CONTAMINATED frame - a fifth of its points displaced together,
as an object that has moved since the map was built - the kernels, scales and poses the replay and the device are compared at, and the
planted Huber edge.  Everything is computed once per process and never modified."""
import functools

import numpy as np

import gicp_scenes as gs
import normal_icp_scenes as sc
import normals_ref as nr
import robust_ref as rr

RADIUS = sc.RADIUS
KINDS = (1, 2, 3)
SCALES_N = (0.02, 0.1)                  # "robust_scale", metres
SCALES_G = (0.5, 2.0)                   # "gicp_robust_scale", whitened units
GM = rr.KINDS["geman_mcclure"]
C_N, C_G = 0.05, 1.0                    # the scales of the contaminated-frame runs
N_MOVED = 104                           # 20 % of the frame
SHIFT = (0.125, 0.0, 0.25)              # metres, in the sensor frame


@functools.lru_cache(maxsize=None)
def contaminated():
    """-> dict: src (the lot's 523-point frame with the N_MOVED points nearest a seeded frame point moved by SHIFT), moved (their
    indices), m5 (the contaminated frame's own k = 5 normals) and clean_m5 (the clean frame's)"""
    L = gs.lot()
    rng = np.random.default_rng(7)
    seed = int(rng.integers(len(L["src"])))
    d = np.linalg.norm(L["src"].astype(np.float64) - L["src"][seed].astype(np.float64), axis=1)
    moved = np.sort(np.argsort(d, kind="stable")[:N_MOVED])
    src = np.array(L["src"])
    src[moved] = (src[moved].astype(np.float64) + np.array(SHIFT)).astype(np.float32)
    m = nr.normals_reference(src, k=5)
    assert m["n_sparse"] == 0
    return dict(src=sc.frozen(src), moved=sc.frozen(moved), m5=sc.frozen(m["normals"]), clean_m5=L["m5"])


@functools.lru_cache(maxsize=None)
def reference_run(engine, frame, kind):
    """robust_ref.icp_normals / icp_gicp ("NONE", max_iterations 40, the k = 5 normals on both sides) of the contaminated ("dirty") or
    the clean frame from INIT with the kernel `kind` at C_N / C_G -> (T, converged, records); shared by the CPU and the GPU tests"""
    from test_normal_icp_reference import cfg_pk01
    L, S = gs.lot(), contaminated()
    cfg = cfg_pk01(max_iterations=40)
    src, m = (S["src"], S["m5"]) if frame == "dirty" else (L["src"], L["m5"])
    if engine == "normals":
        return rr.icp_normals(L["tgt"], L["n5"], src, L["INIT"], cfg, kind, C_N, "NONE")
    return rr.icp_gicp(L["tgt"], L["n5"], src, m, L["INIT"], cfg, kind, C_G, "NONE", gs.EPS)


def rot_trans_error(T, GT):
    """(metres, degrees) between two poses"""
    d = np.linalg.inv(GT) @ T
    c = min(1.0, max(-1.0, 0.5 * (np.trace(d[:3, :3]) - 1.0)))
    return float(np.linalg.norm(T[:3, 3] - GT[:3, 3])), float(np.degrees(np.arccos(c)))


# The planted Huber edge: a 16-point map on z = 0 (a 4 x 4 lattice, spacing 1 m: exact in float) with the normals (0, 0, 1), the identity
# pose, scale 0.125.  Source points above map points at z = 0, 0.125 and 0.25: r is the height, exactly; u2 = (r*r) / (0.125*0.125) is
# 0, 1 and 4, exactly, so k is 1 (inside), 1 (AT the edge: u <= 1 holds) and sqrt(1 / 2).
EDGE_SCALE = 0.125
EDGE_MAP = np.array([[x, y, 0.0] for x in range(4) for y in range(4)], np.float32)
EDGE_NORMALS = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (16, 1))
EDGE_SRC = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.125], [3.0, 1.0, 0.25]], np.float32)
EDGE_K = (1.0, 1.0, float(np.sqrt(np.float64(0.5))))


@functools.lru_cache(maxsize=None)
def gicp_edge():
    """The same for the third engine, source normals (0, 0, 1): W is diagonal and r_2 = w22 * z.  The height of the edge point is the
    float z for which the REFERENCE gives u2 == 1.0 exactly at scale c = w22 * 0.125 ... found here, on the CPU, by construction: with
    c = r_2(z = 0.125) (a double, passed as the scale) u2 = (r_2*r_2) / (c*c) is exactly 1.  -> dict: src, src_normals, c, k"""
    m = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (3, 1))
    probe = rr.linearize_gicp(EDGE_MAP, EDGE_NORMALS, EDGE_SRC, m, np.eye(4), RADIUS, 0, 1.0, gs.EPS)
    assert (probe["flag"] == 1).all() and not probe["r"][:, :2].any()
    c = float(probe["r"][1, 2])                             # the whitened height of the middle point: the scale that puts it AT the edge
    k, u2 = rr.point_factors_gicp(probe, 1, c)
    assert u2[0] == 0.0 and u2[1] == 1.0 and u2[2] > 1.0
    return dict(src=EDGE_SRC, src_normals=m, c=c, k=tuple(float(x) for x in k))
