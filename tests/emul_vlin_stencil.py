"""ctypes binding of the HOST REPLAY of the fourth engine's per-correspondence functions (tests/host_emul/emul_vlin_stencil.cpp:
dcreg_amd/csrc/device/voxel_icp.hpp compiled for the CPU with the shim of tests/host_emul/).  TEST INFRASTRUCTURE ONLY, a library of its
own beside tests/emul_vlin.py's: the stencil, the neighbour lookups through the table and the rule's arithmetic per correspondence are
checked here without a GPU.  Nothing under dcreg_amd/ imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

from emul_vlin import CLANG, _ptr, records  # noqa: F401  (records: a reference map's 48-byte records)

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
_DEV = os.path.join(os.path.dirname(_HERE), "..", "dcreg_amd", "csrc", "device")
_LIB = os.path.join(_HERE, "libdcreg_emul_vlin_stencil.so")
_SRC = [os.path.join(_HERE, "emul_vlin_stencil.cpp"), os.path.join(_HERE, "emul.cpp"), os.path.join(_HERE, "host_emul_shim.hpp"),
        os.path.join(_DEV, "search.hpp"), os.path.join(_DEV, "normal_icp.hpp"), os.path.join(_DEV, "gicp.hpp"), os.path.join(_DEV, "voxel_icp.hpp")]


def build(force=False):
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(f) for f in _SRC):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + _HERE,
                               _SRC[0], "-o", _LIB])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.emu_hilbert_order.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.emu_vlin_stencil.argtypes = ([C.c_void_p, C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_double, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 9)
        _lib = L
    return _lib


def linearize(rec, coords, box, leaf, src, T, mode=0, src_normals=None, eps=1e-3, kind=0, scale=1.0, neighbors=7):
    """emul_vlin.linearize with S = neighbors correspondences per point through vlin_offset / vmap_find_voxel / vlin_corr / glin_row on the
    host -> the dump with its S axis behind the point axis (source order; also for S = 1) and the sums (added in processing order)"""
    S = int(neighbors)
    src = np.ascontiguousarray(np.asarray(src, np.float32)[:, :3])
    n = len(src)
    order = np.empty(n, np.uint32)
    lib().emu_hilbert_order(_ptr(src), n, _ptr(order))
    srt = np.ascontiguousarray(src[order])
    n4 = None
    if mode:
        n4 = np.full((n, 4), np.nan, np.float32)
        n4[:, :3] = np.asarray(src_normals, np.float32)[order, :3]
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = np.ascontiguousarray(T[:3, :3]).reshape(9), np.ascontiguousarray(T[:3, 3])
    rec = np.ascontiguousarray(rec, np.float32)
    coords = np.ascontiguousarray(coords, np.int64)
    bx = np.ascontiguousarray(np.concatenate([box[0], box[1]]), np.int64)
    out = {"voxel_idx": np.full((n, S), -1, np.int32), "flag": np.zeros((n, S), np.uint8), "mean": np.zeros((n, S, 3)), "cov": np.zeros((n, S, 6)),
           "normal_src": np.zeros((n, 3)), "w": np.zeros((n, S, 3, 3)), "r": np.zeros((n, S, 3)), "row": np.zeros((n, S, 3, 8))}
    sums = np.zeros(31)
    rc = lib().emu_vlin_stencil(_ptr(rec), _ptr(coords), len(coords), float(leaf), _ptr(bx), _ptr(srt), _ptr(n4), _ptr(order), n, _ptr(R), _ptr(t),
                                int(mode), float(eps), int(kind), float(scale), S, _ptr(out["voxel_idx"]), _ptr(out["flag"]), _ptr(out["mean"]),
                                _ptr(out["cov"]), _ptr(out["normal_src"]), _ptr(out["w"]), _ptr(out["r"]), _ptr(out["row"]), _ptr(sums))
    assert rc == 0
    out.update(H_upper=sums[:21].copy(), g=sums[21:27].copy(), sum_r2=sums[27], sum_b2=sums[28], n_eff=int(round(sums[29])),
               n_pt=int(round(sums[30])))
    return out
