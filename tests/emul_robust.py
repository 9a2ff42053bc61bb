"""ctypes binding of the HOST REPLAY of the second and third engine's per-point functions with a robust kernel on
(tests/host_emul/emul_robust.cpp: dcreg_amd/csrc/device/normal_icp.hpp and gicp.hpp compiled for the CPU with the shim of
tests/host_emul/, on the index emul.cpp builds).  TEST INFRASTRUCTURE ONLY, a library of its own beside tests/emul_nlin.py's and
tests/emul_glin.py's: the kernels' arithmetic is checked here without a GPU.  Nothing under dcreg_amd/ imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
_DEV = os.path.join(os.path.dirname(_HERE), "..", "dcreg_amd", "csrc", "device")
_LIB = os.path.join(_HERE, "libdcreg_emul_robust.so")
_SRC = [os.path.join(_HERE, "emul_robust.cpp"), os.path.join(_HERE, "emul.cpp"), os.path.join(_HERE, "host_emul_shim.hpp"),
        os.path.join(_DEV, "search.hpp"), os.path.join(_DEV, "normal_icp.hpp"), os.path.join(_DEV, "gicp.hpp")]
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


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
        L.emu_index_build.restype = C.c_void_p
        L.emu_index_build.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]
        L.emu_index_free.argtypes = [C.c_void_p]
        L.emu_hilbert_order.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.emu_nlin_robust.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                      C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 9
        L.emu_glin_robust.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_void_p,
                                      C.c_int] + [C.c_void_p] * 10
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Map:
    """The device's grid index over a map (cells sized for `radius`, or `cell` metres) and its kept normals [n, 3] float32."""

    def __init__(self, xyz, normals, radius, cell=0.0, x_subdiv=8):
        self.xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        n4 = np.full((len(self.xyz), 4), np.nan, np.float32)
        n4[:, :3] = np.asarray(normals, np.float32)[:, :3]
        self.normals4 = np.ascontiguousarray(n4)
        self.ptr = lib().emu_index_build(_ptr(self.xyz), len(self.xyz), float(radius), float(cell), 2.0, 1, int(x_subdiv))

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().emu_index_free(self.ptr)
            self.ptr = None


class Source:
    """A source cloud in the device's processing order, its kept normals [n, 3] float32 in that order (None: the second engine only) and
    its warm words (None: nothing kept yet)."""

    def __init__(self, xyz, normals=None):
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        self.order = np.empty(len(xyz), np.uint32)
        lib().emu_hilbert_order(_ptr(xyz), len(xyz), _ptr(self.order))
        self.sorted = np.ascontiguousarray(xyz[self.order])
        self.normals4 = None
        if normals is not None:
            n4 = np.full((len(xyz), 4), np.nan, np.float32)
            n4[:, :3] = np.asarray(normals, np.float32)[self.order, :3]
            self.normals4 = np.ascontiguousarray(n4)
        self.n = len(xyz)
        self.warm = None


def _pose(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.ascontiguousarray(T[:3, :3]).reshape(9), np.ascontiguousarray(T[:3, 3])


def _words(src, warm):
    have = warm and src.warm is not None
    words = None
    if warm:
        words = src.warm if have else np.full(src.n, 0xA5A5A5A5, np.uint32)      # garbage on purpose: never read without use_warm
    return words, have


def _finish(out, sums, ev, have):
    out.update(H_upper=sums[:21].copy(), g=sums[21:27].copy(), sum_r2=sums[27], sum_b2=sums[28], n_eff=int(round(sums[29])),
               n_pt=int(round(sums[30])), evals=ev.value, warm_used=bool(have))
    return out


def linearize_normals(m, src, T, radius, kind, c, wd=0, warm=True, w_slope=0.9, w_min=0.1):
    """One linearisation through nlin_point on the host with the kernel `kind` at scale c -> the dump (source order), the sums (added in
    processing order) and `evals`.  warm: as tests/emul_nlin.py linearize."""
    R, t = _pose(T)
    n = src.n
    out = {"nn_idx": np.full(n, -1, np.int32), "nn_d2": np.full(n, np.inf, np.float32), "flag": np.zeros(n, np.uint8),
           "normal": np.zeros((n, 3)), "r": np.zeros(n), "s": np.zeros(n), "row": np.zeros((n, 8))}
    sums = np.zeros(31)
    ev = C.c_int64(0)
    words, have = _words(src, warm)
    rc = lib().emu_nlin_robust(m.ptr, _ptr(m.normals4), _ptr(src.sorted), _ptr(src.order), n, _ptr(R), _ptr(t), float(radius), float(w_slope),
                               float(w_min), int(wd), int(kind), float(c), _ptr(words), int(bool(have)), _ptr(out["nn_idx"]), _ptr(out["nn_d2"]),
                               _ptr(out["flag"]), _ptr(out["normal"]), _ptr(out["r"]), _ptr(out["s"]), _ptr(out["row"]), _ptr(sums),
                               C.cast(C.byref(ev), C.c_void_p))
    assert rc == 0
    if warm:
        src.warm = words
    return _finish(out, sums, ev, have)


def linearize_gicp(m, src, T, radius, kind, c, eps=1e-3, warm=True):
    """One linearisation through glin_point / glin_row / glin_row_scale on the host with the kernel `kind` at scale c; as
    tests/emul_glin.py linearize."""
    R, t = _pose(T)
    n = src.n
    out = {"nn_idx": np.full(n, -1, np.int32), "nn_d2": np.full(n, np.inf, np.float32), "flag": np.zeros(n, np.uint8),
           "normal_map": np.zeros((n, 3)), "normal_src": np.zeros((n, 3)), "w": np.zeros((n, 3, 3)), "r": np.zeros((n, 3)),
           "row": np.zeros((n, 3, 8))}
    sums = np.zeros(31)
    ev = C.c_int64(0)
    words, have = _words(src, warm)
    rc = lib().emu_glin_robust(m.ptr, _ptr(m.normals4), _ptr(src.sorted), _ptr(src.normals4), _ptr(src.order), n, _ptr(R), _ptr(t), float(radius),
                               float(eps), int(kind), float(c), _ptr(words), int(bool(have)), _ptr(out["nn_idx"]), _ptr(out["nn_d2"]),
                               _ptr(out["flag"]), _ptr(out["normal_map"]), _ptr(out["normal_src"]), _ptr(out["w"]), _ptr(out["r"]), _ptr(out["row"]),
                               _ptr(sums), C.cast(C.byref(ev), C.c_void_p))
    assert rc == 0
    if warm:
        src.warm = words
    return _finish(out, sums, ev, have)
