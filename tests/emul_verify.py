"""ctypes binding of the HOST REPLAY of the verification call's per-point function (tests/host_emul/emul_verify.cpp:
dcreg_amd/csrc/device/verify.hpp compiled for the CPU with the shim of tests/host_emul/, on the index emul.cpp builds).  TEST
INFRASTRUCTURE ONLY, a library of its own beside tests/emul.py's: the bounded search from the start key, the strict gate and the integer
term are checked here without a GPU.  Nothing under dcreg_amd/ imports it."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
_DEV = os.path.join(os.path.dirname(_HERE), "..", "dcreg_amd", "csrc", "device")
_LIB = os.path.join(_HERE, "libdcreg_emul_verify.so")
_SRC = [os.path.join(_HERE, "emul_verify.cpp"), os.path.join(_HERE, "emul.cpp"), os.path.join(_HERE, "host_emul_shim.hpp"),
        os.path.join(_DEV, "search.hpp"), os.path.join(_DEV, "normal_icp.hpp"), os.path.join(_DEV, "verify.hpp")]
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
        L.emu_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 5
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Map:
    """The device's grid index over a map (cells sized for `radius`, or `cell` metres)."""

    def __init__(self, xyz, radius, cell=0.0, x_subdiv=8):
        self.xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        self.ptr = lib().emu_index_build(_ptr(self.xyz), len(self.xyz), float(radius), float(cell), 2.0, 1, int(x_subdiv))

    def __del__(self):
        if getattr(self, "ptr", None):
            lib().emu_index_free(self.ptr)
            self.ptr = None


def verify(m, cloud, Ts, d):
    """verify_point for every (pose, point) of a finite cloud -> dict inl [P, n] uint8, nn [P, n] int32, d2 [P, n] float32, e [P, n] uint64,
    count [P], cost [P] (Python ints) and evals"""
    pts = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    Ts = np.asarray(Ts, np.float64).reshape(-1, 4, 4)
    P, n = len(Ts), len(pts)
    table = np.ascontiguousarray(np.concatenate([Ts[:, :3, :3].reshape(P, 9), Ts[:, :3, 3]], axis=1))
    out = {"inl": np.zeros((P, n), np.uint8), "nn": np.zeros((P, n), np.int32), "d2": np.zeros((P, n), np.float32), "e": np.zeros((P, n), np.uint64)}
    ev = C.c_int64(0)
    rc = lib().emu_verify(m.ptr, _ptr(pts), n, _ptr(table), P, float(d), _ptr(out["inl"]), _ptr(out["nn"]), _ptr(out["d2"]), _ptr(out["e"]),
                          C.cast(C.byref(ev), C.c_void_p))
    assert rc == 0
    out["count"] = [int(r.sum()) for r in out["inl"]]
    out["cost"] = [sum(int(v) for v in r) for r in out["e"]]
    out["evals"] = ev.value
    return out
