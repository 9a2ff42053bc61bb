"""CPU test of the five-neighbour search (dcreg_amd/csrc/device/search.hpp search5, replayed on the host: tests/host_emul/emul_five.cpp)
against brute force, where it matters: a lattice with duplicated points, queries with exact distance ties at the fifth neighbour.  The
search keeps five entries and prunes at the fifth best distance itself, so a tie between the fifth kept and a point not kept must come
from what the heap turned away - the deferred filter hands it every candidate AT the pruning distance -, and the 64-bit-key search then
picks the canonical five: smallest original index among equal distances."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emul

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
_LIB = os.path.join(_HERE, "libdcreg_emul_five.so")
_SRC = [os.path.join(_HERE, "emul_five.cpp")] + list(emul._SRC)


@pytest.fixture(scope="module")
def lib5():
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(f) for f in _SRC):
        subprocess.check_call([emul.CLANG, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + _HERE, _SRC[0], "-o", _LIB])
    L = C.CDLL(_LIB)
    L.emu_index_build.restype = C.c_void_p
    L.emu_index_build.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]
    L.emu_index_free.argtypes = [C.c_void_p]
    L.emu_search5.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    return L


def _brute5(tgt, q, bound):
    """canonical five under the strict bound: ascending (float distance of the device's chain, original index)"""
    d = q[None, :].astype(np.float32) - tgt                          # float32 throughout, x, y, z in that order, no FMA
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    order = np.lexsort((np.arange(len(tgt)), d2))[:5]
    return [int(i) for i in order if d2[i] < bound], d2


@pytest.mark.parametrize("sweep", [0, 1])
def test_search5_keeps_the_canonical_five_on_a_lattice_with_duplicates(lib5, sweep):
    g = np.arange(0, 9, dtype=np.float32) * np.float32(0.3)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    tgt = np.ascontiguousarray(np.concatenate([lat, lat[::7]]), np.float32)          # every seventh point twice
    rng = np.random.default_rng(5)
    pick = rng.integers(0, len(lat), 300)
    q = np.concatenate([lat[pick],                                                    # on a lattice point: 6 neighbours at one distance
                        lat[pick[:150]] + np.float32(0.15),                           # cell centres: 8 at one distance
                        lat[pick[:150]] + np.array([0.15, 0.0, 0.0], np.float32),     # edge midpoints: 2 + 8 ...
                        lat[pick[:100]] + rng.normal(0, 0.05, (100, 3)).astype(np.float32),
                        lat[:20] - np.float32(0.9)]).astype(np.float32)               # outside: fewer than five inside the bound
    q = np.ascontiguousarray(q)
    radius = 0.7
    bound = np.nextafter(np.float32(radius * radius), np.float32(np.inf))
    idx = lib5.emu_index_build(tgt.ctypes.data_as(C.c_void_p), len(tgt), radius * 1.05, 0.0, 2.0, 1, 8)
    try:
        out_idx = np.empty((len(q), 5), np.int32); out_d2 = np.empty((len(q), 5), np.float32)
        assert lib5.emu_search5(idx, q.ctypes.data_as(C.c_void_p), len(q), C.c_float(float(bound)), sweep, out_idx.ctypes.data_as(C.c_void_p),
                                out_d2.ctypes.data_as(C.c_void_p)) == 0
    finally:
        lib5.emu_index_free(idx)
    tied = short = 0
    for i in range(len(q)):
        want, d2 = _brute5(tgt, q[i], bound)
        got = [int(x) for x in out_idx[i] if x >= 0]
        assert sorted(got) == sorted(want), (i, got, want)
        assert np.array_equal(np.sort(out_d2[i][: len(got)]), np.sort(d2[want])), i
        short += len(want) < 5
        if len(want) == 5:
            tied += int((d2 == d2[want[-1]]).sum() > (d2[want] == d2[want[-1]]).sum())      # a point not kept at the fifth distance
    assert tied > 200 and short >= 10, (tied, short)          # the cases the test is about did occur
