"""The debug forms of the two 1-NN engines (dcreg_linearize_normals_debug, dcreg_linearize_gicp_debug) asked for SOME of their arrays: the
runner cuts one block of device memory into the requested arrays from a table of fields, and the Python wrappers always ask for all of
them.  At 257 source points - one full block and one lane, so the second block's other waves carry zero rows - every requested array must
be bitwise the all-fields call's, an array that was not passed must stay as it was, and the 31 sums must be the plain call's."""
import ctypes as C

import numpy as np
import pytest

import exact_sums_scene as ex
import gicp_scenes as gs
import normal_icp_scenes as sc
from dcreg_amd import api

pytestmark = pytest.mark.gpu

N = 257
# (key, dtype, shape per point) in the order of the struct's fields
NLIN_FIELDS = [("nn_idx", np.int32, ()), ("nn_d2", np.float32, ()), ("flag", np.uint8, ()), ("normal", np.float64, (3,)), ("r", np.float64, ()),
               ("s", np.float64, ()), ("row", np.float64, (8,))]
GLIN_FIELDS = [("nn_idx", np.int32, ()), ("nn_d2", np.float32, ()), ("flag", np.uint8, ()), ("normal_map", np.float64, (3,)),
               ("normal_src", np.float64, (3,)), ("w", np.float64, (3, 3)), ("r", np.float64, (3,)), ("row", np.float64, (3, 8))]


def nlin_engine():
    S = ex.scene(N, "cyclic", 1)
    tgt, nrm = ex.lattice_map()
    c = api.Context(0)
    c.set_target(tgt, ex.RADIUS)
    c.set_source(S["src"])
    c.set_target_normals(np.ascontiguousarray(nrm))
    p = api.default_lin_params(ex.RADIUS, 1)
    p.weight_slope, p.weight_min = ex.SLOPE, ex.W_MIN
    return c, S["T"], p, "dcreg_linearize_normals", api.NlinDebug, NLIN_FIELDS


def glin_engine():
    L = gs.lot()
    c = api.Context(0)
    c.set_target(L["tgt"], gs.RADIUS)
    c.set_source(sc.sized_source(N))
    c.set_target_normals(np.ascontiguousarray(L["nb"], np.float32))
    c.set_source_normals(np.ascontiguousarray(gs.sized_source_normals(N), np.float32))
    return c, L["GT"], api.default_lin_params(gs.RADIUS, 1), "dcreg_linearize_gicp", api.GlinDebug, GLIN_FIELDS


def sentinel(dtype, shape):
    a = np.empty((N,) + shape, dtype)
    a.view(np.uint8)[...] = 0xA5
    return a


def call(c, symbol, T, p, struct=None, fields=(), asked=()):
    """-> (the 31 sums, {key: array}); struct None: the plain call.  Every array starts as the sentinel; those of `asked` are passed"""
    R, t = np.ascontiguousarray(T[:3, :3], np.float64).reshape(9), np.ascontiguousarray(T[:3, 3], np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = api.LinOut()
    arrays = {k: sentinel(dt, sh) for k, dt, sh in fields}
    if struct is None:
        rc = getattr(c._L, symbol)(c._h, dp(R), dp(t), C.byref(p), C.byref(out))
    else:
        dbg = struct()                                       # (every pointer null)
        types = dict(struct._fields_)
        for k in asked:
            setattr(dbg, k, arrays[k].ctypes.data_as(types[k]))
        rc = getattr(c._L, symbol + "_debug")(c._h, dp(R), dp(t), C.byref(p), C.byref(out), C.byref(dbg))
    assert rc == 0, (symbol, asked, rc)
    sums = np.concatenate([np.array(out.H_upper), np.array(out.g), [out.sum_r2, out.sum_b2, float(out.n_eff), float(out.n_pt)]])
    return sums, arrays


@pytest.mark.parametrize("engine", [nlin_engine, glin_engine])
def test_a_dump_of_some_fields_is_the_dump_of_all_and_leaves_the_others_alone(engine):
    c, T, p, symbol, struct, fields = engine()
    try:
        keys = [k for k, _, _ in fields]
        plain, _ = call(c, symbol, T, p)
        assert plain[29] > 0 and plain[30] >= plain[29]                      # (the scene has effective points: the sums say something)
        full_sums, full = call(c, symbol, T, p, struct, fields, keys)
        assert sc.same_bits(full_sums, plain), (symbol, "all")
        for k, dt, sh in fields:
            assert not sc.same_bits(full[k], sentinel(dt, sh)), (symbol, k)  # (every array of the full call was written)
        for asked in (["flag", "row"], ["nn_idx", "r"], keys[-1:]):
            sums, got = call(c, symbol, T, p, struct, fields, asked)
            assert sc.same_bits(sums, plain), (symbol, asked)
            for k, dt, sh in fields:
                want = full[k] if k in asked else sentinel(dt, sh)
                assert sc.same_bits(got[k], want), (symbol, asked, k)
        again, _ = call(c, symbol, T, p)                                     # (and the plain call after the dumps: the warm words are untouched)
        assert sc.same_bits(again, plain), (symbol, "after")
    finally:
        c.close()
