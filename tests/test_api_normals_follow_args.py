"""Kept normals that follow the map, the binding without a device: the info block against the header and dcreg_sizeof, the exports, the
refusals of the C-ABI that need no context, and the arguments the Context methods check before anything reaches the library."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

NEW = ("dcreg_target_normals_get", "dcreg_target_normals_get_device", "dcreg_target_normals_follow_info")


def test_the_info_block_matches_the_header_and_every_symbol_is_exported():
    L = api.load()
    assert [f[0] for f in api.NormalsFollowInfo._fields_] == ["n_target", "n_refit", "n_carried", "followed", "reserved_"]
    assert C.sizeof(api.NormalsFollowInfo) == 32 and L.dcreg_sizeof(b"dcreg_normals_follow_info") == 32
    assert api._STRUCTS["dcreg_normals_follow_info"] is api.NormalsFollowInfo
    for name in NEW:
        assert name in api.EXPORTS and hasattr(L, name), name
    for name in ("kept_target_normals", "normals_follow_info"):
        assert callable(getattr(api.Context, name)), name


def test_the_c_abi_refuses_a_null_context_and_a_null_info():
    L = api.load()
    out = np.full((4, 4), 7.0, np.float32)
    info = api.NormalsFollowInfo()
    info.n_refit = 5
    assert L.dcreg_target_normals_get(None, out.ctypes.data, 4) == api.E_INVALID
    assert L.dcreg_target_normals_get(None, None, 0) == api.E_INVALID
    assert L.dcreg_target_normals_get_device(None, None, 4) == api.E_INVALID
    assert L.dcreg_target_normals_follow_info(None, C.byref(info)) == api.E_INVALID
    assert L.dcreg_target_normals_follow_info(None, None) == api.E_INVALID
    assert (out == 7.0).all() and info.n_refit == 5              # nothing was written


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def test_the_device_getter_checks_its_capacity_first():
    c = _ctx()
    for bad in (None, -1, 1 << 31, 2.5, True):
        with pytest.raises(ValueError, match="capacity"):
            c.kept_target_normals(dev_ptr=16, capacity=bad)
    with pytest.raises(ValueError, match="dev_ptr"):
        c.kept_target_normals(capacity=4)       # a capacity means the device form
