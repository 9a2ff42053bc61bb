"""The kept voxel map that follows the map, the binding without a device: the info block against the header and dcreg_sizeof, the export,
the refusals of the C-ABI that need no context, and the two options by name."""
import ctypes as C

from dcreg_amd import api

FIELDS = ["n_target", "n_touched", "n_refit", "n_carried", "n_kept", "followed", "reserved_"]


class _Ctx(C.Structure):
    """a zeroed block of memory stands in for a context: set_option writes its options, a refusal leaves its text in it"""
    _fields_ = [("bytes", C.c_char * (1 << 16))]


def test_the_info_block_matches_the_header_and_the_symbol_is_exported():
    L = api.load()
    assert [f[0] for f in api.VoxelsFollowInfo._fields_] == FIELDS
    assert C.sizeof(api.VoxelsFollowInfo) == 48 and L.dcreg_sizeof(b"dcreg_voxels_follow_info") == 48
    assert api._STRUCTS["dcreg_voxels_follow_info"] is api.VoxelsFollowInfo
    assert "dcreg_target_voxels_follow_info" in api.EXPORTS and hasattr(L, "dcreg_target_voxels_follow_info")
    assert callable(api.Context.voxels_follow_info)
    header = open(api.os.path.join(api._HERE, "..", "include", "dcreg.h")).read()
    assert "int64_t n_target, n_touched, n_refit, n_carried, n_kept;\n    int followed;\n    int reserved_;\n} dcreg_voxels_follow_info;" in header


def test_the_c_abi_refuses_a_null_context_and_a_null_info():
    L = api.load()
    info = api.VoxelsFollowInfo()
    info.n_refit, info.followed = 5, 7
    blob = _Ctx()
    assert L.dcreg_target_voxels_follow_info(None, C.byref(info)) == api.E_INVALID
    assert L.dcreg_target_voxels_follow_info(None, None) == api.E_INVALID
    assert L.dcreg_target_voxels_follow_info(C.c_void_p(C.addressof(blob)), None) == api.E_INVALID
    assert info.n_refit == 5 and info.followed == 7              # nothing was written


def test_the_options_are_accepted_by_name():
    L = api.load()
    blob = _Ctx()
    ctx = C.c_void_p(C.addressof(blob))
    for value in (1.0, 0.0):
        assert L.dcreg_set_option(ctx, b"voxels_follow", C.c_double(value)) == api.OK
    for value in (0.0, 0.25, 1.0, -3.0, 7.0):                    # (clamped to 0 .. 1, never refused)
        assert L.dcreg_set_option(ctx, b"voxels_follow_full_share", C.c_double(value)) == api.OK
    assert L.dcreg_set_option(ctx, b"voxels_follows", C.c_double(1.0)) == api.E_INVALID
    info = api.VoxelsFollowInfo()
    info.followed = 7
    assert L.dcreg_target_voxels_follow_info(ctx, C.byref(info)) == api.OK
    assert [int(getattr(info, f)) for f in FIELDS] == [0] * 7     # no update yet
