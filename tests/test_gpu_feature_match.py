"""Feature-space matching on the device (dcreg_feature_match*) against the brute-force matcher of tests/fpfh_ref.py, which applies
include/dcreg.h's rule literally: indices, distances (doubles, bitwise), second-best, mutual flags and counts must be the reference's
whatever the sizes, the LDS tile and the split of the candidates over blocks."""
import ctypes as C

import numpy as np
import pytest

import fpfh_ref as fr
from dcreg_amd import api
from test_fpfh_reference import lot_cloud, moved_copy
from test_gpu_device_seam import D2H, DevCloud, hip

pytestmark = pytest.mark.gpu

TILE = 128                       # candidate rows per LDS tile of k_match (features.hip kMatchTile)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def rows(n, seed=0, width=33):
    """histogram-like rows: non-negative floats, many of them zero"""
    rng = np.random.default_rng(900 + seed + 7 * n)
    a = rng.uniform(0.0, 100.0, (n, width)) * (rng.uniform(size=(n, width)) < 0.6)
    return a.astype(np.float32)


def same_f64(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def assert_match(got, ref, what=""):
    for key in ("idx", "idx2", "mutual"):
        assert np.array_equal(got[key], ref[key]), (what, key)
    for key in ("d", "d2"):
        assert same_f64(got[key], ref[key]), (what, key)
    for key in ("n_a_valid", "n_b_valid", "n_mutual"):
        assert got[key] == ref[key], (what, key, got[key], ref[key])


SIZES = [0, 1, 2, 63, 64, 65, 257]


@pytest.mark.parametrize("n_a", SIZES)
def test_sizes_across_wave_and_block_boundaries(ctx, n_a):
    a = rows(n_a, 1)
    for n_b in SIZES:
        b = rows(n_b, 2)
        got = ctx.feature_match(a, b)
        if n_a == 0:                           # (a call without queries does nothing: no output, the info all zero)
            assert all(len(got[key]) == 0 for key in ("idx", "d", "idx2", "d2", "mutual")) and got["n_a_valid"] == got["n_b_valid"] == got["n_mutual"] == 0
            continue
        assert_match(got, fr.match_reference(a, b), (n_a, n_b))


@pytest.mark.parametrize("n_b", [TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE + 5])
def test_candidates_around_the_tile_size(ctx, n_b):
    a, b = rows(200, 3), rows(n_b, 4)
    assert_match(ctx.feature_match(a, b), fr.match_reference(a, b), n_b)


def test_the_result_does_not_depend_on_the_split(ctx):
    a, b = rows(300, 5), rows(3000, 6)
    b[1500:1510] = b[20:30]                    # equal distances on both sides of every split below
    b[2999] = b[0]
    a[:40] = b[np.r_[20:30, 1500:1510, 0:20]]
    ref = fr.match_reference(a, b)
    assert np.all(ref["d"][:40] == 0.0) and np.array_equal(ref["idx"][:10], np.arange(20, 30)) and np.array_equal(ref["idx2"][:10], np.arange(1500, 1510))
    assert ref["idx"][20] == 0 and ref["idx2"][20] == 2999
    c = api.Context(0)
    try:
        for split in (0, 1, TILE - 1, TILE, 1000, 1499, 5000):
            c.set_option("feature_match_split", split)
            assert_match(c.feature_match(a, b), ref, split)
    finally:
        c.close()


def test_repeated_rows_nan_rows_and_rows_that_are_all_invalid(ctx):
    a, b = rows(150, 7), rows(400, 8)
    b[100:104] = b[3]                          # ties go to the lowest index, second = first at D = 0
    a[0] = b[3]
    a[5, 32], a[77, 0], b[9, 16], b[399, 1] = np.nan, np.inf, np.nan, -np.inf
    b[200] = a[5]
    ref = fr.match_reference(a, b)
    assert ref["idx"][0] == 3 and ref["idx2"][0] == 100 and ref["d"][0] == ref["d2"][0] == 0.0
    assert ref["idx"][5] == -1 and np.isnan(ref["d"][77]) and (ref["n_a_valid"], ref["n_b_valid"]) == (148, 397)
    got = ctx.feature_match(a, b)
    assert_match(got, ref, "nan rows")
    dead = np.full((50, 33), np.nan, np.float32)
    for x, y in ((a, dead), (dead, b), (dead, dead)):
        ref = fr.match_reference(x, y)
        assert np.all(ref["idx"] == -1) and ref["n_mutual"] == 0
        assert_match(ctx.feature_match(x, y), ref, "all invalid")


def test_one_valid_candidate_has_no_second(ctx):
    a, b = rows(70, 9), rows(5, 10)
    b[[0, 1, 3, 4], 2] = np.nan
    ref = fr.match_reference(a, b)
    assert np.all(ref["idx"] == 2) and np.all(ref["idx2"] == -1) and np.all(np.isinf(ref["d2"])) and ref["n_mutual"] == 1
    assert_match(ctx.feature_match(a, b), ref, "one candidate")


def test_optional_outputs_strided_rows_and_the_device_form(ctx):
    a, b = rows(130, 11, 40), rows(260, 12, 35)
    a[4, 36], b[7, 34] = np.nan, np.nan        # (beyond the 33 values: not read)
    b[50, 3] = np.nan
    ref = fr.match_reference(a, b)
    assert ref["n_a_valid"] == 130 and ref["n_b_valid"] == 259
    assert_match(ctx.feature_match(a, b), ref, "strided")
    bare = ctx.feature_match(a, b, want_second=False, want_mutual=False)
    assert sorted(bare) == ["d", "idx", "n_a_valid", "n_b_valid", "n_mutual"] and bare["n_mutual"] == 0
    assert np.array_equal(bare["idx"], ref["idx"]) and same_f64(bare["d"], ref["d"])
    da, db = DevCloud(a), DevCloud(b)
    outs = [DevCloud(np.zeros((130, w), np.float32)) for w in (1, 2, 1, 2, 1)]      # int32, double, int32, double, bytes (4 B each: enough)
    try:
        info = ctx.feature_match_device(da.ptr, 130, 40, db.ptr, 260, 35, *[o.ptr for o in outs])
        assert info == {k: ref[k] for k in ("n_a_valid", "n_b_valid", "n_mutual")}
        host = dict(idx=np.zeros(130, np.int32), d=np.zeros(130), idx2=np.zeros(130, np.int32), d2=np.zeros(130), mutual=np.zeros(130, np.uint8))
        for (key, arr), o in zip(host.items(), outs):
            assert hip().hipMemcpy(C.c_void_p(arr.ctypes.data), C.c_void_p(o.ptr), arr.nbytes, D2H) == 0
        host.update(info)
        assert_match(host, ref, "device form")
    finally:
        for d in [da, db] + outs:
            d.free()


def test_the_library_refuses_what_the_header_lists(ctx):
    L = api.load()
    a, b = rows(8, 13), rows(9, 14)
    idx, d = np.zeros(8, np.int32), np.zeros(8)

    def call(pa=a.ctypes.data, na=8, sa=33, pb=b.ctypes.data, nb=9, sb=33, i=idx.ctypes.data, dd=d.ctypes.data):
        return L.dcreg_feature_match(ctx._h, pa, na, sa, pb, nb, sb, i, dd, None, None, None, None)

    assert call() == api.OK
    for kw in (dict(pa=None), dict(pb=None), dict(i=None), dict(dd=None), dict(sa=32), dict(sb=3), dict(na=-1), dict(nb=-2), dict(na=2 ** 31), dict(nb=2 ** 31)):
        assert call(**kw) == -1, kw
    assert call(na=0, pa=None) == api.OK and call(nb=0, pb=None) == api.OK and np.all(idx == -1) and np.all(np.isinf(d))


def test_the_lots_descriptors_match_their_moved_copy_as_the_reference_says(ctx):
    cloud = lot_cloud()
    normals = ctx.normals(cloud, api.normal_params(k=16))[0]
    mc, mn = moved_copy(cloud, normals)
    p = api.fpfh_params(k=16)
    fa, fb = ctx.fpfh(cloud, normals, params=p)[0], ctx.fpfh(mc, mn, params=p)[0]
    got = ctx.feature_match(fb, fa)
    assert_match(got, fr.match_reference(fb, fa), "lot")
    assert np.mean(got["idx"] == np.arange(len(cloud))) >= 0.995 and got["n_mutual"] >= 0.99 * len(cloud)
