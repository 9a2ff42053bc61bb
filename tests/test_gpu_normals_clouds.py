"""Normals of many clouds in one call (dcreg_normals_clouds*) against dcreg_normals of every cloud alone: every value and every info
record bitwise, NaN for sparse and non-finite points included.  The clouds sit on the sizes where the code takes another path - empty,
fewer than k finite points (no index), exactly k, the wave and block edges, more than one block - and one of them lies 1 km from the
others, so a grid shared between clouds would show.  The single-cloud values are computed once per module and never modified."""
import ctypes as C
import functools

import numpy as np
import pytest

import normals_ref as nr
from dcreg_amd import api
from test_gpu_device_seam import D2H, DevCloud, hip, strided
from test_gpu_normals import same, uniform, with_nan_rows

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 4, 5, 6, 63, 64, 65, 257, 523]
NAN_CLOUD, DUP_CLOUD, FAR_CLOUD, REF_CLOUD = 6, 8, 7, 5        # places in clouds(): 64 / 257 / 65 / 63 points before the planted rows


@functools.lru_cache(maxsize=None)
def clouds():
    """one cloud per size of SIZES: the 64-point one gets NaN rows on top, the 257-point one exact duplicates, the 65-point one lies
    1 km away"""
    out = [uniform(n, seed=40) for n in SIZES]
    out[NAN_CLOUD] = with_nan_rows(out[NAN_CLOUD])
    d = out[DUP_CLOUD].copy()
    d[10:14] = d[200]
    d[100] = d[101]
    out[DUP_CLOUD] = d
    out[FAR_CLOUD] = (out[FAR_CLOUD] + np.float32([1000.0, 0.0, 0.0])).astype(np.float32)
    for a in out:
        a.setflags(write=False)
    return out


PARAMS = {"k5": dict(k=5), "k9": dict(k=9), "k20": dict(k=20), "k5_r": dict(k=5, search_radius=0.4), "k9_view": dict(k=9, search_radius=1.0, viewpoint=(3.0, -2.0, 10.0))}

_alone = {}


def alone(key, cs):
    """Context.normals of every cloud of cs alone: computed once per (parameters, set), shared"""
    if key not in _alone:
        p = api.normal_params(**PARAMS[key[0]])
        c = api.Context(0)
        try:
            _alone[key] = [c.normals(a, p) for a in cs]
        finally:
            c.close()
    return _alone[key]


def assert_clouds_bitwise(got, want, what=""):
    nrm, cur, off, infos = got
    assert len(infos) == len(want) and len(off) == len(want) + 1
    for s, (wn, wc, _, wi) in enumerate(want):
        a, b = int(off[s]), int(off[s + 1])
        assert b - a == len(wn), (what, s)
        assert infos[s] == wi, (what, s, infos[s], wi)
        assert same(nrm[a:b], wn), (what, s)
        assert same(cur[a:b], wc), (what, s)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("key", list(PARAMS))
def test_every_cloud_is_bitwise_the_single_call(ctx, key):
    cs = clouds()
    p = api.normal_params(**PARAMS[key])
    want = alone((key, "edges"), cs)
    got = ctx.normals_clouds(cs, p)
    assert_clouds_bitwise(got, want, key)
    infos = got[3]
    assert infos[0] == {"n_in": 0, "n_finite": 0, "n_sparse": 0, "n_out": 0}
    if p.k == 5:
        assert infos[2] == {"n_in": 4, "n_finite": 4, "n_sparse": 4, "n_out": 0}                   # fewer than k finite points: no index
        assert infos[3]["n_finite"] == 5 and infos[NAN_CLOUD]["n_finite"] < infos[NAN_CLOUD]["n_in"]
        if p.search_radius == 0.0:
            assert infos[3]["n_out"] == 5 and infos[NAN_CLOUD]["n_out"] == infos[NAN_CLOUD]["n_finite"]          # exactly k points: every one has a normal
    if p.search_radius > 0.0:
        assert any(0 < i["n_sparse"] < i["n_finite"] for i in infos)                              # the bound bites in some cloud, not in all
    # only one output wanted: the other is not touched, the values are the same
    n_only = ctx.normals_clouds(cs, p, want_curvature=False)
    c_only = ctx.normals_clouds(cs, p, want_normals=False)
    assert n_only[1] is None and c_only[0] is None and same(n_only[0], got[0]) and same(c_only[1], got[1])
    assert n_only[3] == infos and c_only[3] == infos


def test_a_mid_sized_cloud_is_bitwise_the_reference(ctx):
    cs = clouds()
    p = api.normal_params(k=5)
    nrm, cur, off, infos = ctx.normals_clouds(cs, p)
    ref = nr.normals_reference(cs[REF_CLOUD], k=5)
    a, b = int(off[REF_CLOUD]), int(off[REF_CLOUD + 1])
    assert same(nrm[a:b], ref["normals"]) and same(cur[a:b], ref["curvature"])
    assert all(infos[REF_CLOUD][k] == ref[k] for k in ("n_in", "n_finite", "n_sparse", "n_out"))


def test_the_device_form_and_a_strided_cloud_give_the_same_values(ctx):
    cs = clouds()
    p = api.normal_params(k=5)
    want = alone(("k5", "edges"), cs)
    xyz = np.concatenate(cs, 0)
    off = np.concatenate([[0], np.cumsum([len(a) for a in cs])]).astype(np.int64)
    n = len(xyz)
    assert_clouds_bitwise(ctx.normals_clouds((strided(xyz, 5), off), p), want, "stride 5")
    dev = DevCloud(strided(xyz, 4, fill=3.0))
    out_n, out_c = DevCloud(np.full((n + 1, 3), 7.0, np.float32)), DevCloud(np.full((n + 1, 1), 7.0, np.float32))
    try:
        infos = ctx.normals_clouds_device(dev.ptr, off, 4, p, out_n.ptr, out_c.ptr)
        back_n, back_c = np.zeros((n + 1, 3), np.float32), np.zeros((n + 1, 1), np.float32)
        assert hip().hipMemcpy(C.c_void_p(back_n.ctypes.data), C.c_void_p(out_n.ptr), back_n.nbytes, D2H) == 0
        assert hip().hipMemcpy(C.c_void_p(back_c.ctypes.data), C.c_void_p(out_c.ptr), back_c.nbytes, D2H) == 0
    finally:
        dev.free(); out_n.free(); out_c.free()
    assert_clouds_bitwise((back_n[:n], back_c[:n, 0], off, infos), want, "device")
    assert np.all(back_n[n] == 7.0) and back_c[n, 0] == 7.0                        # one record more than the call's points: it stays


def test_a_smaller_call_after_a_larger_one(ctx):
    """stale buffers: fewer, smaller clouds after the large set, then the large set again"""
    cs = clouds()
    p = api.normal_params(k=5)
    small = [cs[4], cs[1], uniform(40, seed=41), cs[3]]
    for a in small:
        a.setflags(write=False)
    assert_clouds_bitwise(ctx.normals_clouds(cs, p), alone(("k5", "edges"), cs), "large")
    assert_clouds_bitwise(ctx.normals_clouds(small, p), alone(("k5", "small"), small), "small")
    assert_clouds_bitwise(ctx.normals_clouds([cs[0], cs[2]], p), alone(("k5", "none"), [cs[0], cs[2]]), "nothing to index")
    assert_clouds_bitwise(ctx.normals_clouds(cs, p), alone(("k5", "edges"), cs), "large again")
    assert ctx.normals_clouds([], p)[3] == []


def test_the_call_leaves_the_context_alone_and_single_calls_unchanged(ctx):
    cs = clouds()
    p = api.normal_params(k=5)
    c = api.Context(0)
    try:
        c.set_target(cs[9], 0.5)
        c.set_source(cs[8])
        prm = api.default_lin_params(0.5, 1)
        before = c.linearize(np.eye(3), np.zeros(3), prm)
        one = c.normals(cs[8], p)
        c.normals_clouds(cs, p)
        again = c.normals(cs[8], p)
        after = c.linearize(np.eye(3), np.zeros(3), prm)
        assert same(one[0], again[0]) and same(one[1], again[1]) and one[3] == again[3]
        assert before["n_eff"] == after["n_eff"] and np.array_equal(before["H_upper"], after["H_upper"]) and np.array_equal(before["g"], after["g"])
        info = c.index_info()
        assert info.n_target == 523 and info.n_source == 257
    finally:
        c.close()
