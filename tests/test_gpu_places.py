"""Place recognition on the device (dcreg_place_descriptors*, dcreg_places_*) against the numpy reference of tests/places_ref.py, which
applies include/dcreg.h's rules literally.  Descriptors must be bitwise the reference's on clouds without a point within 1e-9 of a bin
edge (asserted of every input first, with the reference alone); distances must agree to 1e-12 - the double evaluation's worst-case error
is roughly 60 * 20 * 2^-53 = 1.3e-13 on values of at most 2, the tolerance about eight times that - and the selection may differ from the
reference's only where reference distances lie within 2e-12 of each other.  The reference is the yardstick, never a second device run."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
import places_ref as pr
from dcreg_amd import api
from test_gpu_device_seam import D2H, DevCloud, _info, hip, strided

pytestmark = pytest.mark.gpu

TOL_D, TOL_SEL = 1e-12, 2e-12
CFG = dict(search_radius=1.0, max_iterations=20, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, use_weight_derivative=1, always_compute_schur=1)


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def clean(clouds, p):
    """the condition on the test data: no point of these clouds within 1e-9 of a bin edge"""
    return all(pr.ambiguous(c, p, 1e-9) == 0 for c in clouds)


def ref_descriptors(clouds, p):
    return np.stack([pr.descriptor(c, p) for c in clouds]) if len(clouds) else np.zeros((0, p.n_rings, p.n_sectors), np.float32)


def record(tr):
    """everything of a registration record but its time"""
    return (tr.converged, tr.iterations, tr.status, tr.trans_error_m, tr.rot_error_deg, tr.final_rmse, tr.final_fitness, tr.corr_num,
            tuple(tr.final_transform[:]), tuple(tr.H_upper[:]), tuple(tr.degenerate_mask[:]))


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drive():
    return pr.drive_scene()


@pytest.fixture(scope="module")
def parking():
    tgt, src = h.scene_parkinglot()
    return np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32), h.pose6d_matrix(**h.PK01_GT)


@pytest.fixture(scope="module")
def sweep(parking):
    """an organised 128 x 1024 sweep over the parking lot: NaN rows where a beam had no return"""
    s = h.lidar_sweep(parking[0], parking[2])
    assert np.isnan(s).any() and np.isfinite(s).all(1).sum() > 10_000
    return s


@pytest.fixture(scope="module")
def randdb():
    """5 000 seeded random descriptors with zero columns and duplicates, 64 queries (some of them copies of entries), and the reference
    distance table of the first 12 queries"""
    p = api.place_params()
    db = pr.random_database(5000, p, seed=3)
    qs = pr.random_database(64, p, seed=4)
    qs[1], qs[5], qs[9] = db[100], db[4321], np.roll(db[78], -13, axis=1)
    return p, db, qs, pr.distance_table(qs[:12], db)


# ---- 1. descriptors
PARAMS = {"default": api.place_params(), "range 30": api.place_params(max_range=30.0), "gated": api.place_params(16, 40, 20.0, 2.0, 3.0),
          "largest": api.place_params(64, 128, 60.0, 0.5, 2.0), "odd": api.place_params(7, 13, 25.0, 0.0, 1.5), "one bin": api.place_params(1, 1, 50.0)}


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_descriptors_are_bitwise_the_reference(ctx, drive, sweep, name):
    p = PARAMS[name]
    rng = np.random.default_rng(12)
    frames = drive["frames"]
    small = [f[:n] for f, n in zip(frames[10:40], rng.integers(1, 900, 30))]          # tiles that straddle clouds
    clouds = [sweep, frames[0], frames[1], np.zeros((0, 3), np.float32)] + small + [frames[2], np.full((5, 3), np.nan, np.float32), frames[3][:2500]]
    assert clean(clouds, p)
    want = ref_descriptors(clouds, p)
    got, info = ctx.place_descriptors(clouds, p)
    assert got.shape == want.shape and got.dtype == np.float32
    for k in range(len(clouds)):
        assert same(got[k], want[k]), (name, k, int((got[k] != want[k]).sum()))
    assert info == pr.info(clouds, p)
    assert info["n_finite"] < info["n_in"] and (name != "gated" or info["n_used"] < info["n_finite"])
    # one cloud alone, another order of its points, and a strided record layout: the same bits
    for k in (0, 1, 7):
        alone, _ = ctx.place_descriptors([clouds[k]], p)
        assert same(alone[0], want[k])
        mixed, _ = ctx.place_descriptors([clouds[k][rng.permutation(len(clouds[k]))]], p)
        assert same(mixed[0], want[k])
    wide, winfo = ctx.place_descriptors([strided(c, 7) for c in clouds], p)
    assert same(wide, want) and winfo == info
    xyz, off, _ = api._clouds(clouds, "test")
    pair, _ = ctx.place_descriptors((xyz, off), p)
    assert same(pair, want)
    # the device form, strided rows from an unaligned start
    dev = DevCloud(strided(xyz, 5), offset=4)
    out = DevCloud(np.zeros((len(clouds), p.n_rings * p.n_sectors), np.float32))
    try:
        dinfo = ctx.place_descriptors_device(dev.ptr, off, 5, out.ptr, p)
        back = np.empty_like(want)
        assert hip().hipMemcpy(C.c_void_p(back.ctypes.data), C.c_void_p(out.ptr), back.nbytes, D2H) == 0
        assert same(back, want) and dinfo == info
    finally:
        dev.free()
        out.free()
    none, ninfo = ctx.place_descriptors([], p)
    assert none.shape == (0, p.n_rings, p.n_sectors) and ninfo == {"n_in": 0, "n_finite": 0, "n_used": 0}


# ---- 2. the database
def test_the_database_holds_the_descriptors_and_outlives_maps_and_sources(ctx, drive, parking):
    p = drive["params"]
    frames = drive["frames"]
    assert clean(frames[:12] + [parking[1]], p)
    want = ref_descriptors(frames[:12], p)
    ctx.places_reset(p)
    assert ctx.places_count() == 0 and ctx.places_get().shape == (0, p.n_rings, p.n_sectors)
    at, info = ctx.places_add_clouds(frames[:5])
    assert at == 0 and info == pr.info(frames[:5], p) and ctx.places_count() == 5
    xyz, off, _ = api._clouds([strided(f, 4) for f in frames[5:9]], "test")
    dev = DevCloud(xyz)
    try:
        at, info = ctx.places_add_clouds_device(dev.ptr, off, 4)
    finally:
        dev.free()
    assert at == 5 and info == pr.info(frames[5:9], p)
    assert ctx.places_add(ctx.place_descriptors(frames[9:11], p)[0]) == 9
    ctx.set_source(frames[11])
    at, info = ctx.places_add_source()
    assert at == 11 and info == pr.info(frames[11:12], p) and ctx.places_count() == 12
    assert same(ctx.places_get(), want) and same(ctx.places_get(3, 4), want[3:7]) and ctx.places_get(12).shape[0] == 0
    # a map, another source, a batched registration and a crop later the places are what they were
    tgt, src, gt = parking
    ctx.set_target(tgt, 1.0)
    ctx.set_source(src)
    cfg = api.default_config(**CFG)
    ctx.register_frames([src, src[:4000]], [gt, gt], "Ours", cfg)
    ctx.insert_source(gt, 0.1)
    ctx.crop(gt[:3, 3] - 30.0, gt[:3, 3] + 30.0)
    assert ctx.places_count() == 12 and same(ctx.places_get(), want)
    at, _ = ctx.places_add_source()                                # the source in its input order
    assert at == 12 and same(ctx.places_get(12, 1)[0], pr.descriptor(src, p))
    # growth keeps what is there
    more = pr.random_database(700, p, seed=21)
    assert ctx.places_add(more) == 13
    assert ctx.places_count() == 713 and same(ctx.places_get(0, 12), want) and same(ctx.places_get(13), more)
    ctx.places_reset(api.place_params(4, 8, 10.0))
    assert ctx.places_count() == 0 and ctx.places_get().shape == (0, 4, 8)


# ---- 3. the search against the reference
def check_search(D, first, last, k, idx, shift, dist, what):
    """D [nq, entries, n_sectors]: the reference distances of the queries against the whole database"""
    nq = D.shape[0]
    assert idx.shape == shift.shape == dist.shape == (nq, k) and idx.dtype == np.int32 and shift.dtype == np.int32 and dist.dtype == np.float64
    best = D.min(2)
    n_hit = min(k, last - first)
    worst_d = worst_shift = worst_out = 0.0
    for q in range(nq):
        e, s, d = idx[q, :n_hit], shift[q, :n_hit], dist[q, :n_hit]
        assert np.all(idx[q, n_hit:] == -1) and np.all(shift[q, n_hit:] == 0) and np.all(np.isposinf(dist[q, n_hit:])), (what, q)
        if n_hit == 0:
            continue
        assert np.all((e >= first) & (e < last)) and len(set(e.tolist())) == n_hit, (what, q)
        assert np.all((s >= 0) & (s < D.shape[2])), (what, q)
        ref = D[q, e, s]
        worst_d = max(worst_d, np.abs(d - ref).max())
        worst_shift = max(worst_shift, (ref - best[q, e]).max())
        assert np.all(np.diff(d) >= 0), (what, q)
        tie = np.diff(d) == 0
        assert np.all(np.diff(e)[tie] > 0), (what, q)                    # equal distances: by index
        out = np.setdiff1d(np.arange(first, last), e)
        if len(out):
            worst_out = max(worst_out, ref[-1] - best[q, out].min())
    print("%s: |dist - ref| %.3g, ref at the shift above the entry's minimum %.3g, an entry left out below the last %.3g"
          % (what, worst_d, worst_shift, worst_out))
    assert worst_d <= TOL_D, what
    assert worst_shift <= TOL_SEL, what
    assert worst_out <= TOL_SEL, what


def test_the_search_on_a_drive_is_the_reference(ctx, drive):
    p = drive["params"]
    assert clean(drive["frames"] + drive["rev_frames"], p)
    db, qs = ref_descriptors(drive["frames"], p), ref_descriptors(drive["rev_frames"], p)
    D = pr.distance_table(qs, db)
    ctx.places_reset(p)
    ctx.places_add_clouds(drive["frames"])
    assert same(ctx.places_get(), db)
    for k, first, last in [(1, 0, 120), (5, 0, 120), (64, 0, 120), (5, 0, 100), (64, 90, 120), (3, 119, 120), (2, 60, 60)]:
        idx, shift, dist, info = ctx.places_query_clouds(drive["rev_frames"], k, first, last)
        check_search(D, first, last, k, idx, shift, dist, "drive, clouds, k %d of [%d, %d)" % (k, first, last))
        assert info == pr.info(drive["rev_frames"], p)
        hidx, hshift, hdist = ctx.places_query(qs, k, first, last)
        assert np.array_equal(hidx, idx) and np.array_equal(hshift, shift) and same64(hdist, dist)
    # the revisits find their keyframes as the reference does: the recorded 23 of 24
    idx, shift, dist, _ = ctx.places_query_clouds(drive["rev_frames"], 1)
    ridx, rshift, _ = pr.search_table(D, 0, 120, 1)
    assert np.array_equal(idx, ridx) and np.array_equal(shift, rshift)
    assert (np.abs(idx[:, 0] - drive["rev_of"]) <= 1).sum() >= 20
    xyz, off, _ = api._clouds(drive["rev_frames"][:6], "test")
    dev = DevCloud(xyz)
    try:
        didx, dshift, ddist, _ = ctx.places_query_clouds_device(dev.ptr, off, 3, 5, 10, 110)
    finally:
        dev.free()
    idx, shift, dist, _ = ctx.places_query_clouds(drive["rev_frames"][:6], 5, 10, 110)
    assert np.array_equal(didx, idx) and np.array_equal(dshift, shift) and same64(ddist, dist)


def test_the_search_on_random_descriptors_is_the_reference(ctx, randdb):
    p, db, qs, D = randdb
    ctx.places_reset(p)
    assert ctx.places_add(db[:3000]) == 0 and ctx.places_add(db[3000:]) == 3000
    assert same(ctx.places_get(), db)
    for k, first, last in [(1, 0, 5000), (5, 0, 5000), (64, 0, 5000), (64, 4090, 4100), (5, 4096, 5000), (7, 1000, 4097), (1, 11, 12)]:
        idx, shift, dist = ctx.places_query(qs[:12], k, first, last)
        check_search(D, first, last, k, idx, shift, dist, "random, k %d of [%d, %d)" % (k, first, last))
    idx, shift, dist = ctx.places_query(qs[:12], 3)
    assert idx[1, 0] == 100 and idx[5, 0] == 4321 and (idx[9, 0], shift[9, 0]) == (78, 13) and np.all(np.abs(dist[[1, 5, 9], 0]) <= TOL_D)
    assert dist[0, 0] > 0.01
    zero = np.zeros((1, p.n_rings, p.n_sectors), np.float32)             # no column in common with anything: 1 at shift 0, by index
    idx, shift, dist = ctx.places_query(zero, 4, 20, 5000)
    assert idx.tolist() == [[20, 21, 22, 23]] and shift.tolist() == [[0] * 4] and dist.tolist() == [[1.0] * 4]


@pytest.mark.parametrize("rings,sectors", [(10, 100), (64, 128), (3, 65), (5, 7), (1, 1)])
def test_the_search_with_other_grids_is_the_reference(ctx, rings, sectors):
    """more than 64 sectors run the wide form of the distance kernel; the tolerance's bound scales with rings * sectors (at most 7 times
    the default grid's for 64 x 128: still below 1e-12)"""
    p = api.place_params(rings, sectors, 40.0)
    db, qs = pr.random_database(300, p, seed=rings), pr.random_database(6, p, seed=sectors + 1)
    qs[2] = np.roll(db[150], -(sectors // 3), axis=1)
    D = pr.distance_table(qs, db)
    ctx.places_reset(p)
    ctx.places_add(db)
    for k, first, last in [(1, 0, 300), (64, 0, 300), (5, 17, 203)]:
        idx, shift, dist = ctx.places_query(qs, k, first, last)
        check_search(D, first, last, k, idx, shift, dist, "%d x %d, k %d of [%d, %d)" % (rings, sectors, k, first, last))


# ---- 4. independence
def test_a_pair_depends_on_its_two_descriptors_only(ctx, randdb):
    p, db, qs, _ = randdb
    ctx.places_reset(p)
    ctx.places_add(db[:4000])
    idx, shift, dist = ctx.places_query(qs, 64)
    again = ctx.places_query(qs, 64)
    assert np.array_equal(again[0], idx) and np.array_equal(again[1], shift) and same64(again[2], dist)      # two runs
    for q in (0, 17, 63):
        a = ctx.places_query(qs[q:q + 1], 64)                                                                # alone
        assert np.array_equal(a[0][0], idx[q]) and np.array_equal(a[1][0], shift[q]) and same64(a[2][0], dist[q])
        a = ctx.places_query(qs[q:q + 1], 5)                                                                 # another k
        assert np.array_equal(a[0][0], idx[q, :5]) and np.array_equal(a[1][0], shift[q, :5]) and same64(a[2][0], dist[q, :5])
    # every entry of a range, one query at a time and in one batch
    one = [ctx.places_query(qs[q:q + 1], 64, 1000, 1064) for q in range(20)]
    many = ctx.places_query(qs[:20], 64, 1000, 1064)
    for q in range(20):
        assert np.array_equal(one[q][0][0], many[0][q]) and np.array_equal(one[q][1][0], many[1][q]) and same64(one[q][2][0], many[2][q])
    table = {(q, e): (s, d) for q in range(20) for e, s, d in zip(many[0][q], many[1][q], many[2][q].view(np.uint64))}
    # a grown database: the old range gives the old result, the whole one the same (shift, distance) for the entries it shares
    ctx.places_add(db[4000:])
    old = ctx.places_query(qs, 64, 0, 4000)
    assert np.array_equal(old[0], idx) and np.array_equal(old[1], shift) and same64(old[2], dist)
    whole = ctx.places_query(qs, 64)
    known = {(q, e): (s, d) for q in range(64) for e, s, d in zip(idx[q], shift[q], dist[q].view(np.uint64))}
    shared = 0
    for q in range(64):
        for e, s, d in zip(whole[0][q], whole[1][q], whole[2][q].view(np.uint64)):
            if (q, e) in known:
                assert known[q, e] == (s, d), (q, e)
                shared += 1
    assert shared > 64 * 32
    wide = ctx.places_query(qs[:20], 64, 990, 1080)
    for q in range(20):
        for e, s, d in zip(wide[0][q], wide[1][q], wide[2][q].view(np.uint64)):
            if (q, e) in table:
                assert table[q, e] == (s, d), (q, e)


# ---- 5. the chain into the registration
def test_query_source_place_guess_register_pairs(ctx, drive):
    p = drive["params"]
    frames, revs = drive["frames"], drive["rev_frames"]
    db = ref_descriptors(frames, p)
    cfg = api.default_config(**CFG)
    ctx.places_reset(p)
    ctx.places_add_clouds(frames)
    for q in (2, 11, 20):
        ctx.set_source(revs[q])
        idx, shift, dist, info = ctx.places_query_source(5)
        assert info == pr.info([revs[q]], p)
        got = ctx.register_pairs([revs[q]] * 5, [frames[e] for e in idx], [api.place_guess(s, p.n_sectors) for s in shift], "Ours", cfg)
        ridx, rshift, _ = pr.search(pr.descriptor(revs[q], p)[None], db, 0, len(db), 5)
        want = ctx.register_pairs([revs[q]] * 5, [frames[e] for e in ridx[0]], [api.place_guess(s, p.n_sectors) for s in rshift[0]], "Ours", cfg)
        assert [record(r) for r in got] == [record(r) for r in want]
        # a later keyframe's range leaves the newest entries out
        idx, _, _, _ = ctx.places_query_source(5, 0, 40)
        assert np.all(idx < 40)


# ---- 6. the rest of the context
def test_the_place_calls_leave_the_rest_of_the_context_alone(drive, parking):
    tgt, src, gt = parking
    p = drive["params"]
    cfg = api.default_config(**CFG)
    prm = api.default_lin_params(1.0, 1)
    c = api.Context(0)
    try:
        c.set_target(tgt, 1.0)
        c.set_source(src)
        frames = [src[:5000], src[1000:7000]]

        def snapshot():
            lin = c.linearize(gt[:3, :3], gt[:3, 3], prm)
            return (lin["n_eff"], lin["n_pt"], tuple(lin["H_upper"]), tuple(lin["g"]), lin["sum_r2"], lin["sum_b2"],
                    [record(r) for r in c.register_frames(frames, [gt, gt], "Ours", cfg)], _info(c))

        before = snapshot()
        xyz, off, _ = api._clouds(drive["rev_frames"][:3], "test")
        dev = DevCloud(xyz)
        out = DevCloud(np.zeros((3, p.n_rings * p.n_sectors), np.float32))
        try:
            steps = [lambda: c.place_descriptors(drive["frames"][:4], p), lambda: c.place_descriptors_device(dev.ptr, off, 3, out.ptr, p),
                     lambda: c.places_reset(p), lambda: c.places_add_clouds(drive["frames"][:30]), lambda: c.places_add_clouds_device(dev.ptr, off, 3),
                     lambda: c.places_add_source(), lambda: c.places_add(c.places_get(2, 5)), lambda: c.places_query(c.places_get(0, 3), 5),
                     lambda: c.places_query_clouds(drive["rev_frames"][:4], 64), lambda: c.places_query_clouds_device(dev.ptr, off, 3, 2, 1, 20),
                     lambda: c.places_query_source(3)]
            for k, step in enumerate(steps):
                step()
                assert snapshot() == before, k
        finally:
            dev.free()
            out.free()
        assert c.places_count() == 30 + 3 + 1 + 5
    finally:
        c.close()


# ---- 7. refusals at the C-ABI
def test_refusals_at_the_c_abi(drive, parking, randdb):
    tgt, src, gt = parking
    p, db, qs, _ = randdb
    L = api.load()
    i64p, ip, fp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    cloud = np.ascontiguousarray(drive["frames"][0])
    off = np.array([0, len(cloud)], np.int64)
    desc = np.ascontiguousarray(db[:3])
    out = np.zeros((4, p.n_rings, p.n_sectors), np.float32)
    idx, shift, dist = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(64)
    res = lambda: (idx.ctypes.data_as(ip), shift.ctypes.data_as(ip), dist.ctypes.data_as(dp))       # noqa: E731
    info = api.PlaceInfo()
    c = api.Context(0)
    h_ = c._h
    try:
        def every_call(params):
            return [("descriptors", lambda: L.dcreg_place_descriptors(h_, 1, cloud.ctypes.data, off.ctypes.data_as(i64p), 3, C.byref(params), out.ctypes.data, None)),
                    ("reset", lambda: L.dcreg_places_reset(h_, C.byref(params))),
                    ("add", lambda: L.dcreg_places_add(h_, 3, desc.ctypes.data_as(fp))),
                    ("add_clouds", lambda: L.dcreg_places_add_clouds(h_, 1, cloud.ctypes.data, off.ctypes.data_as(i64p), 3, C.byref(info))),
                    ("add_source", lambda: L.dcreg_places_add_source(h_, None)),
                    ("get", lambda: L.dcreg_places_get(h_, 0, 1, out.ctypes.data_as(fp))),
                    ("query", lambda: L.dcreg_places_query(h_, 3, desc.ctypes.data_as(fp), 0, 1, 5, *res())),
                    ("query_clouds", lambda: L.dcreg_places_query_clouds(h_, 1, cloud.ctypes.data, off.ctypes.data_as(i64p), 3, 0, 1, 5, *res(), None)),
                    ("query_source", lambda: L.dcreg_places_query_source(h_, 0, 1, 5, *res(), None))]

        # before dcreg_places_reset: add, get and query have no database (the descriptors need none)
        calls = dict(every_call(p))
        for name in ("add", "add_clouds", "add_source", "get", "query", "query_clouds", "query_source"):
            assert calls[name]() == -4, name
            assert b"dcreg_places_reset" in L.dcreg_last_error(h_)
        assert L.dcreg_places_count(h_) == 0 and L.dcreg_places_count(None) == -1
        assert calls["descriptors"]() == 0 and same(out[0], pr.descriptor(cloud, p))
        # bad parameters
        for field, value in [("n_rings", 0), ("n_rings", 65), ("n_sectors", 0), ("n_sectors", 129), ("max_range", 0.0), ("max_range", np.inf),
                             ("max_range", np.nan), ("min_range", -1.0), ("min_range", 80.0), ("min_range", np.nan), ("z_offset", np.nan),
                             ("z_offset", -np.inf)]:
            bad = api.place_params()
            setattr(bad, field, value)
            for name in ("descriptors", "reset"):
                assert dict(every_call(bad))[name]() == -1, (field, value, name)
        assert L.dcreg_places_reset(h_, None) == -1 and L.dcreg_places_count(h_) == 0
        assert calls["add"]() == -4                                       # a refused reset made no database
        # a database of three entries; the source forms have no source yet
        assert calls["reset"]() == 0 and calls["add"]() == 0 and L.dcreg_places_count(h_) == 3
        assert calls["add_source"]() == -4 and calls["query_source"]() == -4 and L.dcreg_places_count(h_) == 3

        def unchanged():
            got = np.zeros_like(desc)
            return L.dcreg_places_count(h_) == 3 and L.dcreg_places_get(h_, 0, 3, got.ctypes.data_as(fp)) == 0 and same(got, desc)

        q = lambda first, last, k: L.dcreg_places_query(h_, 3, desc.ctypes.data_as(fp), first, last, k, *res())       # noqa: E731
        assert q(0, 3, 5) == 0 and idx[:15].reshape(3, 5)[:, 0].tolist() == [0, 1, 2] and np.all(idx[:15].reshape(3, 5)[:, 3:] == -1)
        for first, last, k in [(2, 1, 5), (-1, 2, 5), (0, 4, 5), (4, 4, 5), (0, 3, 0), (0, 3, 65), (0, 3, -1)]:
            assert q(first, last, k) == -1, (first, last, k)
            assert L.dcreg_places_query_clouds(h_, 1, cloud.ctypes.data, off.ctypes.data_as(i64p), 3, first, last, k, *res(), None) == -1
        assert q(3, 3, 1) == 0 and idx[:3].tolist() == [-1, -1, -1]        # an empty range at the end is a range
        assert L.dcreg_places_query(h_, 3, None, 0, 3, 1, *res()) == -1 and L.dcreg_places_query(h_, 3, desc.ctypes.data_as(fp), 0, 3, 1, None, None, None) == -1
        assert L.dcreg_places_query(h_, -1, desc.ctypes.data_as(fp), 0, 3, 1, *res()) == -1
        for value in (np.nan, np.inf, -np.inf):
            bad = desc.copy()
            bad[2, 7, 31] = value
            assert L.dcreg_places_add(h_, 3, bad.ctypes.data_as(fp)) == -1 and b"finite" in L.dcreg_last_error(h_)
            assert L.dcreg_places_query(h_, 3, bad.ctypes.data_as(fp), 0, 3, 1, *res()) == -1
            assert unchanged()
        assert L.dcreg_places_add(h_, -1, desc.ctypes.data_as(fp)) == -1 and L.dcreg_places_add(h_, 2, None) == -1
        assert L.dcreg_places_get(h_, 2, 2, out.ctypes.data_as(fp)) == -1 and L.dcreg_places_get(h_, -1, 1, out.ctypes.data_as(fp)) == -1
        assert L.dcreg_places_get(h_, 0, 3, None) == -1
        # clouds as the voxel calls refuse them
        bad_off = np.array([1, len(cloud)], np.int64)
        assert L.dcreg_places_add_clouds(h_, 1, cloud.ctypes.data, bad_off.ctypes.data_as(i64p), 3, None) == -1
        assert L.dcreg_places_add_clouds(h_, 1, cloud.ctypes.data, off.ctypes.data_as(i64p), 2, None) == -1
        assert L.dcreg_places_add_clouds(h_, 1, None, off.ctypes.data_as(i64p), 3, None) == -1
        assert L.dcreg_places_add_clouds(h_, -1, cloud.ctypes.data, off.ctypes.data_as(i64p), 3, None) == -1
        assert L.dcreg_place_descriptors(h_, 1, cloud.ctypes.data, off.ctypes.data_as(i64p), 3, C.byref(p), None, None) == -1
        assert unchanged()
        # while a gated launch waits for its pose every call is refused at once, and the launch still gives its result
        c.set_target(tgt, 1.0)
        c.set_source(src)
        prm = api.default_lin_params(1.0, 1)
        want = c.linearize(gt[:3, :3], gt[:3, 3], prm)
        c.linearize_gated_begin(prm, slot=0)
        for name, call in every_call(p):
            assert call() == -4, name
        c.gate_open(gt[:3, :3], gt[:3, 3])
        got = c.linearize_end(slot=0)
        assert got["n_eff"] == want["n_eff"] and np.array_equal(got["H_upper"], want["H_upper"]) and np.array_equal(got["g"], want["g"])
        assert unchanged()
        assert calls["add_source"]() == 0 and L.dcreg_places_query_source(h_, 0, 4, 5, *res(), None) == 0 and idx[0] == 3 and abs(dist[0]) <= TOL_D
    finally:
        c.close()
