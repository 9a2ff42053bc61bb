"""Place recognition on the device at its bin edges and past the limits of its search, against the numpy reference of
tests/places_ref.py and the scenes of tests/places_edge_scenes.py (tests/test_places_edge_scenes.py shows on the CPU that they have
teeth).  The reference is the yardstick, never a second device run.

Descriptors, counts, indices and shifts are exact.  Every point of an edge cloud is either a decided point - on an edge, its bin fixed by
include/dcreg.h's literal double evaluation, moved by some other evaluation - or at least 1e-9 from every edge; this is asserted first,
with the reference alone, and no point is left out of the comparison.

Distances keep the tolerances of tests/test_gpu_places.py: |dist - ref| <= TOL_D = 1e-12 and a selection that differs from the
reference's only where reference distances lie within TOL_SEL = 2e-12.  Its bound, restated for the grids here: the double evaluation's
worst-case error is roughly rings * sectors * 2^-53 on values of at most 2, that is 1.3e-13 for the default 20 x 60 grid.  The largest
grid of this file is 8 x 128 (1 024 products against the default's 1 200: 1.1e-13) and the search scenes use 2 x 3: both below the
default grid's bound, which the tolerance exceeds about eight times."""
import numpy as np
import pytest

import places_edge_scenes as es
import places_ref as pr
from dcreg_amd import api
from test_gpu_places import TOL_D, check_search, ref_descriptors, same, same64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def bins_of(d):
    return np.flatnonzero(np.asarray(d).reshape(-1)).tolist()


# ---- 1. descriptors at the edges
@pytest.mark.parametrize("name", sorted(es.GRIDS))
def test_decided_points_fall_in_the_bin_of_the_literal_rule(ctx, name):
    """one cloud per point (its height positive: the point alone shows its bin and whether the gate took it), then all of them in one
    cloud with heights rising and with heights falling"""
    S = es.edge_scene(name)
    p, xy, nd = S["params"], S["xy"], S["n_decided"]
    assert es.clean_or_decided(S) and nd >= 30
    clouds = S["clouds_each"] + S["clouds_all"]
    want = ref_descriptors(clouds, p)
    got, info = ctx.place_descriptors(clouds, p)
    wrong = [k for k in range(len(clouds)) if not same(got[k], want[k])]
    report = [(k, "decided" if k < nd else "clean" if k < len(xy) else "all", xy[k].tolist() if k < len(xy) else None, bins_of(want[k])[:4],
               bins_of(got[k])[:4]) for k in wrong[:16]]
    print("%s: %d decided and %d clean points, %d clouds differ" % (name, nd, len(xy) - nd, len(wrong)))
    assert not wrong, (name, len(wrong), report)
    assert info == pr.info(clouds, p)
    for k in (len(xy), len(xy) + 1):                                   # one cloud in the call: the block-local maximum
        alone, ainfo = ctx.place_descriptors([clouds[k]], p)
        assert same(alone[0], want[k]) and ainfo == pr.info([clouds[k]], p)
    # ... and through the database
    ctx.places_reset(p)
    at, dinfo = ctx.places_add_clouds(clouds[:nd])
    assert at == 0 and dinfo == pr.info(clouds[:nd], p) and same(ctx.places_get(), want[:nd])


@pytest.mark.parametrize("name", ["below", "mixed", "ends", "minus_zero", "crowd", "every", "one"])
def test_heights_keep_their_largest_value_whatever_its_sign(ctx, name):
    p, clouds = es.height_scenes()[name]
    assert all(pr.ambiguous(c, p, es.GUARD) == 0 for c in clouds)
    want = ref_descriptors(clouds, p)
    got, info = ctx.place_descriptors(clouds, p)
    for k in range(len(clouds)):
        assert same(got[k], want[k]), (name, k, want[k].tolist(), got[k].tolist())
        alone, _ = ctx.place_descriptors([clouds[k]], p)
        assert same(alone[0], want[k]), (name, k)
        mixed, _ = ctx.place_descriptors([clouds[k][::-1]], p)
        assert same(mixed[0], want[k]), (name, k)
    assert info == pr.info(clouds, p)


def test_five_thousand_tiny_clouds_in_one_call(ctx):
    p, clouds = es.many_clouds()
    assert all(pr.ambiguous(c, p, es.GUARD) == 0 for c in clouds)
    want = ref_descriptors(clouds, p)
    got, info = ctx.place_descriptors(clouds, p)
    wrong = [k for k in range(len(clouds)) if not same(got[k], want[k])]
    assert not wrong, (len(wrong), wrong[:10])
    assert info == pr.info(clouds, p)
    ctx.places_reset(p)
    at, ainfo = ctx.places_add_clouds(clouds)
    assert at == 0 and ainfo == info and ctx.places_count() == es.N_CROWD and same(ctx.places_get(), want)


# ---- 2. the search past its limits
@pytest.fixture(scope="module")
def levels():
    db, qs, pick = es.levels_scene()
    return db, qs, pick, pr.small_table(qs, db)


def copies_come_by_index(idx, dist, pick, first, last, what):
    """a copy of a returned entry has bitwise its distance (a pair depends on its two descriptors only): every copy inside the range with
    a smaller index is returned too"""
    order = np.argsort(pick, kind="stable")
    start = np.searchsorted(pick[order], np.arange(pick.max() + 2))
    for q in range(len(idx)):
        got = set(idx[q].tolist())
        for e in idx[q]:
            if e < 0:
                continue
            group = order[start[pick[e]]:start[pick[e] + 1]]
            earlier = group[(group >= first) & (group < e)]
            assert all(int(c) in got for c in earlier), (what, q, int(e), earlier[:5].tolist())
        d = dist[q][idx[q] >= 0]
        groups = pick[idx[q][idx[q] >= 0]]
        assert all(d[i] == d[j] for i in range(len(d)) for j in range(i) if groups[i] == groups[j]), (what, q)


def test_two_and_three_selection_launches_are_the_reference(ctx, levels):
    """262 144 candidates leave 64 chunks (64 * 64 = 4 096 survivors: one more launch), 262 145 leave 65 (4 160 survivors with k = 64: two
    more launches, the third level; k = 1 and 5 take two launches on either side).  Whole ranges and ranges that start at entry 1 of the
    larger database"""
    db, qs, pick, D = levels
    ctx.places_reset(es.SMALL)
    assert ctx.places_add(db) == 0 and ctx.places_count() == es.N_LEVELS
    cases = [(64, 0, 262_144), (64, 0, 262_145), (64, 1, 262_145), (64, 1, 262_146), (1, 0, 262_144), (5, 0, 262_144), (1, 1, 262_146), (5, 1, 262_146)]
    for k, first, last in cases:
        what = "levels, k %d of [%d, %d)" % (k, first, last)
        idx, shift, dist = ctx.places_query(qs, k, first, last)
        check_search(D, first, last, k, idx, shift, dist, what)
        copies_come_by_index(idx, dist, pick, first, last, what)
    idx, shift, dist = ctx.places_query(qs, 64, 0, 262_145)
    assert abs(dist[0, 0]) <= TOL_D and abs(dist[1, 0]) <= TOL_D       # (copies of entries: with two rings many other entries reach 0 too)
    assert idx[2].tolist() == list(range(64)) and np.all(dist[2] == 1.0) and not shift[2].any()       # no column in common: by index
    spread = [len(set((idx[q] // 4096).tolist())) for q in range(len(qs))]
    assert max(spread) >= 16                                           # the 64 best of a query come from many first-level chunks


def rows_are_their_representatives(res, pick):
    """every row of a result is bitwise the row of the first query with the same descriptor -> those first rows"""
    rep = np.array([np.flatnonzero(pick == g)[0] for g in range(pick.max() + 1)])
    idx, shift, dist = res
    assert np.array_equal(idx, idx[rep[pick]]) and np.array_equal(shift, shift[rep[pick]]) and same64(dist, dist[rep[pick]])
    return rep


@pytest.fixture(scope="module")
def batch_ref(levels):
    distinct, _ = es.drawn_queries(127, 8, 60)
    return distinct, pr.small_table(distinct, levels[0])


@pytest.mark.parametrize("nq", [63, 64, 127])
def test_query_batches_give_every_query_its_own_row(ctx, levels, batch_ref, nq):
    """262 145 entries: 63 queries fill one batch of 2^24 pairs, 64 need a second one of a single query, 127 a third.  The queries are
    drawn from 8 descriptors, neighbours across a batch boundary differ; every row is bitwise its single-query result and the row of
    every other query with its descriptor, and those results are the reference's"""
    db = levels[0]
    distinct, D = batch_ref
    _, pick = es.drawn_queries(nq, 8, 60)
    ctx.places_reset(es.SMALL)
    ctx.places_add(db)
    k, first, last = 5, 0, 262_145
    res = ctx.places_query(distinct[pick], k, first, last)
    rep = rows_are_their_representatives(res, pick)
    check_search(D, first, last, k, res[0][rep], res[1][rep], res[2][rep], "batches, %d queries" % nq)
    for g in range(len(distinct)):
        idx, shift, dist = ctx.places_query(distinct[g:g + 1], k, first, last)                  # the query alone
        rows = np.flatnonzero(pick == g)
        assert np.all(res[0][rows] == idx[0]) and np.all(res[1][rows] == shift[0]), (nq, g)
        assert np.all(res[2][rows].view(np.uint64) == dist[0].view(np.uint64)), (nq, g)
    assert np.abs(res[2] - D[pick[:, None], res[0], res[1]]).max() <= TOL_D


@pytest.fixture(scope="module")
def crowd_ref():
    db, _ = es.small_descriptors(40, 71, 25)
    distinct, _ = es.drawn_queries(70_000, 64, 60)
    return db, distinct, pr.distance_table(distinct, db)


@pytest.mark.parametrize("nq", [65_535, 65_536, 65_537, 70_000])
def test_more_queries_than_a_launch_grid_is_tall(ctx, crowd_ref, nq):
    """40 entries, k = 5: every query count here is a single batch, so the selection's launch grid is as tall as the call has queries.
    The call succeeds and every row is the reference's: bitwise the row of the first query with its descriptor, which check_search
    holds to the reference, and within TOL_D of the reference at its own (entry, shift)"""
    db, distinct, D = crowd_ref
    _, pick = es.drawn_queries(nq, 64, 60)
    ctx.places_reset(es.SMALL)
    ctx.places_add(db)
    res = ctx.places_query(distinct[pick], 5)
    assert res[0].shape == (nq, 5) and res[0].min() >= 0
    rep = rows_are_their_representatives(res, pick)
    check_search(D, 0, 40, 5, res[0][rep], res[1][rep], res[2][rep], "%d queries" % nq)
    assert np.abs(res[2] - D[pick[:, None], res[0], res[1]]).max() <= TOL_D


# ---- 3. the distance rule's own edges
SECTORS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)              # either side of the 16-column tiles and of the 64-lane split
RINGS = (3, 4, 5, 8)                                                  # either side of the groups of four rings


@pytest.mark.parametrize("rings", RINGS)
@pytest.mark.parametrize("sectors", SECTORS)
def test_the_distance_rule_at_its_edges(ctx, rings, sectors):
    """Column masks with a known count m of common columns, exact ties between shifts, one-column descriptors and an entry rolled by
    every shift, on 150 random entries and six planted ones.
    Why the ties are exact: when every column of a descriptor is the same vector (or the descriptor has period S / 2), the normalised
    columns are bitwise equal too, so every product q_j . c_l that a shift n sums is bitwise the one another shift sums at the same
    position j - each is one chain of fused multiply-adds over the rings in ring order - and the sums over j run in the same order: D_n
    has the same bits for all tied n, on the device as in the reference, and the rule's smallest n wins: shift 0."""
    R, S = rings, sectors
    p = api.place_params(R, S, 40.0)
    rng = np.random.default_rng(1000 * R + S)
    col = lambda: rng.uniform(0.5, 6.0, R).astype(np.float32)         # noqa: E731
    base = pr.random_database(150, p, seed=100 * R + S)
    full = rng.uniform(0.5, 6.0, (R, S)).astype(np.float32)
    alike = np.repeat(col()[:, None], S, 1)
    half = np.tile(rng.uniform(0.5, 6.0, (R, S // 2)).astype(np.float32), 2) if S % 2 == 0 else np.repeat(col()[:, None], S, 1)
    c_lone, c_anti, c_q = int(rng.integers(0, S)), int(rng.integers(0, S)), int(rng.integers(0, S))
    v_lone, v_anti = col(), col()
    lone, anti, zero = np.zeros((R, S), np.float32), np.zeros((R, S), np.float32), np.zeros((R, S), np.float32)
    lone[:, c_lone], anti[:, c_anti] = v_lone, -v_anti
    db = np.concatenate([base, np.stack([full, alike, half, lone, anti, zero])])
    FULL, ALIKE, HALF, LONE, ANTI, ZERO = range(150, 156)
    ne = len(db)
    n0, n1, j0, j1 = int(rng.integers(0, S)), int(rng.integers(0, S)), int(rng.integers(0, S)), int(rng.integers(0, S))
    q_one = np.zeros_like(full)                                        # m = 1 at shift n0: column j0 of the entry rolled by n0
    q_one[:, j0] = np.roll(full, -n0, axis=1)[:, j0]
    q_but = np.roll(full, -n1, axis=1)                                 # m = S - 1 at every shift: one column of the rolled entry missing
    q_but[:, j1] = 0.0
    q_lone, q_anti = np.zeros_like(full), np.zeros_like(full)
    q_lone[:, c_q], q_anti[:, c_q] = v_lone, v_anti
    qs = np.stack([q_one, q_but, alike, half, q_lone, q_anti, zero, pr.random_database(1, p, seed=S)[0]])
    D = pr.distance_table(qs, db)
    # what the reference itself says of the planted pairs
    assert D[0, FULL, n0] <= 1e-15 and D[1, FULL, n1] <= 1e-15 and np.all(D[2, ALIKE] == D[2, ALIKE, 0]) and D[2, ALIKE, 0] <= 1e-15
    assert S % 2 or (D[3, HALF, 0] == D[3, HALF, S // 2] and D[3, HALF, 0] <= 1e-15)
    n_lone, n_anti = (c_lone - c_q) % S, (c_anti - c_q) % S
    assert D[4, LONE, n_lone] <= 1e-15 and np.array_equal(np.delete(D[4, LONE], n_lone), np.ones(S - 1))
    assert abs(D[5, ANTI, n_anti] - 2.0) <= 1e-15 and np.array_equal(np.delete(D[5, ANTI], n_anti), np.ones(S - 1))
    assert np.array_equal(D[6], np.ones((ne, S))) and np.array_equal(D[:, ZERO], np.ones((len(qs), S)))
    ctx.places_reset(p)
    ctx.places_add(db)
    for k, first, last in [(1, 0, ne), (64, 0, ne), (5, 3, ne - 2)]:
        idx, shift, dist = ctx.places_query(qs, k, first, last)
        check_search(D, first, last, k, idx, shift, dist, "%d x %d edges, k %d of [%d, %d)" % (R, S, k, first, last))
    idx, shift, dist = ctx.places_query(qs, 4)
    for q, entry, n in [(0, FULL, n0), (1, FULL, n1), (2, ALIKE, 0), (3, HALF, 0), (4, LONE, n_lone)]:
        assert (idx[q, 0], shift[q, 0]) == (entry, n) and abs(dist[q, 0]) <= TOL_D, (R, S, q, idx[q, 0], shift[q, 0], dist[q, 0])
    assert idx[6].tolist() == [0, 1, 2, 3] and shift[6].tolist() == [0] * 4 and dist[6].tolist() == [1.0] * 4          # m = 0 everywhere
    # one entry at a time: ties by shift, m = 0 at all shifts but the one that costs 2, both descriptors zero
    for q, entry, n, d in [(2, ALIKE, 0, 0.0), (3, HALF, 0, 0.0), (5, ANTI, 1 if n_anti == 0 else 0, 1.0), (6, ZERO, 0, 1.0),
                           (5, ZERO, 0, 1.0), (6, FULL, 0, 1.0)]:
        i, s, dd = ctx.places_query(qs[q:q + 1], 2, entry, entry + 1)
        assert i.tolist() == [[entry, -1]] and s.tolist() == [[n, 0]] and abs(dd[0, 0] - d) <= TOL_D and np.isposinf(dd[0, 1]), (R, S, q, entry, s, dd)
        assert d == 0.0 or dd[0, 0] == d                                # (1 at m = 0 is the rule's constant, not a sum)
    # the entry rolled by every shift finds the entry at that shift
    rolled = np.stack([np.roll(full, -n, axis=1) for n in range(S)])
    for n in (0, 1, S - 1):
        assert pr.distance(rolled[n], full) == (pytest.approx(0.0, abs=1e-15), n)
    idx, shift, dist = ctx.places_query(rolled, 1)
    assert np.all(idx[:, 0] == FULL) and np.array_equal(shift[:, 0], np.arange(S)) and np.abs(dist).max() <= TOL_D, (R, S)
    print("%d x %d: rolled entry |dist| %.3g" % (R, S, np.abs(dist).max()))
