"""The numpy reference of the place-recognition rules (tests/places_ref.py) pinned on its own, without a device: the direction of the
shift, empty columns, the tie-breaks, the bulk evaluation against the literal one, and the drive-and-revisit check with its recorded counts."""
import numpy as np
import pytest

import places_ref as pr
from dcreg_amd import api

P = api.place_params()


def polar_cloud(n, p, seed, turn_sectors=0):
    """n points well inside their bins (ring and sector coordinates 0.2 .. 0.8 into a bin), the whole cloud turned about z by
    -turn_sectors sectors: what a sensor yawed by +turn_sectors sectors at the same place sees"""
    rng = np.random.default_rng(seed)
    ring = rng.integers(0, p.n_rings, n) + rng.uniform(0.2, 0.8, n)
    sector = rng.integers(0, p.n_sectors, n) + rng.uniform(0.2, 0.8, n)
    rho = ring * p.max_range / p.n_rings
    th = (sector - turn_sectors) * 2 * np.pi / p.n_sectors
    return np.stack([rho * np.cos(th), rho * np.sin(th), rng.uniform(-1.5, 4.0, n)], 1).astype(np.float32)


def test_a_descriptor_takes_the_maximum_height_of_every_bin_and_zero_for_an_empty_one():
    p = api.place_params(4, 8, 8.0, 1.0, 2.0)
    cloud = np.array([[2.5, 0.1, 1.0], [2.6, 0.2, 3.0], [2.7, 0.3, -5.0],      # ring 1, sector 0: max 3 + 2
                      [0.0, 3.9, 0.5],                                            # ring 1, sector 2 (azimuth 90 deg)
                      [-7.9, -0.1, -1.0],                                         # ring 3, sector 4 (just past 180 deg)
                      [0.5, 0.5, 9.0], [8.0, 0.0, 9.0], [20.0, 1.0, 9.0],         # inside min_range, at max_range, beyond
                      [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [2.0, 2.0, np.nan]], np.float32)
    d = pr.descriptor(cloud, p)
    want = np.zeros((4, 8), np.float32)
    want[1, 0], want[1, 2], want[3, 4] = 5.0, 2.5, 1.0
    assert np.array_equal(d, want)
    assert pr.info([cloud], p) == {"n_in": 11, "n_finite": 8, "n_used": 5}
    assert pr.ambiguous(cloud, p) == 1                        # (0, 3.9): its azimuth is a quarter turn, a sector edge of 8
    assert pr.ambiguous(cloud[[0, 1, 2, 4]], p) == 0


@pytest.mark.parametrize("n", [0, 1, 7, 30, 59])
def test_rolled_columns_have_distance_zero_at_the_shift_the_direction_rule_gives(n):
    """a sensor yawed by +n sectors sees column j + n of the entry in its column j: np.roll by -n; the best shift is n, not -n"""
    c = pr.descriptor(polar_cloud(2_000, P, seed=1), P)
    q = np.roll(c, -n, axis=1)
    D = pr.distances(q, c)
    assert D[n] <= 1e-15
    assert pr.distance(q, c)[1] == n and pr.distance(q, c)[0] <= 1e-15
    if (2 * n) % P.n_sectors:                                   # (half a turn is its own opposite)
        assert D[(-n) % P.n_sectors] > 0.01
    # ... and that is what rotating the cloud itself by whole sectors does
    turned = polar_cloud(2_000, P, seed=1, turn_sectors=n)
    assert pr.ambiguous(turned, P) == 0
    assert np.array_equal(pr.descriptor(turned, P), q)
    # the start pose of api.place_guess maps the turned cloud back onto the original
    T = api.place_guess(n, P.n_sectors)
    back = turned.astype(np.float64) @ T[:3, :3].T
    assert np.abs(back - polar_cloud(2_000, P, seed=1)).max() < 1e-4


def test_empty_columns_are_skipped_and_no_common_column_gives_one():
    rng = np.random.default_rng(2)
    c = rng.uniform(0.5, 6.0, (P.n_rings, P.n_sectors)).astype(np.float32)
    q = c.copy()
    q[:, 10:25] = 0.0                                           # the query saw nothing there: those columns do not count
    assert pr.distance(q, c) == (pytest.approx(0.0, abs=1e-15), 0)
    full = pr.distances(c, c)
    part = pr.distances(q, c)
    assert part[0] <= 1e-15 and np.all(part[1:] > 0.01) and np.all(full[1:] > 0.01)
    # at shift n only the columns whose partner has a norm too are averaged
    n = 7
    j = np.array([k for k in range(P.n_sectors) if not 10 <= k < 25])
    cj = c[:, (j + n) % P.n_sectors].astype(np.float64)
    qj = q[:, j].astype(np.float64)
    want = np.mean(1.0 - (qj * cj).sum(0) / (np.sqrt((qj * qj).sum(0)) * np.sqrt((cj * cj).sum(0))))
    assert abs(part[n] - want) <= 1e-15
    # no column in common at any shift: 1 everywhere, shift 0
    zero = np.zeros_like(c)
    assert np.array_equal(pr.distances(zero, c), np.ones(P.n_sectors)) and pr.distance(zero, c) == (1.0, 0)
    assert np.array_equal(pr.distances(c, zero), np.ones(P.n_sectors)) and pr.distance(zero, zero) == (1.0, 0)
    one = np.zeros_like(c)
    one[:, 3] = 1.0
    lone = np.zeros_like(c)
    lone[:, 40] = 2.0
    D = pr.distances(one, lone)                                 # one column each: they meet at shift 37 only
    assert D[37] <= 1e-15 and np.array_equal(np.delete(D, 37), np.ones(P.n_sectors - 1))


def test_ties_break_on_the_smallest_shift_and_on_the_index():
    rng = np.random.default_rng(3)
    col = rng.uniform(0.5, 6.0, P.n_rings).astype(np.float32)
    same = np.repeat(col[:, None], P.n_sectors, 1)              # every column alike: every shift attains the minimum
    assert pr.distance(same, same)[1] == 0
    half = np.tile(rng.uniform(0.5, 6.0, (P.n_rings, P.n_sectors // 2)).astype(np.float32), 2)      # period 30: shifts 0 and 30 tie
    D = pr.distances(half, half)
    assert D[0] == D[30] and pr.distance(half, half)[1] == 0
    other = rng.uniform(0.5, 6.0, (P.n_rings, P.n_sectors)).astype(np.float32)
    db = np.stack([other, half, same, half, half])
    idx, shift, dist = pr.search(half[None], db, 0, 5, 5)
    assert idx[0].tolist() == [1, 3, 4, 2, 0] or idx[0].tolist() == [1, 3, 4, 0, 2]
    assert idx[0, :3].tolist() == [1, 3, 4] and shift[0, :3].tolist() == [0, 0, 0] and np.all(dist[0, :3] == dist[0, 0])
    assert np.all(np.diff(dist[0]) >= 0)
    idx, shift, dist = pr.search(half[None], db, 2, 5, 4)       # a sub-range, and a slot beyond it
    assert idx[0].tolist() == [3, 4, 2, -1] and shift[0, 3] == 0 and dist[0, 3] == np.inf
    idx, shift, dist = pr.search(half[None], db, 2, 2, 2)
    assert idx.tolist() == [[-1, -1]] and shift.tolist() == [[0, 0]] and np.all(np.isinf(dist))


def test_the_bulk_evaluation_is_the_literal_one():
    p = api.place_params(6, 24, 30.0)
    db = pr.random_database(40, p, seed=8)
    qs = pr.random_database(5, p, seed=9)
    qs[2] = db[13]
    D = pr.distance_table(qs, db, block=16)
    for q in range(len(qs)):
        for e in range(len(db)):
            assert np.abs(D[q, e] - pr.distances(qs[q], db[e])).max() <= 1e-15, (q, e)
    assert D[2, 13].min() <= 1e-15 and np.array_equal(D[:, 11], np.ones((5, 24)))        # (entry 11 is all zero)


def test_the_revisits_of_a_drive_find_their_keyframes():
    """120 keyframes through a 4 M-point prior map, 24 revisits at a random yaw up to 1.5 m off the path (seed 5).  Recorded with this file:
    0 ambiguous points, 23 of the 24 top-1 entries within one keyframe of the true one, every such shift within one sector of the true yaw"""
    sc = pr.drive_scene()
    p = sc["params"]
    assert len(sc["frames"]) == 120 and len(sc["rev_frames"]) == 24
    assert sum(pr.ambiguous(f, p) for f in sc["frames"] + sc["rev_frames"]) == 0
    db = np.stack([pr.descriptor(f, p) for f in sc["frames"]])
    qs = np.stack([pr.descriptor(f, p) for f in sc["rev_frames"]])
    idx, shift, dist = pr.search(qs, db, 0, len(db), 1)
    near = np.abs(idx[:, 0] - sc["rev_of"]) <= 1
    print("top-1 within one keyframe:", int(near.sum()), "of", len(near))
    assert near.sum() >= 20
    for q in np.flatnonzero(near):
        rel = np.linalg.inv(sc["poses"][idx[q, 0]]) @ sc["rev_poses"][q]
        yaw = np.arctan2(rel[1, 0], rel[0, 0])
        off = (shift[q, 0] * 2 * np.pi / p.n_sectors - yaw + np.pi) % (2 * np.pi) - np.pi
        assert abs(off) <= 2 * np.pi / p.n_sectors, (q, off)
