"""The scenes that drive the ball walk of the radius descriptors (features.hip ball_walk) past one 64-row batch, defined once for the
device tests of tests/test_gpu_fpfh_map_updates.py, and what makes them those scenes - asserted of the geometry and of the numpy
references alone, without a device:
  - how many (y, z) rows of the grid the ball of a point reaches at each forced cell edge, computed with the walk's own arithmetic
    (`ball_rows`): one batch at 0.5, two at 0.2, seven at 0.1 for the points inside the box;
  - the cap at which points become crowded in a SECOND or later batch (`crowded_batch`: the batch that holds neighbour cap + 1 in the
    walk's row order);
  - the references' own excluded share stays within EDGE_CAP on every scene, so that the device tests' assert_matches compares every
    point it can."""
import functools

import numpy as np

import fpfh_radius_ref as rr
import fpfh_ref as fr
import normals_ref as nr
from test_fpfh_radius_reference import next_radius, unit_normals
from test_fpfh_reference import EDGE_CAP
from test_normals_reference import lattice

WAVE = 64                                   # rows per batch of ball_walk (kWave)
BOX_N, BOX_SIDE, BALL_RADIUS = 557, 3.0, 1.0
CELLS = (0.5, 0.2, 0.1)
BALL_CAP = 60                               # max_neighbors of the crowded scene: inner points of the box have about 85 neighbours
LATTICE_CELLS = (0.25, 0.125)
K_FORMS = ((32, 0.0), (8, 0.6))             # (k, search_radius) of the k-form on the 0.1-cell index


@functools.lru_cache(maxsize=None)
def box_scene():
    """BOX_N points uniform in a cube of BOX_SIDE metres with seeded unit normals; the arrays are shared: do not write to them"""
    cloud = np.random.default_rng(3100 + BOX_N).uniform(0.0, BOX_SIDE, (BOX_N, 3)).astype(np.float32)
    return cloud, unit_normals(BOX_N, 3)


@functools.lru_cache(maxsize=None)
def lattice_scene():
    """the lattice of the scenes edge:at / edge:above (tests/test_fpfh_radius_reference.py): 4 x 4 x 4 points, spacing 0.25"""
    return lattice((4, 4, 4)), unit_normals(64)


LATTICE_RADII = {"at": 0.5, "above": next_radius(0.5)}


@functools.lru_cache(maxsize=None)
def box_reference(cap=rr.MAX_CAP):
    cloud, normals = box_scene()
    return rr.fpfh_radius_reference(cloud, normals, BALL_RADIUS, cap)


@functools.lru_cache(maxsize=None)
def lattice_reference(which):
    cloud, normals = lattice_scene()
    return rr.fpfh_radius_reference(cloud, normals, LATTICE_RADII[which])


@functools.lru_cache(maxsize=None)
def box_k_reference(k, search_radius):
    cloud, normals = box_scene()
    return fr.fpfh_reference(cloud, normals, k=k, search_radius=search_radius)


def grid_of(cloud, cell):
    """origin and dims of the grid that context.hip build_grid_at lays over a cloud at a forced cell edge -> (origin [3], dims [3])"""
    mn, mx = cloud.min(axis=0).astype(np.float64), cloud.max(axis=0).astype(np.float64)
    return mn, (np.floor((mx - mn) * (1.0 / cell)) + 1).astype(np.int64)


def _cell(x, n):
    return np.clip(np.floor(x), 0, n - 1).astype(np.int64)


def ball_rows(cloud, origin, dims, cell, radius):
    """per point the rows ball_walk lays out for it (nrows), and y0, z0, nyr of its row box, with the kernel's arithmetic in double"""
    inv_h = 1.0 / cell
    f = (cloud.astype(np.float64) - origin) * inv_h
    reach = np.sqrt(np.float64(rr.r2_of(radius))) * inv_h * 1.00001 + 1e-4
    y0, y1 = _cell(f[:, 1] - reach, dims[1]), _cell(f[:, 1] + reach, dims[1])
    z0, z1 = _cell(f[:, 2] - reach, dims[2]), _cell(f[:, 2] + reach, dims[2])
    nyr = y1 - y0 + 1
    return nyr * (z1 - z0 + 1), y0, z0, nyr


def crowded_batch(cloud, origin, dims, cell, radius, cap):
    """for every point with more than cap neighbours the batch of rows (0 = the first 64) in which the walk meets neighbour cap + 1 and
    stops; -1 for the others.  The walk takes the rows in (z, y) order, 64 a batch, and counts a batch's candidates before the next"""
    nrows, y0, z0, nyr = ball_rows(cloud, origin, dims, cell, radius)
    f = (cloud.astype(np.float64) - origin) * (1.0 / cell)
    cy, cz = _cell(f[:, 1], dims[1]), _cell(f[:, 2], dims[2])
    D = nr.d2_f32(cloud, cloud)
    out = np.full(len(cloud), -1, np.int64)
    for i in range(len(cloud)):
        j = np.flatnonzero(D[i] < rr.r2_of(radius))
        if len(j) > cap:
            out[i] = np.sort(((cz[j] - z0[i]) * nyr[i] + (cy[j] - y0[i])) // WAVE)[cap]
    return out


def inner(cloud, radius):
    """the points whose ball lies inside the cloud's box in y and z: no row of theirs is clamped away"""
    lo, hi = cloud.min(axis=0), cloud.max(axis=0)
    return ((cloud[:, 1:] - radius >= lo[1:]) & (cloud[:, 1:] + radius <= hi[1:])).all(axis=1)


# ---- the regimes, from the geometry
def test_the_forced_cell_edges_put_the_ball_below_between_and_above_the_batch_sizes():
    cloud, _ = box_scene()
    mid = inner(cloud, BALL_RADIUS)
    assert mid.sum() >= 20
    rows = {}
    for cell in CELLS:
        origin, dims = grid_of(cloud, cell)
        rows[cell] = ball_rows(cloud, origin, dims, cell, BALL_RADIUS)[0]
        print("cell %.2f: dims %s, rows min %d max %d, inner %d .. %d" % (cell, dims, rows[cell].min(), rows[cell].max(), rows[cell][mid].min(),
                                                                         rows[cell][mid].max()))
    # 2 R / h + 1 cells a side where the box does not cut the ball: 5 x 5 rows at 0.5, 11 x 11 at 0.2, 21 x 21 at 0.1
    assert rows[0.5].max() <= WAVE                                                  # one batch for every point
    assert np.all(rows[0.2][mid] > WAVE) and rows[0.2].max() <= 2 * WAVE            # two batches inside the box, never three
    assert ((rows[0.2] > WAVE) & (rows[0.2] <= 2 * WAVE)).sum() >= 100 and (rows[0.2] <= WAVE).sum() >= 20
    assert np.all(rows[0.1][mid] > 6 * WAVE) and (rows[0.1] > 2 * WAVE).mean() > 0.9    # seven batches inside, three and more nearly everywhere
    assert rows[0.1].min() > WAVE                                                   # ... and no point of the box with one batch only


def test_the_cap_crowds_points_in_a_second_or_later_batch():
    cloud, _ = box_scene()
    ref, free = box_reference(BALL_CAP), box_reference()
    assert 20 <= ref["n_crowded"] < ref["n_used"] // 2 and ref["m_max"] == BALL_CAP + 1 and free["n_crowded"] == 0 and free["m_max"] > BALL_CAP
    assert np.array_equal(ref["crowded"], free["m"] > BALL_CAP) and not ref["has_spfh"][ref["crowded"]].any() and not ref["counts"][ref["crowded"]].any()
    # their neighbours get nothing from them: a point beside a crowded one has another descriptor than under the lifted cap
    changed = ~ref["crowded"] & (ref["fpfh"].view(np.uint32) != free["fpfh"].view(np.uint32)).any(axis=1)
    assert changed.sum() >= ref["n_crowded"]
    for cell, least in ((0.2, 1), (0.1, 2)):
        origin, dims = grid_of(cloud, cell)
        b = crowded_batch(cloud, origin, dims, cell, BALL_RADIUS, BALL_CAP)
        assert np.array_equal(b >= 0, ref["crowded"])
        print("cell %.2f: crowded points stop in batches %s" % (cell, np.bincount(b[b >= 0])))
        assert (b >= least).sum() >= 10                          # the early return inside a later batch is taken
    origin, dims = grid_of(cloud, 0.5)
    assert crowded_batch(cloud, origin, dims, 0.5, BALL_RADIUS, BALL_CAP).max() == 0


def test_the_lattice_lies_on_the_faces_of_both_forced_grids():
    cloud, _ = lattice_scene()
    for cell in LATTICE_CELLS:
        origin, dims = grid_of(cloud, cell)
        f = (cloud.astype(np.float64) - origin) / cell
        assert np.array_equal(f, np.rint(f)) and list(dims) == [int(round(0.75 / cell)) + 1] * 3      # every point on a face; the max corner in the last cell
        assert f.max() == dims[0] - 1
    # the ball of edge:at ends exactly on a face: two steps of the lattice are two cells of 0.25 and four of 0.125
    assert rr.r2_of(LATTICE_RADII["at"]) == np.float32(0.25) and np.sqrt(0.25) / 0.25 == 2.0 and np.sqrt(0.25) / 0.125 == 4.0
    at, above = lattice_reference("at"), lattice_reference("above")
    assert at["m_max"] == 27 and above["m_max"] == 30


# ---- the references stay inside the edge-near cap on every scene, so the device comparison exempts (next to) nothing
def test_the_references_of_these_scenes_stay_within_the_edge_cap():
    refs = {"box": box_reference(), "box capped": box_reference(BALL_CAP), "lattice at": lattice_reference("at"),
            "lattice above": lattice_reference("above")}
    refs.update({"k-form %r" % (kf,): box_k_reference(*kf) for kf in K_FORMS})
    for name, r in refs.items():
        assert r["excluded"].sum() <= EDGE_CAP * max(r["n_used"], 1), (name, int(r["excluded"].sum()), r["n_used"])
    assert box_reference()["n_out"] == BOX_N and box_reference()["m_sum"] / BOX_N > 40
    k32, k8 = box_k_reference(*K_FORMS[0]), box_k_reference(*K_FORMS[1])
    assert k32["m"].min() == 32 and k8["m"].max() == 8 and (k8["m"] < 8).any()           # the bound leaves some points short of k
