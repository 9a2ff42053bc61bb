"""The numpy reference of the place-recognition rules of include/dcreg.h, written out literally: Scan Context descriptors, the column-shift
distance, the exhaustive top-k search - and the seeded scenes the place tests share.  The device is held to this file, never to a second
device run.  p is an api.PlaceParams (or anything with n_rings, n_sectors, max_range, min_range, z_offset)."""
import numpy as np

TWO_PI = 2.0 * np.pi


def bin_coords(cloud, p):
    """-> (used [n] bool, a [n], b [n]): which points the descriptor uses, and their ring and sector coordinates (double)"""
    xyz = np.asarray(cloud, np.float32)[:, :3]
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(xyz).all(1)
        r2 = x * x + y * y
        used = finite & (r2 >= p.min_range * p.min_range) & (r2 < p.max_range * p.max_range)
        a = np.sqrt(r2) * p.n_rings / p.max_range
        th = np.arctan2(y, x)
        th = np.where(th < 0.0, th + TWO_PI, th)
        b = th * p.n_sectors / TWO_PI
    return used, a, b


def descriptor(cloud, p):
    """the descriptor of one cloud -> [n_rings, n_sectors] float32"""
    xyz = np.asarray(cloud, np.float32)[:, :3]
    used, a, b = bin_coords(xyz, p)
    ring = np.minimum(np.floor(a[used]).astype(np.int64), p.n_rings - 1)
    sector = np.minimum(np.floor(b[used]).astype(np.int64), p.n_sectors - 1)
    val = (xyz[used, 2].astype(np.float64) + p.z_offset).astype(np.float32)
    d = np.full(p.n_rings * p.n_sectors, -np.inf, np.float32)
    np.maximum.at(d, ring * p.n_sectors + sector, val)
    d[np.isneginf(d)] = 0.0
    return d.reshape(p.n_rings, p.n_sectors)


def info(clouds, p):
    """dcreg_place_info of a call's clouds"""
    n_in = n_finite = n_used = 0
    for c in clouds:
        c = np.asarray(c, np.float32)
        n_in += len(c)
        n_finite += int(np.isfinite(c[:, :3]).all(1).sum())
        n_used += int(bin_coords(c, p)[0].sum())
    return {"n_in": n_in, "n_finite": n_finite, "n_used": n_used}


def ambiguous(cloud, p, guard=1e-9):
    """used points whose ring or sector coordinate lies within `guard` of an integer: they may fall in either neighbouring bin"""
    used, a, b = bin_coords(cloud, p)
    a, b = a[used], b[used]
    return int(((np.abs(a - np.round(a)) <= guard) | (np.abs(b - np.round(b)) <= guard)).sum())


def column_norms(d):
    d = np.asarray(d, np.float32).astype(np.float64)
    return np.sqrt((d * d).sum(0))


def distances(q, c):
    """D_n of a query descriptor q and an entry c, n = 0 .. n_sectors - 1 (double), the rule written out"""
    q = np.asarray(q, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    S = q.shape[1]
    nq, nc = column_norms(q), column_norms(c)
    D = np.ones(S)
    for n in range(S):
        cs, ncs = np.roll(c, -n, axis=1), np.roll(nc, -n)          # column j of cs is column (j + n) mod S of c
        ok = (nq > 0.0) & (ncs > 0.0)
        m = int(ok.sum())
        if m:
            D[n] = np.sum(1.0 - (q[:, ok] * cs[:, ok]).sum(0) / (nq[ok] * ncs[ok])) / m
    return D


def distance(q, c):
    """-> (min_n D_n, the smallest n that attains it)"""
    D = distances(q, c)
    n = int(np.argmin(D))               # (argmin returns the first minimum)
    return float(D[n]), n


def distance_table(qs, db, block=256):
    """D[query, entry, n] for every pair, the same rule evaluated in bulk (test_places_reference.py holds it to `distances`)"""
    qs = np.asarray(qs, np.float32).astype(np.float64)
    db = np.asarray(db, np.float32).astype(np.float64)
    nq, R, S = qs.shape
    ne = db.shape[0]
    out = np.ones((nq, ne, S))
    if nq == 0 or ne == 0:
        return out
    qn = np.sqrt((qs * qs).sum(1))
    cn = np.sqrt((db * db).sum(1))
    j = np.arange(S)
    col = (j[None, :] + j[:, None]) % S                      # col[n, j] = (j + n) mod S
    for e0 in range(0, ne, block):
        c, n_c = db[e0:e0 + block], cn[e0:e0 + block]
        for qi in range(nq):
            dots = np.einsum("rj,erl->ejl", qs[qi], c)      # [entry, query column j, entry column l]
            den = qn[qi][None, :, None] * n_c[:, None, :]
            ok = den > 0.0
            with np.errstate(invalid="ignore", divide="ignore"):
                term = np.where(ok, 1.0 - dots / den, 0.0)
            t = term[:, j[None, :], col]                   # [entry, n, j]
            m = ok[:, j[None, :], col].sum(2)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[qi, e0:e0 + block] = np.where(m > 0, t.sum(2) / np.maximum(m, 1), 1.0)
    return out


def small_table(qs, db):
    """D[query, entry, n] of distance_table for grids of a few bins and databases of 10^5 entries and more: the rule written out per
    (query, n, j) and evaluated over all entries at once (test_places_edge_scenes.py holds it to `distances`).  The terms of a shift are
    added in the order of the query's columns, as `distances` adds them"""
    qs = np.asarray(qs, np.float32).astype(np.float64)
    db = np.asarray(db, np.float32).astype(np.float64)
    nq, R, S = qs.shape
    ne = db.shape[0]
    out = np.ones((nq, ne, S))
    if nq == 0 or ne == 0:
        return out
    qn = np.sqrt((qs * qs).sum(1))
    cn = np.sqrt((db * db).sum(1))
    for qi in range(nq):
        for n in range(S):
            total, m = np.zeros(ne), np.zeros(ne, np.int64)
            for j in range(S):
                if not qn[qi, j] > 0.0:
                    continue
                l = (j + n) % S
                ok = cn[:, l] > 0.0
                dot = np.zeros(ne)
                for r in range(R):
                    dot += qs[qi, r, j] * db[:, r, l]
                with np.errstate(invalid="ignore", divide="ignore"):
                    total += np.where(ok, 1.0 - dot / (qn[qi, j] * cn[:, l]), 0.0)
                m += ok
            out[qi, :, n] = np.where(m > 0, total / np.maximum(m, 1), 1.0)
    return out


def search_table(D, first, last, k):
    """the search on a distance table D[query, entry, n] -> (idx [nq, k] int32, shift [nq, k] int32, dist [nq, k] float64)"""
    nq = D.shape[0]
    idx = np.full((nq, k), -1, np.int32)
    shift = np.zeros((nq, k), np.int32)
    dist = np.full((nq, k), np.inf)
    if last > first:
        best = D[:, first:last].min(2)
        arg = D[:, first:last].argmin(2)                     # the smallest shift that attains it
        for q in range(nq):
            order = np.lexsort((np.arange(first, last), best[q]))[:k]          # by (distance, index)
            idx[q, :len(order)] = first + order
            shift[q, :len(order)] = arg[q, order]
            dist[q, :len(order)] = best[q, order]
    return idx, shift, dist


def search(qs, db, first, last, k):
    return search_table(distance_table(qs, db), first, last, k)


# ---- the scenes the tests share
DRIVE_KEYFRAMES, DRIVE_REVISITS = 120, 24
_drive_cache = {}


def drive_scene(seed=5):
    """A 120-keyframe drive through a 4 M-point prior map (440 m square) and 24 revisits: sweeps taken later near seeded keyframes, up to
    1.5 m off the path, at a random yaw.  -> dict: world, params (max_range 30), poses, frames (the keyframes' clouds), rev_of (the keyframe
    each revisit is near), rev_poses, rev_frames"""
    if seed in _drive_cache:
        return _drive_cache[seed]
    from dcreg_amd import api, scenes
    world, _ = scenes.scene_prior_map(n_map=4_000_000, extent=220.0)
    poses, frames = scenes.drive(world, DRIVE_KEYFRAMES, n_frame=8_000, seed=seed)
    rev_of, rev_poses, rev_frames = scenes.revisits(world, poses, DRIVE_REVISITS, 1.5, 8_000, seed=seed + 100)
    out = {"world": world, "params": api.place_params(max_range=30.0), "poses": [np.asarray(T, np.float64) for T in poses], "frames": frames,
           "rev_of": rev_of, "rev_poses": rev_poses, "rev_frames": rev_frames}
    _drive_cache[seed] = out
    return out


def random_database(n, p, seed=3):
    """n seeded random descriptors [n, n_rings, n_sectors] float32 with zero columns and duplicates among them: heights in [0, 6), every
    fifth descriptor with a run of empty columns, every seventh a copy of an earlier one, one all-zero descriptor"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, 6.0, (n, p.n_rings, p.n_sectors)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.2] = 0.0
    for e in range(0, n, 5):
        j0, w = rng.integers(0, p.n_sectors), rng.integers(1, max(2, p.n_sectors // 2))
        d[e][:, (j0 + np.arange(w)) % p.n_sectors] = 0.0
    for e in range(7, n, 7):
        d[e] = d[rng.integers(0, e)]
    if n > 11:
        d[11] = 0.0
    return d
