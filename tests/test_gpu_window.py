"""The window index of a large map (context.hpp, context.hip roi_ensure) at its edges.  Every case runs a context that searches the window
("roi_index" 2, "roi_margin" 0 unless stated) beside one that searches the whole map ("roi_index" 0), makes the same calls on both and
asks for bitwise the same sums.  The scene is sparse (scenes.scene_sparse_map: map points ~ 1.4 m apart), so that a window whose box is
short by a fraction of a metre at the frame's edge changes the neighbours of the queries there; each case first proves, through the whole
map's k-NN, that enough queries have a neighbour outside the box of a window built for radius 0.5 for such an error to show."""
import functools

import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from oracle import pyoracle as po
from test_gpu_configs import assert_runs_equal, cfg_pair
from test_gpu_parity import assert_lin_equal
from test_gpu_round6 import _same_sums

pytestmark = pytest.mark.gpu

HINT = 0.5                       # the maps' radius hint (dcreg_set_target)
CERT_MARGIN = 0.05               # the default "cert_margin"
FAR = (2500.0, -1800.0, 35.0)    # case H: the scene this far from the origin


@functools.lru_cache(maxsize=None)
def _scene(offset=(0.0, 0.0, 0.0)):
    return h.scene_sparse_map(offset=offset)


def _pad(radius, hint=HINT):
    """context.hip roi_pad_for: what a launch at this radius needs of the window beyond the source's box"""
    return max(radius, hint) * (1.0 + CERT_MARGIN) * 1.001 + 1e-3


def _source_box(src, T):
    """context.hip source_box_at: the box of the eight corners of the source's body-frame box at pose T"""
    mn, mx = src.min(0).astype(np.float64), src.max(0).astype(np.float64)
    c = np.array([[mx[0] if k & 1 else mn[0], mx[1] if k & 2 else mn[1], mx[2] if k & 4 else mn[2]] for k in range(8)])
    w = c @ T[:3, :3].T + T[:3, 3]
    return w.min(0), w.max(0)


def _prm(radius):
    return api.default_lin_params(radius, 0)


def _at(T, dx=0.0, dy=0.0, dz=0.0, roll=0.0, pitch=0.0, yaw=0.0):
    """T moved in its own frame, then shifted in the map frame by (dx, dy, dz)"""
    M = T @ h.pose6d_matrix(0.0, 0.0, 0.0, roll, pitch, yaw)
    M[:3, 3] += (dx, dy, dz)
    return M


def _pair(tgt, src, margin=0.0, opts=None, hint=HINT):
    whole, win = api.Context(0), api.Context(0)
    whole.set_option("roi_index", 0)
    win.set_option("roi_index", 2)
    win.set_option("roi_margin", margin)
    for c in (whole, win):
        for k, v in (opts or {}).items():
            c.set_option(k, v)
        c.set_target(tgt, hint)
        c.set_source(src)
    return whole, win


def _edge_queries(whole, tgt, src, T, radius=2.0, built_for=0.5):
    """queries at pose T whose five nearest map points (whole map, all within `radius`) are not all inside the box of a window built at T
    for radius `built_for`: each of them would lose a neighbour if a launch at `radius` searched that window"""
    q = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    idx, d2 = whole.knn(q, 5, 0.0)
    assert (idx >= 0).all()
    nb = tgt[idx].astype(np.float64)                                          # (original indices)
    assert np.allclose(((nb - q[:, None, :].astype(np.float64)) ** 2).sum(-1), d2, rtol=1e-4, atol=1e-6)
    lo, hi = _source_box(src, T)
    p = _pad(built_for)
    out = ((nb < lo - p) | (nb > hi + p)).any(-1).any(-1)
    return int((out & (d2[:, 4] <= radius * radius)).sum())


def _check_window(win, tgt64, cell):
    """case J: the window holds at least the map's points inside its box and at most those inside the box grown by 3 whole-map cells;
    it is active exactly when it holds some but not all of the map"""
    info = win.roi_info()
    lo, hi = np.array(info["box_min"]), np.array(info["box_max"])
    inside = int(np.all((tgt64 >= lo) & (tgt64 <= hi), 1).sum())
    grown = int(np.all((tgt64 >= lo - 3 * cell) & (tgt64 <= hi + 3 * cell), 1).sum())
    n = len(tgt64)
    assert info["active"] == (0 < info["points"] < n), info
    if info["points"] == 0:            # no window: nothing of the map near the box, or all of it
        assert inside == 0 or grown == n, (info, inside, grown)
    else:
        assert inside <= info["points"] <= grown, (info, inside, grown)
    return info


class _Walk:
    """the same linearisations on both contexts; sums bitwise equal, the window checked after every launch"""

    def __init__(self, whole, win, tgt):
        self.whole, self.win, self.tgt64 = whole, win, tgt.astype(np.float64)
        self.cell = whole.index_info().cell

    def __call__(self, T, radii=(0.5, 2.0)):
        for r in radii:
            a = self.whole.linearize(T[:3, :3], T[:3, 3], _prm(r))
            b = self.win.linearize(T[:3, :3], T[:3, 3], _prm(r))
            assert _same_sums(a, b), (r, a["n_eff"], b["n_eff"])
            self.info = _check_window(self.win, self.tgt64, self.cell)
        return a

    @property
    def built(self):
        return self.win.roi_info()["windows_built"]


def _close(*cs):
    for c in cs:
        c.close()


# ---------------------------------------------------------------- A, H, J: geometry, near the origin and far from it
@pytest.mark.timeout(600)
@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), FAR], ids=["origin", "far"])
def test_window_geometry(offset):
    tgt, src, T = _scene(offset)
    whole, win = _pair(tgt, src)
    try:
        assert _edge_queries(whole, tgt, src, T) >= 15
        walk = _Walk(whole, win, tgt)
        a = walk(T)
        assert a["n_eff"] > len(src) // 2 and walk.info["active"]
        d30 = np.deg2rad(30.0)
        for kw in (dict(roll=d30), dict(roll=-d30), dict(pitch=d30), dict(pitch=-d30), dict(pitch=np.pi / 2), dict(yaw=np.pi)):
            walk(_at(T, **kw))
        lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
        # boxes that run past the grid (the cell range is clamped), at two corners of the map
        walk(_at(T, dx=hi[0] - 6.0 - T[0, 3], dy=hi[1] - 6.0 - T[1, 3]))
        walk(_at(T, dx=lo[0] + 6.0 - T[0, 3], dy=lo[1] + 6.0 - T[1, 3], yaw=0.7))
        # wholly off the map: no window, nothing found; then back onto it
        k = walk.built
        off = walk(_at(T, dx=5000.0))
        assert off["n_eff"] == 0 and not walk.info["active"] and walk.built > k
        walk(T)
        assert walk.info["active"]
    finally:
        _close(whole, win)
    # a map smaller than its window: the box holds all of it, the whole map serves
    tgt64 = tgt.astype(np.float64)
    small = tgt[np.hypot(tgt64[:, 0] - T[0, 3], tgt64[:, 1] - T[1, 3]) < 15.0]
    whole, win = _pair(small, src)
    try:
        walk = _Walk(whole, win, small)
        walk(T)
        assert walk.built >= 1 and not walk.info["active"] and walk.info["points"] == 0
    finally:
        _close(whole, win)
    # moves just inside the margin reuse the window, one just beyond it rebuilds it
    whole, win = _pair(tgt, src, margin=3.0)
    try:
        walk = _Walk(whole, win, tgt)
        walk(T, radii=(2.0,))
        k = walk.built
        for dx, dy, dz in ((2.99, 0, 0), (-2.99, 0, 0), (0, 2.99, 0), (0, -2.99, -2.99), (0, 0, 2.99)):
            walk(_at(T, dx=dx, dy=dy, dz=dz), radii=(2.0, 0.5))
            assert walk.built == k and walk.info["active"], (dx, dy, dz)
        walk(_at(T, dx=3.01), radii=(2.0,))
        assert walk.built == k + 1
        walk(_at(T, dx=3.01, dz=-6.03), radii=(2.0,))
        assert walk.built == k + 2
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- B: the search radius against the window's pad
@pytest.mark.timeout(600)
def test_window_radius():
    tgt, src, T = _scene()
    whole, win = _pair(tgt, src)
    try:
        assert _edge_queries(whole, tgt, src, T) >= 15
        walk = _Walk(whole, win, tgt)
        walk(T, radii=(0.5,))
        k = walk.built
        built = []
        for r in (0.3, 1.0, 2.0, 0.5):
            out = walk(T, radii=(r,))
            built.append(walk.built - k)
            if r == 2.0:
                ref = po.linearize(po.KdTree(tgt), src, T[:3, :3], T[:3, 3], po.default_lin_params(2.0, 0))
                assert_lin_equal(out, ref)
        assert built == [0, 1, 2, 2], built             # (0.3 needs no more than 0.5: the radius hint sets the pad)
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- C: the source changes at a fixed pose
@pytest.mark.timeout(600)
def test_window_source_changes():
    tgt, src, T = _scene()
    wide = h.map_frames(tgt, [T], n_frame=6_000, seed=3, frame_range=40.0)[0]
    near = h.map_frames(tgt, [T], n_frame=6_000, seed=4, frame_range=5.0)[0]
    whole, win = _pair(tgt, src)
    try:
        assert _edge_queries(whole, tgt, src, T) >= 15
        walk = _Walk(whole, win, tgt)
        walk(T)
        for s in (wide, near, src[:1], src[:64], src[:65], src):
            for c in (whole, win):
                c.set_source(s)
            walk(T)
        assert walk.info["active"]
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- D: a gated launch at a larger radius than the window was built for
@pytest.mark.timeout(600)
def test_gated_launch_at_a_larger_radius_than_the_window():
    tgt, src, T = _scene()
    whole, win = _pair(tgt, src)
    try:
        assert _edge_queries(whole, tgt, src, T) >= 15
        R, t = T[:3, :3], T[:3, 3]
        for r_gate in (2.0, 0.5):
            outs = []
            for c in (whole, win):
                c.linearize(R, t, _prm(0.5))                  # a window for radius 0.5 around T
                c.linearize_gated_begin(_prm(r_gate), slot=1)
                c.gate_open(R, t)
                outs.append(c.linearize_end(slot=1))
            assert _same_sums(outs[0], outs[1]), (r_gate, outs[0]["n_eff"], outs[1]["n_eff"])
            assert _same_sums(outs[0], whole.linearize(R, t, _prm(r_gate)))
        # the window is back for the next plain launch
        assert _same_sums(whole.linearize(R, t, _prm(2.0)), win.linearize(R, t, _prm(2.0))) and win.roi_info()["active"]
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- E: two plain launches in flight, the second leaves the window
@pytest.mark.timeout(600)
def test_two_plain_launches_in_flight():
    tgt, src, T = _scene()
    whole, win = _pair(tgt, src)
    try:
        T2 = _at(T, dx=40.0, yaw=0.2)
        outs = []
        for c in (whole, win):
            c.linearize(T[:3, :3], T[:3, 3], _prm(2.0))
            c.linearize_begin(T[:3, :3], T[:3, 3], _prm(2.0), slot=0)
            c.linearize_begin(T2[:3, :3], T2[:3, 3], _prm(2.0), slot=1)
            outs.append((c.linearize_end(slot=0), c.linearize_end(slot=1)))
        assert win.roi_info()["windows_built"] == 2
        assert _same_sums(outs[0][0], outs[1][0]) and _same_sums(outs[0][1], outs[1][1])
        assert outs[0][0]["n_eff"] > 0 and outs[0][1]["n_eff"] > 0
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- F: poses that are not poses are refused, and change nothing
def _bad_poses(T):
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    inf_t = t.copy(); inf_t[1] = np.inf
    nan_R = R.copy(); nan_R[1, 2] = np.nan
    return [(R, inf_t), (nan_R, t), (np.full((3, 3), np.nan), np.full(3, np.nan))]


@pytest.mark.timeout(600)
def test_non_finite_poses_are_refused():
    tgt, src, T = _scene()
    Rg, tg = T[:3, :3], T[:3, 3]
    cfg = api.default_config(search_radius=2.0, max_iterations=5, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, use_weight_derivative=0,
                             always_compute_schur=1)
    local = tgt[np.hypot(tgt[:, 0] - tg[0], tgt[:, 1] - tg[1]) < 30.0]
    whole, win = _pair(tgt, src)
    try:
        for c in (whole, win):
            c.set_option("record_launches", 1)
            c.reserve_warm_states(2)
        P = _prm(2.0)
        for c in (whole, win):
            c.linearize(Rg, tg, P)
            c.linearize(Rg, tg, P)
        assert win.roi_info()["active"] and not whole.roi_info()["active"]

        def as_T(R, t):
            M = np.eye(4); M[:3, :3] = R; M[:3, 3] = t
            return M

        entries = {
            "linearize": lambda c, R, t: c.linearize(R, t, P),
            "batch": lambda c, R, t: c.linearize_batch(np.stack([Rg, R]), np.stack([tg, t]), P),
            "batch_begin": lambda c, R, t: c.linearize_begin(R, t, P, slot=0),
            "batch_begin_warm": lambda c, R, t: c.linearize_batch_warm(np.stack([Rg, R]), np.stack([tg, t]), [0, 1], P),
            "debug": lambda c, R, t: c.linearize(R, t, P, debug=True),
            "stamped": lambda c, R, t: c.linearize_stamped(R, t, P),
            "frames": lambda c, R, t: c.register_frames([src, src], [T, as_T(R, t)], "Ours", cfg),
            "pairs": lambda c, R, t: c.register_pairs([src], [local], [as_T(R, t)], "Ours", cfg),
            "icp_run": lambda c, R, t: c.icp_run(as_T(R, t), "Ours", cfg),
            "trials": lambda c, R, t: c.icp_run_trials([T, as_T(R, t)], "Ours", cfg),
        }
        for c in (win, whole):
            before = c.roi_info()
            c.launch_series(reset=True)
            for name, fn in entries.items():
                for k, (R, t) in enumerate(_bad_poses(T)):
                    with pytest.raises(api.DcregError) as e:
                        fn(c, R, t)
                    assert "failed (-1)" in str(e.value), (name, k, str(e.value))
                    assert c.roi_info() == before, (name, k)
            # a refused gate keeps waiting: opened afterwards with a finite pose it gives the plain launch's sums
            c.linearize_gated_begin(P, slot=1)
            for k, (R, t) in enumerate(_bad_poses(T)):
                with pytest.raises(api.DcregError) as e:
                    c.gate_open(R, t)
                assert "failed (-1)" in str(e.value), (k, str(e.value))
            c.gate_open(Rg, tg)
            gated = c.linearize_end(slot=1)
            assert c.roi_info() == before
            searched = c.launch_series(reset=True)["searched"]
            assert len(searched) == 1                   # nothing but the gated launch ran ...
            assert searched[0] < len(src)               # ... at the pose of the last two, from the neighbour state they left
            assert _same_sums(gated, whole.linearize(Rg, tg, P))
        # the pose of the stale mixed box (t = (x + 10, inf, z)), then a finite pose 10 m along x: the window follows it
        R, t = Rg.copy(), tg + np.array([10.0, 0.0, 0.0])
        t_bad = t.copy(); t_bad[1] = np.inf
        with pytest.raises(api.DcregError):
            win.linearize(R, t_bad, P)
        assert _same_sums(whole.linearize(R, t, P), win.linearize(R, t, P))
        assert win.roi_info()["active"] and win.roi_info()["box_min"][0] > tg[0] - 16.0         # (a box around the new pose)
    finally:
        _close(whole, win)


@pytest.mark.timeout(600)
def test_refused_launches_change_nothing():
    """A launch refused for its parameters or its warm-state ids (DCREG_E_INVALID) leaves the context as it was: window box, rebuild
    count and active index, the neighbour states and their keys.  Refused at a pose 10 m off the window, the next launch at the old pose
    searches from the state the earlier launches left and gives the whole map's sums; a batch at the old pose after a refused batch at
    another radius finds its warm states as they were."""
    tgt, src, T = _scene()
    Rg, tg = T[:3, :3], T[:3, 3]
    Rf, tf = Rg, tg + np.array([10.0, 0.0, 0.0])
    whole, win = _pair(tgt, src)
    try:
        P = _prm(2.0)
        for c in (whole, win):
            c.set_option("record_launches", 1)
            c.reserve_warm_states(2)
        for _ in range(2):
            win.linearize(Rg, tg, P)
            kept = whole.linearize_batch_warm(np.stack([Rg, Rg]), np.stack([tg, tg]), [0, 1], P)
        assert win.roi_info()["active"]
        ref = whole.linearize(Rg, tg, P)

        def prm(**kw):
            q = _prm(2.0)
            for k, v in kw.items():
                setattr(q, k, v)
            return q

        two = (np.stack([Rf, Rf]), np.stack([tf, tf]))
        refusals = {
            "radius 0": lambda c: c.linearize(Rf, tf, prm(search_radius=0.0)),
            "radius nan": lambda c: c.linearize(Rf, tf, prm(search_radius=np.nan)),
            "k 3": lambda c: c.linearize(Rf, tf, prm(k=3)),
            "parameterization 7": lambda c: c.linearize(Rf, tf, prm(parameterization=7)),
            "unreserved state": lambda c: c.linearize_batch_warm(*two, [0, 2], P),
            "duplicate state": lambda c: c.linearize_batch_warm(*two, [1, 1], P),
        }
        win.launch_series(reset=True)
        for name, fn in refusals.items():
            before = win.roi_info()
            with pytest.raises(api.DcregError) as e:
                fn(win)
            assert "failed (-1)" in str(e.value), (name, str(e.value))
            assert win.roi_info() == before, name
            out = win.linearize(Rg, tg, P)
            searched = win.launch_series(reset=True)["searched"]
            assert len(searched) == 1 and searched[0] < len(src), (name, searched)
            assert _same_sums(out, ref), name
        # the batch states: a duplicate id at another search radius (another state key) is refused before the key is taken
        whole.launch_series(reset=True)
        with pytest.raises(api.DcregError):
            whole.linearize_batch_warm(*two, [1, 1], _prm(3.0))
        outs = whole.linearize_batch_warm(np.stack([Rg, Rg]), np.stack([tg, tg]), [0, 1], P)
        searched = whole.launch_series(reset=True)["searched"]
        assert len(searched) == 1 and searched[0] < 2 * len(src), searched
        assert all(_same_sums(o, k) for o, k in zip(outs, kept))
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- G: kernel options on the window
@pytest.mark.timeout(600)
@pytest.mark.parametrize("opts", [{"team_pass": 0}, {"team_pass": 2}, {"advance": 2}, {"one_wave": 2}, {"use_certificates": 0},
                                  {"fast_plane_fit": 0}, {"fast_plane_fit": 1}], ids=lambda o: "%s=%s" % next(iter(o.items())))
def test_kernel_options_on_the_window(opts):
    tgt, src, T = _scene()
    whole, win = _pair(tgt, src, opts=opts)
    try:
        walk = _Walk(whole, win, tgt)
        for M in (T, _at(T, dx=0.03, dy=-0.02, yaw=0.002), _at(T, dx=0.3, dy=0.2, yaw=0.02), _at(T, dx=12.0, dy=-4.0, yaw=0.3)):
            walk(M)
        assert walk.built >= 2
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- I: map updates while the window is active
@pytest.mark.timeout(600)
def test_map_updates_under_an_active_window():
    tgt, src, T = _scene()
    R, t = T[:3, :3], T[:3, 3]
    whole, win = _pair(tgt, src)

    def fresh_sums(c):
        f = api.Context(0)
        try:
            f.set_target(c.target_points(), HINT)
            f.set_source(src)
            return [f.linearize(R, t, _prm(r)) for r in (0.5, 2.0)]
        finally:
            f.close()

    try:
        walk = _Walk(whole, win, tgt)
        walk(T)
        assert walk.info["active"]
        lo, hi = tgt.min(0).astype(np.float64) - 1.0, tgt.max(0).astype(np.float64) + 1.0
        hi[0] = t[0] + 6.0                                   # a slab boundary through the window
        Tfar = _at(T, dx=-150.0, dy=80.0, yaw=1.0)
        for step in ("crop", "insert"):
            for c in (whole, win):
                u = c.crop(lo, hi) if step == "crop" else c.insert(src, Tfar)
                assert (u["n_removed"] if step == "crop" else u["n_added"]) > 0
            want = fresh_sums(win)
            walk.tgt64 = win.target_points().astype(np.float64)
            for r, w in zip((0.5, 2.0), want):
                got = win.linearize(R, t, _prm(r))
                assert _same_sums(got, w) and _same_sums(whole.linearize(R, t, _prm(r)), w), (step, r)
                _check_window(win, walk.tgt64, walk.cell)
            assert win.roi_info()["active"]
    finally:
        _close(whole, win)


# ---------------------------------------------------------------- K: a drive, the window engaged by the table budget
@pytest.mark.timeout(900)
def test_a_drive_on_the_window_engaged_by_the_budget():
    tgt, _, T = _scene()
    poses = [_at(T, dx=3.0 * k, dy=0.4 * k, yaw=0.004 * k) for k in range(24)]
    frames = h.map_frames(tgt, poses, n_frame=3_000, seed=9, frame_range=20.0)
    dT = h.pose6d_matrix(0.12, -0.08, 0.03, 0.002, -0.001, 0.006)
    capped, free = api.Context(0), api.Context(0)
    try:
        capped.set_option("max_table_entries", 1 << 20)          # (the cell edge grows to three times what the radius hint asks for)
        for c in (capped, free):
            c.set_target(tgt, HINT)
        assert capped.roi_info()["whole_map_capped"] and not free.roi_info()["whole_map_capped"]
        for k, (P, F) in enumerate(zip(poses, frames)):
            cfg, ocfg = cfg_pair(2.0, 30, 0, 1e-5, 1e-3, P.reshape(16))
            recs = []
            for c in (capped, free):
                c.set_source(F)
                res, logs = c.icp_run(P @ dT, "Ours", cfg)
                recs.append((tuple(res.R[:]), tuple(res.t[:]), res.iterations, res.converged, res.status,
                             [(tuple(L.H_upper[:]), tuple(L.gradient[:]), L.effective_points, L.corr_pt_count, tuple(L.update_dx[:])) for L in logs]))
            assert recs[0] == recs[1], k
            assert recs[0][4] == 0 and recs[0][2] >= 2, (k, recs[0][2:5])
        info = capped.roi_info()
        assert info["active"] and info["windows_built"] >= 3 and free.roi_info()["windows_built"] == 0
        ores, ologs = po.icp_run(po.KdTree(tgt), frames[-1], poses[-1] @ dT, "Ours", ocfg)
        assert_runs_equal(res, logs, ores, ologs)
    finally:
        _close(capped, free)
