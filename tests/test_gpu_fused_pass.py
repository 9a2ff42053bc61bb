"""GPU tests of the advance pass that carries its launch out alone (kernels.hpp k_advance ROWS; option "advance_fused", run with -m gpu
on an MI355X; everything through the C-ABI): one kernel tests the certificates, works the tile's list off in dense waves and builds the
rows of the tile's query blocks itself.  Its 31 sums are bitwise those of the pass with the linearisation kernel behind it and of the
linearisation kernel alone - on walks, in whole engine runs behind the gate, and whatever the state's history."""
import numpy as np
import pytest

import helpers as h
import p2plane_rows
from dcreg_amd import api

pytestmark = pytest.mark.gpu

TILE = 1536          # points per block of the advance pass (kernels.hpp kAdvTile)


def _same_sums(a, b):
    return (a["n_eff"] == b["n_eff"] and a["n_pt"] == b["n_pt"] and np.array_equal(a["H_upper"], b["H_upper"]) and np.array_equal(a["g"], b["g"])
            and a["sum_r2"] == b["sum_r2"] and a["sum_b2"] == b["sum_b2"])


def _scene(scene, n_src):
    """A target of a few ten thousand points and exactly n_src source points on it."""
    rng = np.random.default_rng(77)
    if scene == "cylinder":
        tgt, radius = h.scene_cylinder(40_000, seed=8, noise=0.01), 1.0
        src = (tgt[::2][:n_src] + rng.normal(0, 0.004, (n_src, 3))).astype(np.float32)
    else:
        # the lattice with duplicates of test_gpu_round5._scene, larger: every query has exact distance ties (certificates without
        # slack), and a shell of queries around it comes and goes through the gate radius (OUT points)
        g = np.arange(0, 30, dtype=np.float32) * 0.3
        tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        tgt, radius = np.concatenate([tgt, tgt[::7]]), 0.7
        src = (tgt[(np.arange(n_src) * 5) % len(tgt)] + np.float32(0.11)).astype(np.float32)
        far = np.arange(0, n_src, 41)
        src[far, 0] = np.float32(8.7) + rng.uniform(0.3, 0.9, len(far)).astype(np.float32)
    assert len(src) == n_src
    return tgt, src, radius


def _ctx(tgt, src, radius, fast, **opts):
    c = api.Context(0)
    c.set_option("fast_plane_fit", fast)
    c.set_option("team_pass", 0)
    for k, v in opts.items():
        c.set_option(k, v)
    c.set_option("record_launches", 1)
    c.set_target(tgt, radius); c.set_source(src)
    return c


STEPS = [0.0, 1e-6, 1e-4, 3e-4, 1e-3, -1e-3, 2e-3, 1e-5, 4e-3, 6e-3, -6e-3, 1e-2, 1e-4, 3e-2, 0.2, 1e-3, 5.0, -5.0, 5e-4, 0.0]


# 16897: 67 query blocks, the last one of ONE point; 12 tiles, the 11th across chunks 0 / 1; chunk 1 of three blocks; a ragged last tile,
# block and wave.  18432: exactly 12 full tiles.  (Both above 64 query blocks: not direct launches.)
@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("n_src", [16897, 18432])
@pytest.mark.parametrize("scene", ["cylinder", "lattice_dups"])
def test_fused_pass_walk_matches_the_two_kernel_and_plain_forms(scene, n_src, fast):
    """A pose walk that mixes micrometre steps, centimetre steps and a jump, through three contexts: the pass forced and fused (one
    kernel), forced in its two-kernel form, and off.  The 31 sums agree bit for bit at every step; at the last pose they also agree
    with a context that searches every point (certificates off).  The launch log says the fused kernel ran; the searched counts say
    that tiles occurred with more than 64 listed points and with none."""
    tgt, src, radius = _scene(scene, n_src)
    prm = api.default_lin_params(radius, 1)
    ctxs = {"fused": _ctx(tgt, src, radius, fast, advance=2, advance_fused=1), "two": _ctx(tgt, src, radius, fast, advance=2, advance_fused=0),
            "plain": _ctx(tgt, src, radius, fast, advance=0)}
    n_tiles = -(-n_src // TILE)
    T = np.eye(4)
    listed = []
    for k, sz in enumerate(STEPS):
        T = h.pose6d_matrix(sz * 0.6, -sz * 0.3, sz * 0.2, sz * 0.002, -sz * 0.001, sz * 0.004) @ T
        outs = {name: c.linearize(T[:3, :3], T[:3, 3], prm) for name, c in ctxs.items()}
        assert _same_sums(outs["fused"], outs["plain"]), (scene, n_src, fast, k)
        assert _same_sums(outs["two"], outs["plain"]), (scene, n_src, fast, k)
        ser = {name: c.launch_series(reset=True) for name, c in ctxs.items()}
        assert all(len(s["ms"]) == 1 for s in ser.values())
        # which kernels ran: the first launch fills the state (no pass), every later one takes the pass
        assert ser["fused"]["structure"][0] == (2 if k > 0 else 0) and ser["fused"]["advanced"][0] == (1 if k > 0 else 0), k
        assert ser["two"]["structure"][0] == (1 if k > 0 else 0) and ser["plain"]["structure"][0] == 0, k
        if k > 0:
            listed.append((int(ser["fused"]["searched"][0]), int(ser["fused"]["refitted"][0])))
    print(scene, n_src, fast, "listed (searched, refitted) per step:", listed)
    # more than 64 searches per tile on average: some tile listed more than 64 (several dense chunks per wave); the 5 m jumps leave no
    # certificate standing: every point listed, and counted once (the fused kernel never searches a point a second time)
    assert max(s for s, _ in listed) == n_src > 64 * n_tiles
    # a launch with fewer listed points than tiles has a tile with an empty list (the noisy cloud has no distance ties to speak of:
    # at the repeated pose that closes the walk every certificate stands; every query of the lattice has ties - no such launch there)
    if scene == "cylinder":
        assert min(s + r for s, r in listed) < n_tiles
    allc = _ctx(tgt, src, radius, fast, use_certificates=0, advance=0)
    assert _same_sums(allc.linearize(T[:3, :3], T[:3, 3], prm), outs["fused"])
    allc.close()
    for c in ctxs.values():
        c.close()


def _engine_pair():
    tgt = h.scene_corridor(20_480, seed=9, length=40.0)
    src = (tgt + np.random.default_rng(10).normal(0, 0.01, tgt.shape)).astype(np.float32)
    return tgt, src


ENGINE_FORMS = (("fused", {"advance": 1, "advance_min_blocks": 1, "advance_fused": 1}), ("two", {"advance": 1, "advance_min_blocks": 1, "advance_fused": 0}),
                ("off", {"advance": 0}))


def test_fused_pass_in_whole_runs_behind_the_gate():
    """Engine level: two back-to-back 30-iteration runs of a 20 k-point corridor pair (the pipelined engine queues every launch behind a
    gate), the pass chosen by the host's rule ("advance_min_blocks" = 1) in its fused and its two-kernel form, and off: every
    iteration's H, g, counts and pose are bitwise the same; the rule picked the pass for some launches and not for others, and where
    it did the fused context ran one kernel."""
    tgt, src = _engine_pair()
    T0 = h.pose6d_matrix(0.05, -0.08, 0.03, h.deg2rad(0.2), h.deg2rad(-0.1), h.deg2rad(0.5))
    cfg = api.default_config(search_radius=1.0, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=0.0,
                             CONVERGENCE_THRESH_TRANS=0.0, use_weight_derivative=1, always_compute_schur=1)
    logs, ser = {}, {}
    for name, opts in ENGINE_FORMS:
        c = _ctx(tgt, src, 1.0, 1, **opts)
        runs = []
        for rep in range(2):                       # the second run starts from the first one's converged state
            res, lg = c.icp_run(T0, "Ours", cfg)
            runs.append([(np.array(L.H_upper[:]), np.array(L.gradient[:]), L.effective_points, L.corr_pt_count, np.array(L.transform_matrix[:])) for L in lg[:res.iterations]])
        logs[name] = runs
        ser[name] = c.launch_series(reset=True)
        c.close()
    for name in ("fused", "two"):
        for rep in range(2):
            assert len(logs[name][rep]) == len(logs["off"][rep]) == 30
            for it, (x, y) in enumerate(zip(logs[name][rep], logs["off"][rep])):
                assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3] and np.array_equal(x[4], y[4]), (name, rep, it)
    print("passes picked by the rule:", "".join("A" if a else "." for a in ser["fused"]["advanced"]))
    assert ser["off"]["advanced"].sum() == 0 and ser["off"]["structure"].sum() == 0
    assert 0 < ser["fused"]["advanced"].sum() < len(ser["fused"]["advanced"])
    assert np.array_equal(ser["fused"]["structure"], 2 * ser["fused"]["advanced"])
    assert np.array_equal(ser["two"]["structure"], ser["two"]["advanced"]) and np.array_equal(ser["two"]["advanced"], ser["fused"]["advanced"])


def test_fused_pass_in_a_run_of_the_euler_engine():
    """The second engine (roll / pitch / yaw row): a run with the pass in front of every launch that can take it, fused and in two
    kernels, and off - the same H, g, counts and pose at every iteration, bit for bit; the fused kernel ran."""
    tgt, src = _engine_pair()
    cfg = api.default_config(search_radius=1.0, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=0.0,
                             CONVERGENCE_THRESH_TRANS=0.0, use_weight_derivative=1, always_compute_schur=1)
    p0 = (h.deg2rad(0.2), h.deg2rad(-0.1), h.deg2rad(0.5), 0.05, -0.08, 0.03)
    logs, ser = {}, {}
    for name, opts in (("fused", {"advance": 2, "advance_fused": 1}), ("two", {"advance": 2, "advance_fused": 0}), ("off", {"advance": 0})):
        c = _ctx(tgt, src, 1.0, 1, **opts)
        res, lg, pose = c.icp_run_euler(p0, "ME-SR", cfg)
        logs[name] = [(np.array(L.H_upper[:]), np.array(L.gradient[:]), L.effective_points, L.corr_pt_count, np.array(L.transform_matrix[:])) for L in lg[:res.iterations]] + [pose]
        ser[name] = c.launch_series(reset=True)
        c.close()
    for name in ("fused", "two"):
        assert len(logs[name]) == len(logs["off"]) > 2
        for it, (x, y) in enumerate(zip(logs[name][:-1], logs["off"][:-1])):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3] and np.array_equal(x[4], y[4]), (name, it)
        assert np.array_equal(logs[name][-1], logs["off"][-1])
    print("euler run, searched per launch:", list(ser["fused"]["searched"]))
    assert (ser["fused"]["structure"] == 2).sum() == len(ser["fused"]["structure"]) - 1 and (ser["two"]["structure"] == 2).sum() == 0


@pytest.mark.parametrize("scene", ["cylinder", "lattice_dups"])
def test_fused_pass_does_not_depend_on_the_states_history(scene):
    """The fused launch at one pose from two different state histories (a context that came in micrometre steps, one that came by a
    jump, and the first one again): bitwise the same sums, and those of a context that never ran the pass."""
    tgt, src, radius = _scene(scene, 16897)
    prm = api.default_lin_params(radius, 1)
    Tend = h.pose6d_matrix(0.012, -0.006, 0.004, 4e-5, -2e-5, 8e-5)
    histories = ([np.eye(4), h.pose6d_matrix(0.0118, -0.006, 0.004, 4e-5, -2e-5, 8e-5)],
                 [h.pose6d_matrix(0.3, 0.2, -0.1, 0.01, 0.0, -0.02)])
    outs = []
    for hist, adv in ((histories[0], 2), (histories[1], 2), (histories[0] + histories[1], 0)):
        c = _ctx(tgt, src, radius, 1, advance=adv, advance_fused=1)
        for T in hist:
            c.linearize(T[:3, :3], T[:3, 3], prm)
        c.launch_series(reset=True)
        outs.append(c.linearize(Tend[:3, :3], Tend[:3, 3], prm))
        again = c.linearize(Tend[:3, :3], Tend[:3, 3], prm)            # (and once more at the very same pose)
        assert _same_sums(again, outs[-1])
        assert list(c.launch_series(reset=True)["structure"]) == ([2, 2] if adv else [0, 0])
        c.close()
    assert _same_sums(outs[0], outs[1]) and _same_sums(outs[0], outs[2])


@pytest.mark.parametrize("scene", ["cylinder", "lattice_dups"])
def test_the_sums_past_one_chunk_are_within_the_derived_bound_of_their_own_rows(scene):
    """The last pose of the walk above at 16 897 points (67 query blocks: chunk sums, a second chunk of three block rows), in a plain
    context of the parity instantiation: every one of the 31 sums against the exact sum over the rows rebuilt from the device's own dump
    (tests/p2plane_rows.py, tests/sums_check.py)."""
    tgt, src, radius = _scene(scene, 16897)
    T = np.eye(4)
    for sz in STEPS:
        T = h.pose6d_matrix(sz * 0.6, -sz * 0.3, sz * 0.2, sz * 0.002, -sz * 0.001, sz * 0.004) @ T
    c = _ctx(tgt, src, radius, 0, advance=0)
    try:
        got, worst = p2plane_rows.assert_dump_sums_entrywise(c, src, T, api.default_lin_params(radius, 1), scene)
        print("%s: n_eff %d of %d, the largest error is %.3g of its bound" % (scene, got["n_eff"], len(src), worst))
        assert got["n_eff"] > 0.9 * len(src)                          # nine points in ten effective: every chunk holds such rows
    finally:
        c.close()
