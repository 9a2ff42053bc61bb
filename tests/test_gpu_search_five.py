"""GPU tests of the five-neighbour launches (kernels.hpp k_lin FIVE, search.hpp lin_search5; option "search_five", run with -m gpu on an
MI355X; everything through the C-ABI): a launch whose searches keep the five nearest and nothing for the next launch - no sixth
neighbour, no certificate, no stored plane.  Scheduling only: its 31 sums are bitwise those of the six-neighbour launch - on walks, when
the mode changes on one context, on a lattice where every query has distance ties, and in whole pipelined runs."""
import numpy as np
import pytest

import helpers as h
from dcreg_amd import api
from oracle import pyoracle as po
from test_gpu_fused_pass import _scene, _same_sums, _engine_pair

pytestmark = pytest.mark.gpu


def _ctx(tgt, src, radius, fast, **opts):
    c = api.Context(0)
    c.set_option("fast_plane_fit", fast)
    for k, v in opts.items():
        c.set_option(k, v)
    c.set_option("record_launches", 1)
    c.set_target(tgt, radius); c.set_source(src)
    return c


# aligned, millimetres, centimetres, 0.8 m jumps and back to steps below a millimetre (and a repeated pose)
STEPS = [0.0, 1e-3, 2e-2, 0.8, -0.8, 5e-2, 8e-3, 1e-3, 3e-4, 1e-4, 0.0, 0.8, 4e-4, 1e-6, 0.0]


@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("scene,n_src", [("cylinder", 16897), ("lattice_dups", 18432)])
def test_walk_sums_do_not_depend_on_the_mode(scene, n_src, fast):
    """A pose walk through four contexts: five-neighbour launches never (0), by the rule with nothing announced (1: plain calls are no
    trajectory - none runs), by the rule with every launch announced as the start of a run (the jumps and the fresh state take them),
    and wherever possible (2).  The 31 sums agree bit for bit at every step.  On the lattice every query has exact distance ties: the
    canonical five (smallest original index among equal distances) are what the sums of mode 0 are made of."""
    tgt, src, radius = _scene(scene, n_src)
    prm = api.default_lin_params(radius, 1)
    ctxs = {"0": _ctx(tgt, src, radius, fast, search_five=0), "1": _ctx(tgt, src, radius, fast, search_five=1),
            "1a": _ctx(tgt, src, radius, fast, search_five=1), "2": _ctx(tgt, src, radius, fast, search_five=2)}
    T = np.eye(4)
    five = {name: [] for name in ctxs}
    for k, sz in enumerate(STEPS):
        T = h.pose6d_matrix(sz * 0.6, -sz * 0.3, sz * 0.2, sz * 0.002, -sz * 0.001, sz * 0.004) @ T
        ctxs["1a"].hint_misalignment(-1.0)
        outs = {name: c.linearize(T[:3, :3], T[:3, 3], prm) for name, c in ctxs.items()}
        for name in ("1", "1a", "2"):
            assert _same_sums(outs[name], outs["0"]), (scene, fast, k, name)
        for name, c in ctxs.items():
            ser = c.launch_series(reset=True)
            assert len(ser["five"]) == 1
            five[name].append(int(ser["five"][0]))
    print(scene, fast, "five-neighbour launches:", five)
    assert sum(five["0"]) == 0 and sum(five["1"]) == 0 and sum(five["2"]) == len(STEPS)
    # announced: the fresh state and the launches behind the 0.8 m jumps - and nothing at the small steps
    assert five["1a"][0] == 1 and five["1a"][3] == 1 and five["1a"][4] == 1 and five["1a"][11] == 1
    assert five["1a"][8] == 0 and five["1a"][9] == 0 and five["1a"][10] == 0 and five["1a"][13] == 0
    for c in ctxs.values():
        c.close()


def test_counts_on_the_fixture_pair_are_the_oracles():
    pts = h.cylinder_cloud()
    tree = po.KdTree(pts)
    c = _ctx(pts, pts, 1.0, 1, search_five=2)
    for T in (h.pose6d_matrix(**h.PAPER_INIT), h.pose6d_matrix(0.004, -0.002, 0.001, 1e-4, 0.0, -2e-4) @ h.pose6d_matrix(**h.PAPER_INIT), np.eye(4)):
        gpu = c.linearize(T[:3, :3], T[:3, 3], api.default_lin_params(1.0, 1))
        ref = po.linearize(tree, pts, T[:3, :3], T[:3, 3], po.default_lin_params(1.0, 1))
        assert gpu["n_eff"] == ref["n_eff"] and gpu["n_pt"] == ref["n_pt"], (gpu["n_eff"], ref["n_eff"], gpu["n_pt"], ref["n_pt"])
    assert c.launch_series(reset=True)["five"].sum() == 3
    c.close()


@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("scene", ["cylinder", "lattice_dups"])
@pytest.mark.parametrize("modes", [(0, 2, 2, 0, 0), (2, 0, 2)])
def test_mode_changes_on_one_context(scene, modes, fast):
    """The launch sequences 6 -> 5 -> 5 -> 6 -> 6 and 5 -> 6 -> 5 on one context, millimetre steps between them (certificates hold for
    some points and fail for others): every launch's sums are bitwise those of a freshly built context at that pose."""
    tgt, src, radius = _scene(scene, 16897)
    prm = api.default_lin_params(radius, 1)
    c = _ctx(tgt, src, radius, fast)
    T = h.pose6d_matrix(0.01, -0.02, 0.005, 1e-4, 0.0, -2e-4)
    for k, m in enumerate(modes):
        T = h.pose6d_matrix(6e-4, -3e-4, 2e-4, 2e-6, -1e-6, 4e-6) @ T
        c.set_option("search_five", m)
        out = c.linearize(T[:3, :3], T[:3, 3], prm)
        assert int(c.launch_series(reset=True)["five"][0]) == (1 if m == 2 else 0)
        f = _ctx(tgt, src, radius, fast, search_five=0)
        assert _same_sums(out, f.linearize(T[:3, :3], T[:3, 3], prm)), (scene, modes, fast, k)
        f.close()
    c.close()


@pytest.mark.parametrize("scene", ["cylinder", "lattice_dups"])
def test_certificates_after_the_return_to_six_neighbour_launches(scene):
    """A five-neighbour launch leaves certificates of radius zero: the next launch - at the very same pose - searches every point (the
    count slots say so) and, being a six-neighbour launch, leaves certificates that serve the launch after it.  The sums are the same
    with certificates in use and without."""
    tgt, src, radius = _scene(scene, 16897)
    n = len(src)
    prm = api.default_lin_params(radius, 1)
    T = h.pose6d_matrix(0.01, -0.02, 0.005, 1e-4, 0.0, -2e-4)
    c = _ctx(tgt, src, radius, 1, search_five=2)
    nocert = _ctx(tgt, src, radius, 1, search_five=0, use_certificates=0)
    ref = nocert.linearize(T[:3, :3], T[:3, 3], prm)
    a = c.linearize(T[:3, :3], T[:3, 3], prm)
    b = c.linearize(T[:3, :3], T[:3, 3], prm)                  # five again: nothing to test, everything searched
    c.set_option("search_five", 0)
    d = c.linearize(T[:3, :3], T[:3, 3], prm)                  # six, at the very same pose
    e = c.linearize(T[:3, :3], T[:3, 3], prm)                  # ... and its certificates serve this one
    ser = c.launch_series(reset=True)
    assert list(ser["five"]) == [1, 1, 0, 0]
    assert list(ser["searched"][:3]) == [n, n, n]
    if scene == "cylinder":                                    # (no distance ties to speak of: every certificate has slack)
        assert ser["searched"][3] < 0.01 * n
    for out in (a, b, d, e):
        assert _same_sums(out, ref)
    c.close(); nocert.close()


def _run_record(c, T0, cfg):
    res, lg = c.icp_run(T0, "Ours", cfg)
    its = [(np.array(L.H_upper[:]), np.array(L.gradient[:]), L.effective_points, L.corr_pt_count, np.array(L.transform_matrix[:])) for L in lg[:res.iterations]]
    return (res.converged, res.iterations, res.status, np.array(res.R[:]), np.array(res.t[:]), np.array(res.icp_cov[:])), its


def test_whole_pipelined_runs_do_not_depend_on_the_rule():
    """Engine level, a 20 k-point corridor pair: a run of fixed length and two runs to convergence (the engine leaves its loop with a
    launch queued ahead, which it calls off; the second starts from the state the first left), with the option at 0 and at 1: pose,
    covariance, iterations, status and every iteration's H, g and counts are bitwise equal.  At 1 the rule takes five-neighbour launches
    at the start of a run and none once the pose has settled."""
    tgt, src = _engine_pair()
    T0 = h.pose6d_matrix(0.05, -0.08, 0.03, h.deg2rad(0.2), h.deg2rad(-0.1), h.deg2rad(0.5))
    fixed = api.default_config(search_radius=1.0, max_iterations=20, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=0.0,
                               CONVERGENCE_THRESH_TRANS=0.0, use_weight_derivative=1, always_compute_schur=1)
    conv = api.default_config(search_radius=1.0, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, use_weight_derivative=1,
                              always_compute_schur=1)
    rec, ser = {}, {}
    for mode in (0, 1):
        c = _ctx(tgt, src, 1.0, 1, search_five=mode)
        rec[mode] = [_run_record(c, T0, fixed)]
        ser[mode] = [c.launch_series(reset=True)]
        for _ in range(2):
            rec[mode].append(_run_record(c, T0, conv))
            ser[mode].append(c.launch_series(reset=True))
        c.close()
    for r, (x, y) in enumerate(zip(rec[0], rec[1])):
        assert x[0][:3] == y[0][:3], (r, x[0][:3], y[0][:3])
        for u, v in zip(x[0][3:], y[0][3:]):
            assert np.array_equal(u, v), r
        assert len(x[1]) == len(y[1])
        for it, (p, q) in enumerate(zip(x[1], y[1])):
            assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[2] == q[2] and p[3] == q[3] and np.array_equal(p[4], q[4]), (r, it)
    assert rec[1][1][0][0] == 1 and rec[1][1][0][1] < 30          # (the runs to convergence did converge before the cap)
    for r in range(3):
        f = list(ser[1][r]["five"])
        print("run", r, "five-neighbour launches:", "".join("5" if x else "." for x in f), "searched permille (mode 0):",
              [int(round(1e3 * a / b)) for a, b in zip(ser[0][r]["searched"], ser[0][r]["points"])])
        assert sum(ser[0][r]["five"]) == 0
        n_five = sum(f)
        assert all(f[:n_five]) and n_five < len(f)                  # one series, at the start of the run, and it ends
        if r == 0:                                                  # (a fresh context; the later runs start within half a cell of a settled pose)
            assert f[0] == 1 and f[1] == 1 and sum(f[10:]) == 0     # ... none once the pose has settled
