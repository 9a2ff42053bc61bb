"""The gates of one linearisation at their thresholds on the GPU (tests/gate_scenes.py builds the scenes; run with -m gpu on an MI355X):
  * cold launches with the parity fit (fast_plane_fit = 0) are bitwise the oracle's, point by point, at every case;
  * cold launches with the fast fit give the oracle's flags at every case whose exact margin is at least FAST_FIT_BAND (dcreg.h);
  * walks that carry queries back and forth across the weight and radius thresholds, under every option that changes how a launch
    is carried out, are bitwise a fresh context's cold launch at every step, with either fit;
  * parameters the states do not key on (weight_slope, weight_min, use_weight_derivative) and those they do (min_normal_norm,
    max_plane_thickness_sq), alternated on one context, give bitwise a fresh context's result;
  * the Euler row of the second engine with the parity fit: flags bitwise, sums within the tolerance of its existing tests."""
import numpy as np
import pytest

import gate_scenes as gs
import helpers as h
from dcreg_amd import api
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

FAST_FIT_BAND = 1e-11      # dcreg.h "fast_plane_fit": the fast fit's flags differ from the oracle's only this close to a threshold


@pytest.fixture(scope="module")
def scenes():
    return gs.all_scenes()


def _lin_params(prm, euler_rpy=None):
    p = api.default_lin_params(prm["search_radius"], prm["use_weight_derivative"], euler_rpy=euler_rpy)
    p.max_plane_thickness_sq = prm["max_plane_thickness_sq"]; p.min_normal_norm = prm["min_normal_norm"]
    p.weight_slope = prm["weight_slope"]; p.weight_min = prm["weight_min"]
    return p


def _ctx(sc, fast, **opts):
    c = api.Context(0)
    c.set_option("fast_plane_fit", fast)
    for k, v in opts.items():
        c.set_option(k, v)
    c.set_target(sc.target, sc.prm["search_radius"]); c.set_source(sc.source)
    return c


def _cold(sc, fast, R, t, prm=None, debug=False):
    c = _ctx(sc, fast)
    out = c.linearize(R, t, _lin_params(prm or sc.prm), debug=debug)
    c.close()
    return out


def _same_sums(a, b):
    return (a["n_eff"] == b["n_eff"] and a["n_pt"] == b["n_pt"] and np.array_equal(a["H_upper"], b["H_upper"]) and np.array_equal(a["g"], b["g"])
            and a["sum_r2"] == b["sum_r2"] and a["sum_b2"] == b["sum_b2"])


def _oracle(sc, R=np.eye(3), t=np.zeros(3), euler_rpy=None):
    return po.linearize(po.KdTree(sc.target), sc.source, R, t, gs.oracle_params(sc.prm, euler_rpy), debug=True)


def test_parity_fit_cold_launch_is_bitwise_the_oracles(scenes):
    for sc in scenes:
        ref = _oracle(sc)
        g = _cold(sc, 0, np.eye(3), np.zeros(3), debug=True)
        bad = np.flatnonzero(g["flag"] != ref["flag"])
        assert bad.size == 0, (sc.name, [(sc.patches[i][3], sc.patches[i][4], int(g["flag"][i]), int(ref["flag"][i])) for i in bad])
        got = ref["flag"] != 0
        assert np.array_equal(g["nn_idx"][got], ref["nn_idx"][got]), sc.name
        assert np.array_equal(g["nn_d2"][got].view(np.uint32), ref["nn_d2"][got].view(np.uint32)), sc.name
        for k in ("normal", "r", "s"):
            assert np.array_equal(g[k], ref[k]), (sc.name, k)
        assert g["n_eff"] == ref["n_eff"] and g["n_pt"] == ref["n_pt"], sc.name
        assert np.abs(g["H_upper"] - ref["H_upper"]).max() <= 1e-12 * np.abs(ref["H_upper"]).max(), sc.name
        assert np.abs(g["g"] - ref["g"]).max() <= 1e-12 * max(np.abs(ref["g"]).max(), 1e-300), sc.name


def test_fast_fit_flags_outside_its_band(scenes):
    """The fast fit's flags equal the oracle's at every case whose exact margin is at least FAST_FIT_BAND; the disagreements inside
    the band are counted per gate, with the largest margin at which each gate flipped (printed with -s)."""
    inside, worst, outside = {}, {}, []
    total = 0
    for sc in scenes:
        ref = _oracle(sc)
        g = _cold(sc, 1, np.eye(3), np.zeros(3), debug=True)
        for i in np.flatnonzero(g["flag"] != ref["flag"]):
            Q, q, gate, label, m, step = sc.patches[i]
            mg = abs(float(gs.exact_margin(gate, Q, q, sc.prm)))
            if mg >= FAST_FIT_BAND:
                outside.append((sc.name, label, m, step, mg, int(g["flag"][i]), int(ref["flag"][i])))
            else:
                inside[gate] = inside.get(gate, 0) + 1
                worst[gate] = max(worst.get(gate, 0.0), mg)
        total += len(sc.patches)
    print("fast fit, %d cases: flips inside the band %.0e per gate %s, largest margin per gate %s; outside: %s"
          % (total, FAST_FIT_BAND, inside, {k: "%.1e" % v for k, v in worst.items()}, outside))
    assert not outside


def _walk():
    """translations of 1e-7 .. 1e-4 m back and forth along one direction, and one rotation"""
    d = np.array([0.48, -0.6, 0.64])
    poses, x = [], np.zeros(3)
    for step in (1e-7, -1e-7, 1e-6, 1e-5, -1e-5, 1e-4, -1e-4, -1e-6, 3e-5, -3e-5):
        x = x + step * d
        poses.append((np.eye(3), x.copy()))
    T = h.pose6d_matrix(0.0, 0.0, 0.0, 2e-6, -1e-6, 3e-6)
    poses.append((T[:3, :3], x.copy()))
    poses.append((np.eye(3), np.zeros(3)))
    return poses


OPTION_SETS = [dict(warm_start=0), dict(warm_start=1), dict(use_certificates=0), dict(use_certificates=1),
               dict(advance=2, team_pass=0), dict(advance=2, team_pass=2), dict(one_wave=2)]


@pytest.mark.parametrize("fast", [0, 1])
def test_walks_across_the_thresholds_are_history_free(scenes, fast):
    walk = _walk()
    for sc in scenes:
        if not (sc.name.startswith("weight") or sc.name.startswith("radius")):
            continue
        cold = [_cold(sc, fast, R, t) for R, t in walk]
        p = _lin_params(sc.prm)
        for opts in OPTION_SETS:
            c = _ctx(sc, fast, **opts)
            for (R, t), ref in zip(walk, cold):
                assert _same_sums(c.linearize(R, t, p), ref), (sc.name, fast, opts)
            c.close()
        # batched warm launches: state i is left by pose i - shift of the launch before
        n = len(walk)
        c = _ctx(sc, fast)
        c.reserve_warm_states(n)
        Rs = np.stack([R for R, _ in walk]); ts = np.stack([t for _, t in walk])
        for shift in (0, 1, 3, 0):
            outs = c.linearize_batch_warm(np.roll(Rs, shift, 0), np.roll(ts, shift, 0), np.arange(n), p)
            for o, j in zip(outs, np.roll(np.arange(n), shift)):
                assert _same_sums(o, cold[j]), (sc.name, fast, "batch", shift)
        c.close()


@pytest.mark.parametrize("fast", [0, 1])
def test_boundary_frame_through_register_frames(scenes, fast):
    """the boundary frame registered through dcreg_register_frames is bitwise its single registration"""
    for name in ("weight 0.9/0.1 wd=1", "radius R=0.3"):
        sc = next(s for s in scenes if s.name.startswith(name))
        T0 = h.pose6d_matrix(3e-5, -2e-5, 1e-5, 1e-6, 0.0, -2e-6)
        cfg = api.default_config(search_radius=sc.prm["search_radius"], max_iterations=10, use_weight_derivative=sc.prm["use_weight_derivative"])
        c = _ctx(sc, fast)
        one = h.single_registration(c, sc.source, T0, "Ours", cfg)
        rec = c.register_frames([sc.source], T0[None], "Ours", cfg)
        c.close()
        h.assert_record(rec[0], one, (name, fast))


def test_parameters_alternated_on_one_context(scenes):
    sc = next(s for s in scenes if s.name.startswith("weight 0.9/0.1 wd=0"))
    base = sc.prm
    variants = [dict(base), dict(base, weight_slope=0.5, weight_min=0.3), dict(base, use_weight_derivative=1),
                dict(base, weight_min=0.3), dict(base, min_normal_norm=1.0 / 40.0), dict(base, max_plane_thickness_sq=0.02 ** 2),
                dict(base, weight_slope=0.5)]
    for fast in (0, 1):
        c = _ctx(sc, fast)
        for _ in range(2):
            for prm in variants:
                out = c.linearize(np.eye(3), np.zeros(3), _lin_params(prm))
                assert _same_sums(out, _cold(sc, fast, np.eye(3), np.zeros(3), prm)), (fast, prm)
        c.close()


def test_euler_row_with_the_parity_fit(scenes):
    sc = next(s for s in scenes if s.name.startswith("weight 0.5/0.3 wd=0"))
    rpy = (0.0, 0.0, 0.0)
    ref = _oracle(sc, euler_rpy=rpy)
    c = _ctx(sc, 0)
    g = c.linearize(np.eye(3), np.zeros(3), _lin_params(sc.prm, euler_rpy=rpy), debug=True)
    c.close()
    assert np.array_equal(g["flag"], ref["flag"]) and g["n_eff"] == ref["n_eff"]
    assert np.abs(g["H_upper"] - ref["H_upper"]).max() <= 1e-9 * np.abs(ref["H_upper"]).max()
