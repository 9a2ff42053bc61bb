"""The gates of one linearisation at their thresholds, on the host (tests/gate_scenes.py builds the scenes): the parity plane fit
(fast_plane_fit = 0) is bitwise the oracle's - plane, gate flags, residuals and weights - on points within a float step, or within
1e-13 .. 1e-7 relative, of a threshold.  The fast fit's band is measured on the GPU only (tests/test_gpu_gate_edges.py): on the host its
reciprocal and square root fall back to IEEE operations."""
from collections import Counter

import numpy as np
import pytest

import emul
import gate_scenes as gs
from oracle import pyoracle as po


@pytest.fixture(scope="module")
def scenes():
    return gs.all_scenes()


def _oracle(sc, debug=True):
    tree = po.KdTree(sc.target)
    return po.linearize(tree, sc.source, np.eye(3), np.zeros(3), gs.oracle_params(sc.prm), debug=debug)


def test_boundary_scenes_sit_on_the_edges(scenes):
    """Every case lies within the margin it was built for, each gate has cases on both sides of its flip in the full scene, and the
    full scene gives the flags the oracle gave each patch alone (the patches are isolated)."""
    per = Counter()
    for sc in scenes:
        ref = _oracle(sc)
        # isolated patches: a query's sixth nearest target point (another patch's) lies beyond 2 R (1 + cert_margin)
        _, d2 = po.KdTree(sc.target).knn(sc.source, k=6)
        assert np.all(d2[:, 5] > (2 * sc.prm["search_radius"] * (1 + gs.CERT_MARGIN)) ** 2), sc.name
        for i, (Q, q, gate, label, m, step) in enumerate(sc.patches):
            assert int(ref["flag"][i]) == gs.oracle_flag(Q, q, sc.prm), (sc.name, i, label)
            if m is not None:
                mg = abs(float(gs.exact_margin(gate, Q, q, sc.prm)))
                assert mg <= m, (sc.name, label, m, mg)
            per[(gate, "step" if m is None else m)] += 1
        if "r0" not in sc.name:
            fl = Counter(int(f) for f in ref["flag"])
            gate = sc.patches[0][2]
            assert fl[1] >= 10 and fl[gs.FLAG_OF_GATE[gate]] >= 10, (sc.name, fl)
    # float-step cases of every gate; exact-margin cases of the three plane gates at every margin
    assert per[("radius", "step")] >= 120 and per[("norm", "step")] >= 40 and per[("thickness", "step")] >= 80 and per[("weight", "step")] >= 160
    for m in gs.MARGINS:
        assert per[("weight", m)] >= 8 and per[("thickness", m)] >= 8 and per[("norm", m)] >= 6, per


def _random_neighbourhoods():
    rng = np.random.default_rng(3)
    for trial in range(3000):
        c = rng.uniform(-50, 50, 3)
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        u = np.cross(n, [1, 0, 0.3]); u /= np.linalg.norm(u); v = np.cross(n, u)
        Q = c + np.outer(rng.uniform(-0.4, 0.4, 5), u) + np.outer(rng.uniform(-0.4, 0.4, 5), v) + np.outer(rng.normal(0, 0.01, 5), n)
        yield Q.astype(np.float32).astype(np.float64)


def test_parity_plane_fit_is_bitwise_the_oracles(scenes):
    """plane_fit_qr + its normalisation (the parity instantiation) against orc_plane_fit: n, d and |x| bit for bit, on 3000 float-rounded
    random neighbourhoods and on every boundary patch."""
    Qs = list(_random_neighbourhoods()) + [np.asarray(Q, np.float64) for sc in scenes for (Q, *_r) in sc.patches]
    bad = []
    for i, Q in enumerate(Qs):
        n, d, ps = emul.plane_fit_nd(Q)
        rn, rd, rps = po.plane_fit(Q)
        if not (np.array_equal(n, rn) and d == rd and ps == rps):
            bad.append(i)
    assert not bad, "%d of %d planes differ from the oracle's (first: %s)" % (len(bad), len(Qs), bad[:5])


@pytest.mark.parametrize("warm", [False, True])
def test_parity_linearisation_is_bitwise_the_oracles_at_the_edges(scenes, warm):
    """emul.linearize with the parity fit on every boundary scene: flag, neighbours, normal, r and s bitwise the oracle's, and the
    sums within rounding of the reduction order; a second launch at the same pose reuses the stored planes and gives the same."""
    for sc in scenes:
        ref = _oracle(sc)
        R = sc.prm["search_radius"]
        idx, S = emul.Index(sc.target, R), emul.Source(sc.source)
        kw = dict(radius=R, wd=sc.prm["use_weight_derivative"], fast=False, warm=warm, max_thick_sq=sc.prm["max_plane_thickness_sq"],
                  min_norm=sc.prm["min_normal_norm"], w_slope=sc.prm["weight_slope"], w_min=sc.prm["weight_min"])
        for _ in range(2 if warm else 1):
            e = emul.linearize(idx, S, np.eye(3), np.zeros(3), debug=True, **kw)
            assert np.array_equal(e["flag"], ref["flag"]), sc.name
            got = ref["flag"] != 0                 # (a point that fails the radius gate keeps no neighbours)
            assert np.array_equal(e["nn_idx"][got], ref["nn_idx"][got]), sc.name
            assert np.array_equal(e["nn_d2"][got].view(np.uint32), ref["nn_d2"][got].view(np.uint32)), sc.name
            for k in ("normal", "r", "s"):
                assert np.array_equal(e[k], ref[k]), (sc.name, k, np.flatnonzero((e[k] != ref[k]).reshape(len(e[k]), -1).any(1)))
            assert e["n_eff"] == ref["n_eff"] and e["n_pt"] == ref["n_pt"]
            scale = np.abs(ref["H_upper"]).max()
            assert np.abs(e["H_upper"] - ref["H_upper"]).max() <= 1e-12 * scale, sc.name
            assert np.abs(e["g"] - ref["g"]).max() <= 1e-12 * max(np.abs(ref["g"]).max(), 1e-300), sc.name
