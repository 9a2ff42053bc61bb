"""Host replay of the second and third engine's per-point functions with a robust kernel on (dcreg_amd/csrc/device/normal_icp.hpp and
gicp.hpp through tests/emul_robust.py) against the numpy reference of tests/robust_ref.py: flags, residuals, weights, whitening matrices
and the SCALED rows bitwise, over the poses of the walk, for every kernel at a small and a large scale; warm and cold replays agree bit
for bit; with no kernel the replay is the plain references'."""
import numpy as np
import pytest

import emul_robust as er
import gicp_scenes as gs
import normal_icp_scenes as sc
import robust_ref as rr
import robust_scenes as rs

RADIUS = sc.RADIUS


@pytest.fixture(scope="module")
def maps():
    L = gs.lot()
    return er.Map(L["tgt"], L["nb"], RADIUS)


@pytest.fixture(scope="module")
def nearest():
    """the nearest map point of every frame point at every pose of the walk: shared by all kernels and scales"""
    import normal_icp_ref as ref
    L = gs.lot()
    return [ref.nearest(L["tgt"], ref.transform(T[:3, :3], T[:3, 3], L["src"])) for T in sc.walk()]


@pytest.mark.parametrize("kind", rs.KINDS)
@pytest.mark.parametrize("c", rs.SCALES_N)
def test_the_second_engine_is_bitwise_the_reference_along_the_walk(maps, nearest, kind, c):
    L = gs.lot()
    warm_src, cold_src = er.Source(L["src"]), er.Source(L["src"])
    for step, T in enumerate(sc.walk()):
        want = rr.linearize_normals(L["tgt"], L["nb"], L["src"], T, RADIUS, kind, c, use_weight_derivative=1, nn=nearest[step])
        w = er.linearize_normals(maps, warm_src, T, RADIUS, kind, c, wd=1, warm=True)
        d = er.linearize_normals(maps, cold_src, T, RADIUS, kind, c, wd=1, warm=False)
        assert w["warm_used"] == (step > 0) and not d["warm_used"]
        for got in (w, d):
            sc.assert_dump_bitwise(got, want, (kind, c, step))
            sc.assert_sums_close(got, want, (kind, c, step))
        sc.assert_sums_bitwise(w, d, (kind, c, step))
        eff = want["flag"] == 1
        assert np.array_equal(want["row"][eff, 7], want["r"][eff])                     # slot 7 stays the residual
        if step == 0:
            k, u2 = rr.point_factors_normals(want, kind, c)
            assert (k < 1.0).any() and (k > 0.0).all() and (k <= 1.0).all()
            if kind == 1 and c == min(rs.SCALES_N):                                    # both Huber branches are taken
                u = np.sqrt(u2)
                assert (u <= 1.0).any() and (u > 1.0).any()
                assert (k[u <= 1.0] == 1.0).all() and (k[u > 1.0] < 1.0).all()


@pytest.mark.parametrize("kind", rs.KINDS)
@pytest.mark.parametrize("c", rs.SCALES_G)
def test_the_third_engine_is_bitwise_the_reference_along_the_walk(maps, nearest, kind, c):
    L = gs.lot()
    warm_src, cold_src = er.Source(L["src"], L["mb"]), er.Source(L["src"], L["mb"])
    for step, T in enumerate(sc.walk()):
        want = rr.linearize_gicp(L["tgt"], L["nb"], L["src"], L["mb"], T, RADIUS, kind, c, gs.EPS, nn=nearest[step])
        w = er.linearize_gicp(maps, warm_src, T, RADIUS, kind, c, gs.EPS, warm=True)
        d = er.linearize_gicp(maps, cold_src, T, RADIUS, kind, c, gs.EPS, warm=False)
        assert w["warm_used"] == (step > 0) and not d["warm_used"]
        for got in (w, d):
            gs.assert_dump_bitwise(got, want, (kind, c, step))
            sc.assert_sums_close(got, want, (kind, c, step))
        sc.assert_sums_bitwise(w, d, (kind, c, step))
        eff = want["flag"] == 1
        assert np.array_equal(want["row"][eff, :, 7], want["r"][eff])
        if step == 0:
            k, u2 = rr.point_factors_gicp(want, kind, c)
            assert (k < 1.0).any() and (k > 0.0).all() and (k <= 1.0).all()
            if kind == 1 and c == min(rs.SCALES_G):
                u = np.sqrt(u2)
                assert (u <= 1.0).any() and (u > 1.0).any()
                assert (k[u <= 1.0] == 1.0).all() and (k[u > 1.0] < 1.0).all()


def test_no_kernel_replays_the_plain_references(maps):
    import gicp_ref as gref
    import normal_icp_ref as ref
    L = gs.lot()
    T = L["INIT"]
    a = er.linearize_normals(maps, er.Source(L["src"]), T, RADIUS, 0, 0.02, wd=1, warm=False)
    sc.assert_dump_bitwise(a, ref.linearize(L["tgt"], L["nb"], L["src"], T, RADIUS, use_weight_derivative=1))
    b = er.linearize_gicp(maps, er.Source(L["src"], L["mb"]), T, RADIUS, 0, 0.5, gs.EPS, warm=False)
    gs.assert_dump_bitwise(b, gref.linearize(L["tgt"], L["nb"], L["src"], L["mb"], T, RADIUS, gs.EPS))


def test_the_planted_huber_edge_on_the_host():
    m = er.Map(rs.EDGE_MAP, rs.EDGE_NORMALS, RADIUS)
    got = er.linearize_normals(m, er.Source(rs.EDGE_SRC), np.eye(4), RADIUS, 1, rs.EDGE_SCALE, wd=0, warm=False)
    assert list(got["flag"]) == [1, 1, 1] and list(got["r"]) == [0.0, 0.125, 0.25]
    assert tuple(got["row"][:, 5] / got["s"]) == rs.EDGE_K
    E = rs.gicp_edge()
    got = er.linearize_gicp(m, er.Source(E["src"], E["src_normals"]), np.eye(4), RADIUS, 1, E["c"], gs.EPS, warm=False)
    plain = er.linearize_gicp(m, er.Source(E["src"], E["src_normals"]), np.eye(4), RADIUS, 0, E["c"], gs.EPS, warm=False)
    assert list(got["flag"]) == [1, 1, 1]
    assert tuple(got["row"][:, 2, 5] / plain["row"][:, 2, 5]) == E["k"] and E["k"][:2] == (1.0, 1.0) and E["k"][2] < 1.0
