"""The numpy reference of the fourth engine (tests/voxels_ref.py) against its own properties, without a device: the counts of the scenes,
the clamp on a plane and on a line, W^T W = S^-1, and the third engine's reference as the special case C' = I - c n n^T."""
import numpy as np

import gicp_ref as gref
import voxels_ref as vr
import voxels_scenes as vs


def test_the_scenes_hold_every_kind_of_voxel_and_point():
    L = vs.lot()
    m = L["vmap"]
    assert (m["n_points"], m["n_voxels"], m["n_small"], m["n_degenerate"], m["n_kept"]) == (4000, 668, 285, 0, 383)
    assert vr.linearize(m, L["src"], L["GT"])["n_pt"] == 395 and vr.linearize(m, L["src"], L["INIT"])["n_pt"] == 365
    P = vs.planted()
    p = P["vmap"]
    assert (p["n_voxels"], p["n_small"], p["n_degenerate"], p["n_kept"]) == (8, 1, 1, 6)
    assert sorted(p["count"].tolist()) == [6, 6, 6, 6, 7, 9]
    for mode in (0, 1):
        assert vr.linearize(p, P["src"], P["T"], mode, P["src_normals"])["flag"].tolist() == P["flags%d" % mode]
    # ascending (z, y, x)
    for m_ in (m, p, vs.lattice()["vmap"]):
        c = m_["coords"]
        key = (c[:, 2] * (1 << 42)) + (c[:, 1] * (1 << 21)) + c[:, 0]
        assert (np.diff(key) > 0).all()


def test_a_plane_clamps_one_eigenvalue_along_its_normal_and_a_line_two():
    n = np.array([1.0, 2.0, 2.0]) / 3.0
    a, b = np.cross(n, [1.0, 0.0, 0.0]), None
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    g = np.linspace(-0.15, 0.15, 7)
    uv = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)       # a square patch: the same spread along both directions of the plane
    pts = (np.array([10.5, 20.5, 30.5]) + uv[:, :1] * a + uv[:, 1:] * b).astype(np.float32)
    m = vr.voxel_map(pts, 1.0, 1e-3, 6)
    assert m["n_kept"] == 1 and m["count"][0] == 49
    l = np.sort(m["l"][0])
    assert l[0] == 1e-3 and l[2] == 1.0 and 0.999 < l[1] <= 1.0
    k = int(np.argmin(m["lam"][0]))
    assert abs(abs(m["V"][0][:, k] @ n) - 1.0) < 1e-6
    # C' has the eigenvalues l: along the normal epsilon
    Cp = m["cov64"][0]
    C = np.array([[Cp[0], Cp[1], Cp[2]], [Cp[1], Cp[3], Cp[4]], [Cp[2], Cp[4], Cp[5]]])
    assert abs(n @ C @ n - 1e-3) < 1e-9
    line = vs.planted()["vmap"]
    assert any(np.array_equal(np.sort(x), [1e-3, 1e-3, 1.0]) for x in line["l"])


def test_w_whitens_the_covariance():
    L = vs.lot()
    for mode in (0, 1):
        r = vr.linearize(L["vmap"], L["src"], L["MID"], mode, L["m5"])
        eff = np.flatnonzero(r["flag"] == 1)
        assert len(eff) > 300
        R = L["MID"][:3, :3]
        for i in eff[::7]:
            s = r["cov"][i].copy()
            if mode:
                s = s + vr.source_cov(R, r["normal_src"][i:i + 1], 1.0 - 1e-3)[0]
            S = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
            W = r["w"][i]
            assert np.abs(W.T @ W @ S - np.eye(3)).max() < 1e-12 * np.linalg.cond(S)
            assert np.abs(W @ S @ W.T - np.eye(3)).max() < 1e-12


def test_mode_1_with_a_plane_record_is_the_third_engine():
    """C' = I - c n n^T with values every step represents exactly (epsilon = 2^-10, axis normals, a quarter turn): the voxel rule's W and
    rows are bitwise gicp_ref's for the same e"""
    eps = 2.0 ** -10
    c = 1.0 - eps
    rng = np.random.default_rng(9)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (10.25, 20.5, 30.125)
    axes = np.eye(3, dtype=np.float32)
    for a in range(3):
        for b in range(3):
            nrm, m = axes[a], axes[b]
            src = rng.uniform(-0.4, 0.4, (8, 3)).astype(np.float32)
            q = vr.transform(R, T[:3, 3], src)
            # one map point per source point: t_j = the voxel's mean, so that e is the same in both rules
            tj = np.array([[10.5, 20.5, 30.5]], np.float32)
            Cp = np.eye(3) - c * np.outer(nrm, nrm)
            vmap = dict(coords=np.array([[0, 0, 0]], np.int64), count=np.array([6], np.int32), mean=tj,
                        cov=np.array([[Cp[0, 0], Cp[1, 0], Cp[2, 0], Cp[1, 1], Cp[2, 1], Cp[2, 2]]], np.float32), leaf=100.0)
            assert (vr.voxel_of(q, 100.0) == 0.0).all()
            got = vr.linearize(vmap, src, T, 1, np.tile(m, (8, 1)), eps)
            want = gref.linearize(tj, nrm[None, :], src, np.tile(m, (8, 1)), T, 10.0, eps)
            assert (got["flag"] == 1).all() and (want["flag"] == 1).all()
            for k in ("w", "r", "row"):
                assert got[k].tobytes() == want[k].tobytes(), (a, b, k)


def test_the_robust_factor_scales_slots_0_to_6():
    L = vs.lot()
    plain = vr.linearize(L["vmap"], L["src"], L["INIT"])
    for kind in (1, 2, 3):
        r = vr.linearize(L["vmap"], L["src"], L["INIT"], kind=kind, scale=0.7)
        eff = r["flag"] == 1
        assert np.array_equal(r["flag"], plain["flag"]) and (r["k"][eff] <= 1.0).all() and (r["k"][eff] < 1.0).any()
        assert np.array_equal(r["row"][..., 7], plain["row"][..., 7])
        assert np.array_equal(r["row"][eff][:, :, :7], r["k"][eff][:, None, None] * plain["row"][eff][:, :, :7])
