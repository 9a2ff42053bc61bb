"""The Python-side argument checks of register_pairs_normals and register_pairs_gicp (dcreg_amd/api.py), on a bare Context: every refusal
comes before the library is touched."""
import numpy as np
import pytest

from dcreg_amd import api

CALLS = ["register_pairs_normals", "register_pairs_gicp"]


def bare():
    return object.__new__(api.Context)


def cloud(n, c=3):
    return np.zeros((n, c), np.float32)


def poses(n):
    return np.tile(np.eye(4), (n, 1, 1))


@pytest.mark.parametrize("call", CALLS)
def test_clouds_that_are_not_xyz_are_refused(call):
    f = getattr(bare(), call)
    cfg = api.default_config()
    with pytest.raises(ValueError):
        f([np.zeros((5, 2), np.float32)], [cloud(5)], poses(1), "Ours", cfg)
    with pytest.raises(ValueError):
        f([cloud(5)], [np.zeros(7, np.float32)], poses(1), "Ours", cfg)


@pytest.mark.parametrize("call", CALLS)
def test_mixed_widths_are_refused(call):
    f = getattr(bare(), call)
    with pytest.raises(ValueError, match="same number of columns"):
        f([cloud(5, 3), cloud(5, 4)], [cloud(5, 3), cloud(5, 3)], poses(2), "Ours", api.default_config())
    with pytest.raises(ValueError, match="same number of columns"):
        f([cloud(5, 4)], [cloud(5, 3)], poses(1), "Ours", api.default_config())


@pytest.mark.parametrize("call", CALLS)
def test_one_target_and_one_pose_per_source(call):
    f = getattr(bare(), call)
    with pytest.raises(ValueError, match="one target per source"):
        f([cloud(5), cloud(5)], [cloud(5)], poses(2), "Ours", api.default_config())
    with pytest.raises(ValueError, match="one initial pose per pair"):
        f([cloud(5), cloud(5)], [cloud(5), cloud(5)], poses(3), "Ours", api.default_config())


def bad_params():
    out = []
    for k in (2, 33):
        p = api.normal_params()
        p.k = k
        out.append(p)
    p = api.normal_params()
    p.orient = 7
    out.append(p)
    for r in (-1.0, np.nan, np.inf):
        p = api.normal_params()
        p.search_radius = r
        out.append(p)
    p = api.normal_params()
    p.viewpoint[1] = np.nan
    out.append(p)
    return out + ["k=5", 5]


@pytest.mark.parametrize("bad", bad_params(), ids=lambda p: "p")
def test_bad_normal_parameters_are_refused(bad):
    c = bare()
    args = ([cloud(5)], [cloud(5)], poses(1), "Ours", api.default_config())
    with pytest.raises(ValueError, match="register_pairs_normals"):
        c.register_pairs_normals(*args, target_normals=bad)
    with pytest.raises(ValueError, match="register_pairs_gicp"):
        c.register_pairs_gicp(*args, target_normals=bad)
    with pytest.raises(ValueError, match="register_pairs_gicp"):
        c.register_pairs_gicp(*args, source_normals=bad)


def test_the_three_pairs_calls_share_their_checks():
    """register_pairs refuses the same arguments, in the same words but for its name"""
    c = bare()
    for call in ["register_pairs"] + CALLS:
        with pytest.raises(ValueError, match="%s: one target per source: 2 sources, 1 targets" % call):
            getattr(c, call)([cloud(5), cloud(5)], [cloud(5)], poses(2), "Ours", api.default_config())
