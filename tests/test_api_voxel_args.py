"""Arguments the voxel-grid methods of Context check before anything reaches the library (no device needed): the leaf is one edge or three,
finite and > 0; the mode is "centroid" or "first"; clouds are 2-D float32 arrays with x y z in their first three columns; offsets start at
0, do not decrease and end at the number of points."""
import numpy as np
import pytest

from dcreg_amd import api

GOOD = np.zeros((10, 3), np.float32)
BAD_CLOUDS = [np.zeros((10, 2), np.float32), np.zeros(30, np.float32), np.zeros((10, 3), np.float64), np.zeros((2, 5, 3), np.float32)]


def _bare():
    return object.__new__(api.Context)          # no device: the checks come first


def _calls(leaf=0.5, mode="centroid", cloud=GOOD):
    c = _bare()
    return [lambda: c.voxel_downsample([cloud], leaf, mode), lambda: c.set_source_voxel(cloud, leaf, mode),
            lambda: c.set_target_voxel(cloud, 1.0, leaf, mode), lambda: c.set_source_voxel_device(0, 10, 3, leaf, mode),
            lambda: c.set_target_voxel_device(0, 10, 3, 1.0, leaf, mode),
            lambda: c.voxel_downsample_device(0, [0, 10], 3, 0, 10, leaf, mode)]


@pytest.mark.parametrize("leaf", [0.0, -0.1, np.nan, np.inf, -np.inf, [0.1, 0.0, 0.1], [0.1, np.nan, 0.1]],
                         ids=["zero", "negative", "nan", "inf", "-inf", "zero y", "nan y"])
def test_leaves_that_are_not_finite_and_positive_are_refused(leaf):
    for call in _calls(leaf=leaf):
        with pytest.raises(ValueError, match="leaf"):
            call()


@pytest.mark.parametrize("leaf", [[], [0.1, 0.1], [0.1] * 4, np.full((3, 3), 0.1)], ids=["none", "two", "four", "3x3"])
def test_leaves_with_the_wrong_number_of_edges_are_refused(leaf):
    for call in _calls(leaf=leaf):
        with pytest.raises(ValueError, match="leaf"):
            call()


@pytest.mark.parametrize("mode", ["mean", "CENTROID", "", 0, None])
def test_unknown_modes_are_refused(mode):
    for call in _calls(mode=mode):
        with pytest.raises(ValueError, match="mode"):
            call()


@pytest.mark.parametrize("bad", BAD_CLOUDS, ids=["2 columns", "1-D", "float64", "3-D"])
def test_clouds_that_are_not_xyz_rows_are_refused(bad):
    c = _bare()
    with pytest.raises(ValueError):
        c.voxel_downsample([bad], 0.5)
    with pytest.raises(ValueError):
        c.voxel_downsample((bad, [0, len(bad)]), 0.5)
    with pytest.raises(ValueError):
        c.set_source_voxel(bad, 0.5)
    with pytest.raises(ValueError):
        c.set_target_voxel(bad, 1.0, 0.5)


def test_clouds_of_a_call_share_their_columns():
    with pytest.raises(ValueError, match="columns"):
        _bare().voxel_downsample([GOOD, np.zeros((4, 4), np.float32)], 0.5)


@pytest.mark.parametrize("off", [[1, 10], [0, 5, 3, 10], [0, 9], [0, 11], [5]], ids=["start 1", "decrease", "short", "long", "no zero"])
def test_mismatched_offsets_are_refused(off):
    with pytest.raises(ValueError, match="offsets"):
        _bare().voxel_downsample((GOOD, off), 0.5)


@pytest.mark.parametrize("off", [[1, 10], [0, 5, 3, 10], [5]], ids=["start 1", "decrease", "no zero"])
def test_mismatched_device_offsets_are_refused(off):
    with pytest.raises(ValueError, match="offsets"):
        _bare().voxel_downsample_device(0, off, 3, 0, 10, 0.5)


def test_the_parameter_block_matches_the_header():
    p = api.voxel_params(0.25, "first", 3)
    assert list(p.leaf) == [0.25] * 3 and p.mode == 1 and p.min_points == 3
    p = api.voxel_params([0.1, 0.2, 0.3])
    assert list(p.leaf) == [0.1, 0.2, 0.3] and p.mode == 0 and p.min_points == 1
