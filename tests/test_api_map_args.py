"""Arguments the map-update methods of Context check before anything reaches the library (no device needed): clouds are 2-D float32
arrays with x y z in their first three columns (passed with their real row stride), poses are 4x4, crop boxes are two 3-vectors."""
import numpy as np
import pytest

from dcreg_amd import api

BAD = [np.zeros((10, 2), np.float32), np.zeros(30, np.float32), np.zeros((10, 3), np.float64), np.zeros((2, 5, 3), np.float32)]
GOOD = np.zeros((10, 3), np.float32)


def _bare():
    return object.__new__(api.Context)          # no device: the checks come first


@pytest.mark.parametrize("bad", BAD, ids=["2 columns", "1-D", "float64", "3-D"])
def test_clouds_that_are_not_xyz_rows_are_refused(bad):
    with pytest.raises(ValueError):
        _bare().insert(bad, np.eye(4))


@pytest.mark.parametrize("T", [np.eye(3), np.eye(4)[:3], np.zeros(16)], ids=["3x3", "3x4", "flat"])
def test_poses_must_be_4x4(T):
    with pytest.raises(ValueError, match="4x4"):
        _bare().insert(GOOD, T)
    with pytest.raises(ValueError, match="4x4"):
        _bare().insert_source(T)
    with pytest.raises(ValueError, match="4x4"):
        _bare().insert_device(0, 10, 3, T)


def test_crop_boxes_are_two_points():
    with pytest.raises(ValueError, match="3 coordinates"):
        _bare().crop([0, 0], [1, 1, 1])
    with pytest.raises(ValueError, match="3 coordinates"):
        _bare().crop([0, 0, 0], [[1, 1, 1]])
