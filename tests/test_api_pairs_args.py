"""Arguments Context.register_pairs checks before anything reaches the library (no device needed): every source and target is a 2-D
float32 array with x y z in its first three columns, all of one width (passed with that real row stride), one target and one initial pose
per source."""
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
        _bare().register_pairs([bad], [GOOD], np.eye(4)[None], "Ours", None)
    with pytest.raises(ValueError):
        _bare().register_pairs([GOOD], [bad], np.eye(4)[None], "Ours", None)


def test_clouds_of_different_widths_are_refused():
    with pytest.raises(ValueError, match="columns"):
        _bare().register_pairs([GOOD], [np.zeros((10, 4), np.float32)], np.eye(4)[None], "Ours", None)
    with pytest.raises(ValueError, match="columns"):
        _bare().register_pairs([GOOD, np.zeros((4, 4), np.float32)], [GOOD, GOOD], np.stack([np.eye(4)] * 2), "Ours", None)


def test_one_target_and_one_pose_per_source():
    with pytest.raises(ValueError, match="one target per source"):
        _bare().register_pairs([GOOD, GOOD], [GOOD], np.stack([np.eye(4)] * 2), "Ours", None)
    with pytest.raises(ValueError, match="one initial pose per pair"):
        _bare().register_pairs([GOOD, GOOD], [GOOD, GOOD], np.eye(4)[None], "Ours", None)
