"""Arguments the Python binding checks before anything reaches the library (no device needed): the clouds of knn, knn_timed and
register_frames are 2-D float32 arrays with x y z in the first three columns, passed with their real row stride."""
import numpy as np
import pytest

from dcreg_amd import api

BAD = [np.zeros((10, 2), np.float32), np.zeros(30, np.float32), np.zeros((10, 3), np.float64), np.zeros((2, 5, 3), np.float32)]


@pytest.mark.parametrize("bad", BAD, ids=["2 columns", "1-D", "float64", "3-D"])
def test_clouds_that_are_not_xyz_rows_are_refused(bad):
    ctx = object.__new__(api.Context)          # no device: the check comes first
    with pytest.raises(ValueError):
        ctx.knn(bad)
    with pytest.raises(ValueError):
        ctx.knn_timed(bad)
    with pytest.raises(ValueError):
        ctx.register_frames([bad], np.eye(4)[None], "Ours", None)
    with pytest.raises(ValueError):
        ctx.register_frames((bad, np.array([0, len(bad)])), np.eye(4)[None], "Ours", None)


def test_frames_of_different_widths_are_refused():
    ctx = object.__new__(api.Context)
    with pytest.raises(ValueError):
        ctx.register_frames([np.zeros((4, 3), np.float32), np.zeros((4, 4), np.float32)], np.stack([np.eye(4)] * 2), "Ours", None)
