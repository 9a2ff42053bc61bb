"""The robust kernels' names and what Context.set_robust checks before anything reaches the library (no device needed)."""
import numpy as np
import pytest

from dcreg_amd import api


class Recorder(api.Context):
    """a Context without a device: set_option only records"""

    def __new__(cls):
        c = object.__new__(cls)
        c.calls = []
        return c

    def __init__(self):
        pass

    def set_option(self, key, value):
        self.calls.append((key, value))

    def close(self):
        pass


def test_the_name_table_is_the_headers():
    assert api.ROBUST == {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3}
    header = open(api.os.path.join(api._HERE, "..", "include", "dcreg.h")).read()
    for name, code in (("NONE", 0), ("HUBER", 1), ("CAUCHY", 2), ("GEMAN_MCCLURE", 3)):
        assert "#define DCREG_ROBUST_%s %d\n" % (name, code) in header


def test_names_and_codes_reach_the_three_options():
    c = Recorder()
    c.set_robust("cauchy")
    assert c.calls == [("robust_kernel", 2)]
    c.calls.clear()
    c.set_robust(3, scale=0.05, gicp_scale=2)
    assert c.calls == [("robust_kernel", 3), ("robust_scale", 0.05), ("gicp_robust_scale", 2.0)]
    c.calls.clear()
    c.set_robust(np.int64(1), gicp_scale=1e6)
    assert c.calls == [("robust_kernel", 1), ("gicp_robust_scale", 1e6)]
    c.calls.clear()
    c.set_robust("none", scale=1e-6)
    assert c.calls == [("robust_kernel", 0), ("robust_scale", 1e-6)]


@pytest.mark.parametrize("kernel", ["tukey", "Huber", "", 4, -1, 1.0, 1.5, np.nan, None, True])
def test_an_unknown_kernel_is_refused_before_the_library(kernel):
    c = object.__new__(api.Context)          # no device: the checks come first
    with pytest.raises(ValueError, match="kernel"):
        c.set_robust(kernel)
    with pytest.raises(ValueError, match="kernel"):
        c.set_robust(kernel, scale=0.1, gicp_scale=1.0)


@pytest.mark.parametrize("bad", [0.0, -1.0, 9e-7, 1.0000001e6, 1e7, np.inf, -np.inf, np.nan, "x"])
def test_a_scale_outside_the_range_is_refused_before_the_library(bad):
    c = Recorder()
    with pytest.raises(ValueError, match="scale"):
        c.set_robust("huber", scale=bad)
    with pytest.raises(ValueError, match="gicp_scale"):
        c.set_robust("huber", gicp_scale=bad)
    with pytest.raises(ValueError, match="gicp_scale"):
        c.set_robust("huber", scale=0.1, gicp_scale=bad)
    assert c.calls == []                     # nothing was set, the kernel neither
