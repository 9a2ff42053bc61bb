"""Seeded random call sequences against a freshly built context (tests/state_walk.py has the model, the operations and the probes;
tests/test_state_walk_model.py what the committed walks cover).  Context A takes a walk of calls in an order no feature's own test tried;
at every check point a fresh context B is built from the model alone - options (the robust kernel, its scales, gicp_epsilon and the voxel
mode among them), set_target of the model's map, set_source, the normals, the kept voxels, the frames, the places, the keyframes - and both
answer the same probes, those of the voxel-distribution engine and of the three pair forms included.  A answers warm from its history, B
cold; include/dcreg.h promises that no bit differs.  The kept voxels and the voxel linearisation's dump are bitwise tests/voxels_ref.py's.
The walks also call the global-alignment chain - FPFH over k neighbours and over a radius, feature matching, the three-pair sampler and the
consensus graph - between the other families whose scratch these calls share; each answer is compared bitwise with the answer of a context
that has done nothing else, and the probe "desc" compares the map form of the descriptors of A and B (and, under given normals, with the
cloud form of the model's map).

A walk runs once and nothing is retried.  If a walk ends in anything but an AssertionError (a HIP error, a return code the model did not
expect from the library's side) the remaining walks are skipped: the cause is to be found by reading code, not by running again."""
import time

import numpy as np
import pytest

import state_walk as W
from dcreg_amd import api

pytestmark = pytest.mark.gpu

# Sequences that once failed, each the shortest that still did, as literals that state_walk.replay accepts (none so far).
PINNED = []

_stopped = []          # the reason the remaining walks are skipped


class GpuDeskew:
    """the expected source of the deskew forms: the cloud form on a helper context (include/dcreg.h: the two are bitwise equal)"""
    tag = "device"

    def __init__(self):
        self.ctx = None

    def __call__(self, path, rec):
        if self.ctx is None:
            self.ctx = api.Context(0)
        if path:
            field, st, P, block = W.sweep_args(True)
            out, _, _ = self.ctx.deskew_path([rec], field, st, P, block)
        else:
            field, motion = W.sweep_args(False)
            out, _, _ = self.ctx.deskew([rec], field, motion)
        return np.ascontiguousarray(out[0])

    def close(self):
        if self.ctx is not None:
            self.ctx.close()


@pytest.fixture(scope="module")
def deskew():
    d = GpuDeskew()
    yield d
    d.close()


def make():
    return api.Context(0)


def guarded(fn):
    if _stopped:
        pytest.skip("an earlier walk ended in %s: not run again until its cause is found" % _stopped[0])
    try:
        return fn()
    except AssertionError:
        raise
    except BaseException as e:
        _stopped.append("%s: %s" % (type(e).__name__, str(e)[:200]))
        raise


@pytest.mark.parametrize("seed", W.SEEDS)
def test_a_walk_answers_as_a_fresh_context(seed, deskew):
    ops = W.walk_ops(seed, W.N_STEPS)
    t0 = time.perf_counter()
    guarded(lambda: W.run_walk(make, seed, ops, W.EVERY, deskew=deskew))
    print("walk %d: %d steps, %d checks, %.2f s" % (seed, len(ops), len(W.check_points(ops, W.EVERY)), time.perf_counter() - t0))


def test_the_pinned_sequences(deskew):
    for n, ops in enumerate(PINNED):
        guarded(lambda: W.run_walk(make, "pinned %d" % n, ops, len(ops) + 1, deskew=deskew))
