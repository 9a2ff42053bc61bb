"""Arguments the consensus methods of Context check before anything reaches the library (no device needed), the structs against the
header and dcreg_sizeof, the default parameters and the refusals of the C-ABI that need no context."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)
IDX = np.arange(10, dtype=np.int32)


def test_the_structs_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.ConsensusParams._fields_] == ["compat_distance", "min_length", "inlier_distance", "n_seeds", "consensus_size", "n_best",
                                                            "refine_iterations", "reserved_"]
    assert [f[0] for f in api.ConsensusRecord._fields_] == ["T", "seed", "seed_rank", "weight", "n_members", "count", "cost", "n_inliers", "refined",
                                                            "rmse"]
    assert [f[0] for f in api.ConsensusInfo._fields_] == ["n_pairs", "n_used", "n_edges", "max_degree", "n_seeds", "n_skipped", "n_scored", "n_returned",
                                                          "reserved_"]
    assert (C.sizeof(api.ConsensusParams), C.sizeof(api.ConsensusRecord), C.sizeof(api.ConsensusInfo)) == (56, 176, 72)
    R = api.ConsensusRecord
    assert (R.seed.offset, R.n_members.offset, R.count.offset, R.cost.offset, R.n_inliers.offset, R.rmse.offset) == (128, 140, 144, 152, 160, 168)
    for name, cls in (("dcreg_consensus_params", api.ConsensusParams), ("dcreg_consensus_record", api.ConsensusRecord),
                      ("dcreg_consensus_info", api.ConsensusInfo)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name
        assert api._STRUCTS[name] is cls
    for name in ("dcreg_default_consensus_params", "dcreg_consensus_correspondences", "dcreg_consensus_correspondences_device"):
        assert name in api.EXPORTS and hasattr(L, name), name


def test_the_default_parameters():
    p = api.ConsensusParams()
    p.compat_distance, p.min_length, p.n_seeds, p.n_best, p.reserved_[1] = 9.0, 5.0, 2, 4, 4.0
    assert api.load().dcreg_default_consensus_params(C.byref(p)) == api.OK
    assert (p.compat_distance, p.min_length, p.inlier_distance, p.n_seeds, p.consensus_size, p.n_best, p.refine_iterations, list(p.reserved_)) == \
        (0.5, 1.0, 0.5, 64, 16, 1, 3, [0.0, 0.0])
    assert bytes(p) == bytes(api.consensus_params())
    assert api.load().dcreg_default_consensus_params(None) == -1
    q = api.consensus_params(compat_distance=1e-9, min_length=0.0, inlier_distance=0.1, n_seeds=1024, consensus_size=64, n_best=32, refine_iterations=8)
    assert (q.min_length, q.n_seeds, q.consensus_size, q.n_best, q.refine_iterations) == (0.0, 1024, 64, 32, 8)
    api.consensus_params(n_seeds=1, consensus_size=3, n_best=1, refine_iterations=0)


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p = api.consensus_params()
    recs = (api.ConsensusRecord * 1)()
    info = api.ConsensusInfo()
    mask = np.zeros(10, np.uint8)
    members = np.full(16, 7, np.int32)
    args = (CLOUD.ctypes.data, 10, 3, CLOUD.ctypes.data, 10, 3, IDX.ctypes.data, IDX.ctypes.data, 10, C.byref(p), recs, mask.ctypes.data,
            members.ctypes.data, None, None, C.byref(info))
    assert L.dcreg_consensus_correspondences(None, *args) == -1
    assert L.dcreg_consensus_correspondences_device(None, *args) == -1
    assert info.n_pairs == 0 and not mask.any() and not any(recs[0].T) and (members == 7).all()


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def _block(**kw):
    p = api.consensus_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [("compat_distance", 0.0), ("compat_distance", -0.5), ("compat_distance", np.nan), ("compat_distance", np.inf), ("min_length", -0.1),
              ("min_length", np.nan), ("min_length", np.inf), ("inlier_distance", 0.0), ("inlier_distance", -0.5), ("inlier_distance", np.nan),
              ("inlier_distance", np.inf), ("n_seeds", 0), ("n_seeds", 1025), ("consensus_size", 2), ("consensus_size", 65), ("n_best", 0),
              ("n_best", 33), ("refine_iterations", -1), ("refine_iterations", 9)]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    with pytest.raises(ValueError, match=field):
        api.consensus_params(**{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.consensus_correspondences(CLOUD, CLOUD, IDX, IDX, p),
                 lambda: c.consensus_correspondences_device(1, 10, 3, 1, 10, 3, 1, 1, 10, p)):
        with pytest.raises(ValueError, match=field):
            call()


def test_clouds_index_arrays_and_counts_are_checked():
    c = _ctx()
    for call in (lambda: c.consensus_correspondences(np.zeros((4, 2), np.float32), CLOUD, IDX, IDX),
                 lambda: c.consensus_correspondences(CLOUD, np.zeros((4, 3), np.float64), IDX, IDX),
                 lambda: c.consensus_correspondences(CLOUD, np.zeros(30, np.float32), IDX, IDX)):
        with pytest.raises(ValueError, match="float32"):
            call()
    for call in (lambda: c.consensus_correspondences(CLOUD, CLOUD, IDX.astype(np.float32), IDX),
                 lambda: c.consensus_correspondences(CLOUD, CLOUD, IDX, IDX.reshape(2, 5)),
                 lambda: c.consensus_correspondences(CLOUD, CLOUD, IDX, np.array([2 ** 31], np.int64))):
        with pytest.raises(ValueError, match="index"):
            call()
    with pytest.raises(ValueError, match="one length"):
        c.consensus_correspondences(CLOUD, CLOUD, IDX, IDX[:9])
    with pytest.raises(ValueError, match="consensus_params"):
        c.consensus_correspondences(CLOUD, CLOUD, IDX, IDX, api.align_params())
    big = np.zeros(32769, np.int32)
    with pytest.raises(ValueError, match="32768 pairs"):
        c.consensus_correspondences(CLOUD, CLOUD, big, big)
    for call in (lambda: c.consensus_correspondences_device(1, 10, 2, 1, 10, 3, 1, 1, 10), lambda: c.consensus_correspondences_device(1, 10, 3, 1, 10, 0, 1, 1, 10)):
        with pytest.raises(ValueError, match="stride"):
            call()
    for call in (lambda: c.consensus_correspondences_device(1, -1, 3, 1, 10, 3, 1, 1, 10),
                 lambda: c.consensus_correspondences_device(1, 10, 3, 1, 2 ** 31, 3, 1, 1, 10)):
        with pytest.raises(ValueError, match="points"):
            call()
    for call in (lambda: c.consensus_correspondences_device(1, 10, 3, 1, 10, 3, 1, 1, -1),
                 lambda: c.consensus_correspondences_device(1, 10, 3, 1, 10, 3, 1, 1, 32769)):
        with pytest.raises(ValueError, match="pairs"):
            call()
    for call in (lambda: c.consensus_correspondences_device(1, 10, 3, 1, 10, 3, 0, 1, 10),
                 lambda: c.consensus_correspondences_device(1, 10, 3, 1, 10, 3, 1, 0, 10)):
        with pytest.raises(ValueError, match="index arrays"):
            call()
