"""Arguments the alignment methods of Context check before anything reaches the library (no device needed), the structs against the
header and dcreg_sizeof, the default parameters, the refusals of the C-ABI that need no context, and correspondences_from_match."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)
IDX = np.arange(10, dtype=np.int32)


def test_the_structs_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.AlignParams._fields_] == ["n_hypotheses", "seed", "inlier_distance", "edge_similarity", "n_best", "refine_iterations",
                                                        "reserved_"]
    assert [f[0] for f in api.AlignRecord._fields_] == ["T", "hypothesis", "pairs", "count", "cost", "n_inliers", "refined", "rmse"]
    assert [f[0] for f in api.AlignInfo._fields_] == ["n_pairs", "n_used", "n_drawn", "n_degenerate", "n_rejected", "n_scored", "n_returned", "reserved_"]
    assert (C.sizeof(api.AlignParams), C.sizeof(api.AlignRecord), C.sizeof(api.AlignInfo)) == (56, 176, 64)
    assert (api.AlignRecord.hypothesis.offset, api.AlignRecord.pairs.offset, api.AlignRecord.cost.offset, api.AlignRecord.rmse.offset) == (128, 136, 152, 168)
    for name, cls in (("dcreg_align_params", api.AlignParams), ("dcreg_align_record", api.AlignRecord), ("dcreg_align_info", api.AlignInfo)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name
        assert api._STRUCTS[name] is cls
    for name in ("dcreg_default_align_params", "dcreg_align_correspondences", "dcreg_align_correspondences_device"):
        assert name in api.EXPORTS and hasattr(L, name), name


def test_the_default_parameters():
    p = api.AlignParams()
    p.n_hypotheses, p.seed, p.inlier_distance, p.n_best, p.reserved_[1] = 9, 5, 2.0, 4, 4.0
    assert api.load().dcreg_default_align_params(C.byref(p)) == api.OK
    assert (p.n_hypotheses, p.seed, p.inlier_distance, p.edge_similarity, p.n_best, p.refine_iterations, list(p.reserved_)) == \
        (100000, 0, 0.5, 0.9, 1, 3, [0.0, 0.0])
    assert bytes(p) == bytes(api.align_params())
    assert api.load().dcreg_default_align_params(None) == -1
    q = api.align_params(n_hypotheses=1 << 24, seed=2 ** 64 - 1, inlier_distance=0.1, edge_similarity=0.0, n_best=32, refine_iterations=8)
    assert (q.n_hypotheses, q.seed, q.n_best, q.refine_iterations) == (1 << 24, 2 ** 64 - 1, 32, 8)
    api.align_params(n_hypotheses=1, n_best=1, refine_iterations=0)


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p = api.align_params()
    recs = (api.AlignRecord * 1)()
    info = api.AlignInfo()
    mask = np.zeros(10, np.uint8)
    args = (CLOUD.ctypes.data, 10, 3, CLOUD.ctypes.data, 10, 3, IDX.ctypes.data, IDX.ctypes.data, 10, C.byref(p), recs, mask.ctypes.data, C.byref(info))
    assert L.dcreg_align_correspondences(None, *args) == -1
    assert L.dcreg_align_correspondences_device(None, *args) == -1
    assert info.n_pairs == 0 and not mask.any() and not any(recs[0].T)


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def _block(**kw):
    p = api.align_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [("n_hypotheses", 0), ("n_hypotheses", -3), ("n_hypotheses", (1 << 24) + 1), ("inlier_distance", 0.0), ("inlier_distance", -0.5),
              ("inlier_distance", np.nan), ("inlier_distance", np.inf), ("edge_similarity", -0.1), ("edge_similarity", 1.0), ("edge_similarity", np.nan),
              ("edge_similarity", np.inf), ("n_best", 0), ("n_best", 33), ("refine_iterations", -1), ("refine_iterations", 9)]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    with pytest.raises(ValueError, match=field):
        api.align_params(**{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.align_correspondences(CLOUD, CLOUD, IDX, IDX, p), lambda: c.align_correspondences_device(1, 10, 3, 1, 10, 3, 1, 1, 10, p)):
        with pytest.raises(ValueError, match=field):
            call()


def test_clouds_index_arrays_and_counts_are_checked():
    c = _ctx()
    for call in (lambda: c.align_correspondences(np.zeros((4, 2), np.float32), CLOUD, IDX, IDX),
                 lambda: c.align_correspondences(CLOUD, np.zeros((4, 3), np.float64), IDX, IDX),
                 lambda: c.align_correspondences(CLOUD, np.zeros(30, np.float32), IDX, IDX)):
        with pytest.raises(ValueError, match="float32"):
            call()
    for call in (lambda: c.align_correspondences(CLOUD, CLOUD, IDX.astype(np.float32), IDX), lambda: c.align_correspondences(CLOUD, CLOUD, IDX, IDX.reshape(2, 5)),
                 lambda: c.align_correspondences(CLOUD, CLOUD, IDX, np.array([2 ** 31], np.int64))):
        with pytest.raises(ValueError, match="index"):
            call()
    with pytest.raises(ValueError, match="one length"):
        c.align_correspondences(CLOUD, CLOUD, IDX, IDX[:9])
    with pytest.raises(ValueError, match="align_params"):
        c.align_correspondences(CLOUD, CLOUD, IDX, IDX, api.fpfh_params())
    for call in (lambda: c.align_correspondences_device(1, 10, 2, 1, 10, 3, 1, 1, 10), lambda: c.align_correspondences_device(1, 10, 3, 1, 10, 0, 1, 1, 10)):
        with pytest.raises(ValueError, match="stride"):
            call()
    for call in (lambda: c.align_correspondences_device(1, -1, 3, 1, 10, 3, 1, 1, 10), lambda: c.align_correspondences_device(1, 10, 3, 1, 2 ** 31, 3, 1, 1, 10)):
        with pytest.raises(ValueError, match="points"):
            call()
    for call in (lambda: c.align_correspondences_device(1, 10, 3, 1, 10, 3, 1, 1, -1), lambda: c.align_correspondences_device(1, 10, 3, 1, 10, 3, 1, 1, 2 ** 31)):
        with pytest.raises(ValueError, match="pairs"):
            call()
    for call in (lambda: c.align_correspondences_device(1, 10, 3, 1, 10, 3, 0, 1, 10), lambda: c.align_correspondences_device(1, 10, 3, 1, 10, 3, 1, 0, 10)):
        with pytest.raises(ValueError, match="index arrays"):
            call()


def test_correspondences_from_match():
    match = {"idx": np.array([4, -1, 2, 0, 3, 1], np.int32), "mutual": np.array([1, 0, 0, 1, 1, 1], np.uint8),
             "d": np.array([1.0, np.nan, 1.0, 4.0, 9.0, 1.0]), "d2": np.array([4.0, np.nan, 2.0, 4.0, 16.0, np.inf])}
    ca, cb = api.correspondences_from_match(match)
    assert ca.dtype == cb.dtype == np.int32 and list(ca) == [0, 3, 4, 5] and list(cb) == [4, 0, 3, 1]
    ca, cb = api.correspondences_from_match(match, mutual_only=False)
    assert list(ca) == [0, 2, 3, 4, 5] and list(cb) == [4, 2, 0, 3, 1]
    # sqrt(d / d2): 0.5, -, 0.707, 1.0, 0.75, 0 (no second-best: passes)
    ca, cb = api.correspondences_from_match(match, mutual_only=False, max_ratio=0.75)
    assert list(ca) == [0, 2, 4, 5] and list(cb) == [4, 2, 3, 1]
    ca, cb = api.correspondences_from_match(match, max_ratio=0.6)
    assert list(ca) == [0, 5]
    with pytest.raises(ValueError, match="mutual"):
        api.correspondences_from_match({"idx": match["idx"]})
    with pytest.raises(ValueError, match="max_ratio"):
        api.correspondences_from_match({"idx": match["idx"]}, mutual_only=False, max_ratio=0.8)
    ca, cb = api.correspondences_from_match({"idx": np.zeros(0, np.int32)}, mutual_only=False)
    assert len(ca) == len(cb) == 0
