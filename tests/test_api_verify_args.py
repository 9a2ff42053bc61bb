"""Arguments the verify methods of Context check before anything reaches the library (no device needed), the structs against the header
and dcreg_sizeof, the default parameters and the refusals of the C-ABI that need no context."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api

CLOUD = np.zeros((10, 3), np.float32)
POSES = np.stack([np.eye(4)] * 3)


def test_the_structs_match_the_header_and_the_library():
    L = api.load()
    assert [f[0] for f in api.VerifyParams._fields_] == ["inlier_distance", "point_stride", "rank_by", "detail_pose", "reserved_"]
    assert [f[0] for f in api.VerifyRecord._fields_] == ["pose", "count", "cost", "score", "fitness", "rmse"]
    assert [f[0] for f in api.VerifyInfo._fields_] == ["n_poses", "n_points", "n_scored", "best_pose", "reserved_"]
    assert (C.sizeof(api.VerifyParams), C.sizeof(api.VerifyRecord), C.sizeof(api.VerifyInfo)) == (40, 40, 48)
    P, R, I = api.VerifyParams, api.VerifyRecord, api.VerifyInfo
    assert (P.inlier_distance.offset, P.point_stride.offset, P.rank_by.offset, P.detail_pose.offset, P.reserved_.offset) == (0, 8, 16, 20, 24)
    assert (R.pose.offset, R.count.offset, R.cost.offset, R.score.offset, R.fitness.offset, R.rmse.offset) == (0, 4, 8, 16, 24, 32)
    assert (I.n_poses.offset, I.n_points.offset, I.n_scored.offset, I.best_pose.offset, I.reserved_.offset) == (0, 8, 16, 24, 32)
    for name, cls in (("dcreg_verify_params", P), ("dcreg_verify_record", R), ("dcreg_verify_info", I)):
        assert L.dcreg_sizeof(name.encode()) == C.sizeof(cls), name
        assert api._STRUCTS[name] is cls
    for name in ("dcreg_default_verify_params", "dcreg_verify_poses", "dcreg_verify_poses_cloud", "dcreg_verify_poses_cloud_device"):
        assert name in api.EXPORTS and hasattr(L, name), name
    # the T of an align or consensus record leads it, and a record is 22 doubles: pose_stride_doubles = 22 reads an array of them in place
    assert api.AlignRecord.T.offset == api.ConsensusRecord.T.offset == 0
    assert C.sizeof(api.AlignRecord) == C.sizeof(api.ConsensusRecord) == 8 * api.VERIFY_RECORD_STRIDE


def test_the_default_parameters():
    p = api.VerifyParams()
    p.inlier_distance, p.point_stride, p.rank_by, p.detail_pose, p.reserved_[1] = 9.0, 5, 1, 4, 4.0
    assert api.load().dcreg_default_verify_params(C.byref(p)) == api.OK
    assert (p.inlier_distance, p.point_stride, p.rank_by, p.detail_pose, list(p.reserved_)) == (0.5, 1, 0, -1, [0.0, 0.0])
    assert bytes(p) == bytes(api.verify_params())
    assert api.load().dcreg_default_verify_params(None) == -1
    q = api.verify_params(inlier_distance=1e-9, point_stride=2 ** 40, rank_by=1, detail_pose=65534)
    assert (q.inlier_distance, q.point_stride, q.rank_by, q.detail_pose) == (1e-9, 2 ** 40, 1, 65534)


def test_the_c_abi_refuses_a_null_context():
    L = api.load()
    p = api.verify_params(detail_pose=0)
    recs = (api.VerifyRecord * 3)()
    recs[0].count = 7
    info = api.VerifyInfo()
    info.n_poses = 5
    mask = np.full(10, 3, np.uint8)
    nn = np.full(10, 7, np.int32)
    tail = (POSES.ctypes.data, 3, 16, C.byref(p), recs, mask.ctypes.data, nn.ctypes.data, C.byref(info))
    assert L.dcreg_verify_poses(None, *tail) == -1
    assert L.dcreg_verify_poses_cloud(None, CLOUD.ctypes.data, 10, 3, *tail) == -1
    assert L.dcreg_verify_poses_cloud_device(None, CLOUD.ctypes.data, 10, 3, *tail) == -1
    assert info.n_poses == 5 and recs[0].count == 7 and (mask == 3).all() and (nn == 7).all()


def _ctx():
    return object.__new__(api.Context)          # no device: the checks come first


def _block(**kw):
    p = api.verify_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [("inlier_distance", 0.0), ("inlier_distance", -0.5), ("inlier_distance", np.nan), ("inlier_distance", np.inf), ("point_stride", 0),
              ("point_stride", -3), ("rank_by", -1), ("rank_by", 2), ("detail_pose", -2), ("detail_pose", 3), ("detail_pose", 70000)]


@pytest.mark.parametrize("field,value", BAD_PARAMS, ids=["%s=%s" % b for b in BAD_PARAMS])
def test_bad_parameters_are_refused_everywhere(field, value):
    if (field, value) not in (("detail_pose", 3), ("detail_pose", 70000)):       # (against the poses: only a call knows how many there are)
        with pytest.raises(ValueError, match=field):
            api.verify_params(**{field: value})
    p = _block(**{field: value})
    c = _ctx()
    for call in (lambda: c.verify_poses(POSES, p), lambda: c.verify_poses(POSES, p, cloud=CLOUD), lambda: c.verify_poses_device(1, 10, 3, POSES, p)):
        with pytest.raises(ValueError, match=field):
            call()


def bad_pose(k, what):
    Ts = POSES.copy()
    if what == "nan":
        Ts[k, 1, 3] = np.nan
    elif what == "inf":
        Ts[k, 2, 0] = np.inf
    elif what == "scaled":
        Ts[k, :3, :3] *= 1.0 + 2e-6
    elif what == "mirror":
        Ts[k, 0, 0] = -1.0
    return Ts


@pytest.mark.parametrize("what", ["nan", "inf", "scaled", "mirror"])
def test_a_bad_pose_is_refused_by_its_index(what):
    c = _ctx()
    for k in (0, 2):
        Ts = bad_pose(k, what)
        for call in (lambda: c.verify_poses(Ts), lambda: c.verify_poses(Ts, cloud=CLOUD), lambda: c.verify_poses_device(1, 10, 3, Ts),
                     lambda: c.verify_poses([{"T": T} for T in Ts])):
            with pytest.raises(ValueError, match="pose %d" % k):
                call()
    ok = POSES.copy()
    ok[:, 3, :] = np.nan                                   # the bottom row is ignored
    ok[1, :3, :3] *= 1.0 + 1e-7                            # inside the rotation rule's 1e-6
    T16, n = api._verify_poses(ok, api.verify_params(), "x")
    assert n == 3 and T16.shape == (3, 16)


def test_poses_clouds_and_counts_are_checked():
    c = _ctx()
    for Ts in (np.eye(4), np.zeros((3, 3, 4)), np.zeros((2, 16))):
        with pytest.raises(ValueError, match=r"\[P, 4, 4\]"):
            c.verify_poses(Ts)
    with pytest.raises(ValueError, match="65535 poses"):
        c.verify_poses(np.broadcast_to(np.eye(4), (65536, 4, 4)))
    with pytest.raises(ValueError, match="verify_params"):
        c.verify_poses(POSES, api.align_params())
    with pytest.raises(ValueError, match="want_detail"):
        c.verify_poses(POSES, want_detail=True)
    for cloud in (np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float64), np.zeros(30, np.float32)):
        with pytest.raises(ValueError, match="float32"):
            c.verify_poses(POSES, cloud=cloud)
    for call in (lambda: c.verify_poses_device(1, 10, 2, POSES), lambda: c.verify_poses_device(1, 10, 0, POSES)):
        with pytest.raises(ValueError, match="stride"):
            call()
    for call in (lambda: c.verify_poses_device(1, -1, 3, POSES), lambda: c.verify_poses_device(1, 2 ** 31, 3, POSES)):
        with pytest.raises(ValueError, match="points"):
            call()
    with pytest.raises(ValueError, match="cloud pointer"):
        c.verify_poses_device(0, 10, 3, POSES)
