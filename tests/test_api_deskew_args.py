"""Arguments the deskew methods of Context check before anything reaches the library (no device needed), the parameter blocks against the
header, and the SE(3) pair the deskew is defined by: a numpy Exp / Log written out here from include/dcreg.h's formulas (the reference of
tests/test_gpu_deskew.py) round-trips, composes along one twist, and agrees with api.se3_exp / se3_log and constant_velocity_motion."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_ref(xi):
    """include/dcreg.h: R = I + A W + B W^2, t = (I + B W + C W^2) v; the series through theta^4 below theta = 1e-3 -> 4x4"""
    xi = np.asarray(xi, np.float64)
    w, v = xi[:3], xi[3:]
    th = np.sqrt(w @ w)
    if th < 1e-3:
        A, B, Cc = 1 - th ** 2 / 6 + th ** 4 / 120, 0.5 - th ** 2 / 24 + th ** 4 / 720, 1 / 6 - th ** 2 / 120 + th ** 4 / 5040
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    W = hat(w)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * W @ W
    T[:3, 3] = (np.eye(3) + B * W + Cc * W @ W) @ v
    return T


def log_ref(T):
    """the inverse of exp_ref for rotations below pi: angle-axis of R, then v = V^-1 t (V inverted numerically)"""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1.0, 1.0))
    vee = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    w = vee if th < 1e-8 else vee * th / np.sin(th)
    th = np.sqrt(w @ w)
    if th < 1e-3:
        B, Cc = 0.5 - th ** 2 / 24 + th ** 4 / 720, 1 / 6 - th ** 2 / 120 + th ** 4 / 5040
    else:
        B, Cc = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    W = hat(w)
    V = np.eye(3) + B * W + Cc * W @ W
    return np.r_[w, np.linalg.solve(V, T[:3, 3])]


TWISTS = [np.array(x, np.float64) for x in ([0, 0, 0, 1.0, 0.2, 0.0], [0.01, -0.02, 0.05, 0, 0, 0], [2e-4, -1e-4, 3e-4, 0.3, 0.1, 0.0],
                                            [0.002, -0.001, 0.052, 1.0, 0.05, 0.01], [0.4, 0.9, -0.3, -2.0, 5.0, 1.0], [0, 0, 0, 0, 0, 0])]


@pytest.mark.parametrize("k", range(len(TWISTS)))
def test_exp_and_log_round_trip(k):
    xi = TWISTS[k]
    assert np.allclose(log_ref(exp_ref(xi)), xi, rtol=0, atol=1e-12)
    assert np.allclose(api.se3_log(exp_ref(xi)), xi, rtol=0, atol=1e-12)
    assert np.allclose(api.se3_exp(xi), exp_ref(xi), rtol=0, atol=1e-14)


@pytest.mark.parametrize("k", range(len(TWISTS)))
@pytest.mark.parametrize("a,b", [(0.3, 0.45), (-0.5, 0.5), (1.0, -0.25), (1e-4, 2.0)])
def test_exp_of_one_twist_composes(k, a, b):
    xi = TWISTS[k]
    assert np.allclose(exp_ref(a * xi) @ exp_ref(b * xi), exp_ref((a + b) * xi), rtol=0, atol=1e-12)


def test_constant_velocity_motion_returns_the_motion_between_two_poses():
    rng = np.random.default_rng(4)
    for xi in TWISTS[:5]:
        T_prev = exp_ref(rng.uniform(-1, 1, 6) * [0.5, 0.5, 3, 50, 50, 5])
        M = exp_ref(xi)
        assert np.allclose(api.constant_velocity_motion(T_prev, T_prev @ M), M, rtol=0, atol=1e-9)
        assert np.allclose(api.constant_velocity_motion(T_prev, T_prev @ M, 0.5), exp_ref(0.5 * log_ref(M)), rtol=0, atol=1e-9)


def test_the_parameter_blocks_match_the_header():
    assert [f[0] for f in api.TimeField._fields_] == ["column", "type", "scale"]
    assert [f[0] for f in api.SweepMotion._fields_] == ["R", "t", "t_begin", "t_end", "ref", "span_from_data", "reserved_"]
    assert [f[0] for f in api.DeskewInfo._fields_] == ["n_in", "n_finite", "n_outside", "t_min", "t_max"]
    assert C.sizeof(api.TimeField) == 16 and C.sizeof(api.SweepMotion) == 8 * 15 + 8 and C.sizeof(api.DeskewInfo) == 40
    assert api.TIME_TYPES == {"f32": 0, "f64": 1, "u32": 2, "u64": 3}
    f = api.time_field(5, "u64", 1e-9)
    assert (f.column, f.type, f.scale) == (5, 3, 1e-9)
    R = exp_ref(TWISTS[3])[:3, :3]
    m = api.sweep_motion(R, [1, 2, 3], (0.25, 0.35), 1.0)
    assert list(m.R) == list(R.reshape(9)) and list(m.t) == [1, 2, 3] and (m.t_begin, m.t_end, m.ref, m.span_from_data) == (0.25, 0.35, 1.0, 0)
    m = api.sweep_motion(np.eye(3), np.zeros(3))
    assert m.span_from_data == 1 and m.ref == 0.5


# ---- refusals: every rule raises ValueError in every wrapper (and in the block's own constructor where it can tell)
REC = np.zeros((10, 6), np.float32)
GOOD_F = dict(column=3, type=0, scale=1.0)
GOOD_M = dict(R=np.eye(3), t=np.zeros(3), span=(0.0, 0.1), ref=0.5)


def _field(column=3, type=0, scale=1.0):
    f = api.TimeField()
    f.column, f.type, f.scale = column, type, scale
    return f


def _motion(R=np.eye(3), t=np.zeros(3), span=(0.0, 0.1), ref=0.5):
    m = api.SweepMotion()
    m.R[:] = list(np.asarray(R, np.float64).reshape(9))
    m.t[:] = list(np.asarray(t, np.float64).reshape(3))
    m.span_from_data = 1 if span is None else 0
    m.t_begin, m.t_end = (0.0, 0.0) if span is None else span
    m.ref = ref
    return m


def _calls(f, m, rec=REC, leaf=None):
    c = object.__new__(api.Context)          # no device: the checks come first
    n, stride = rec.shape
    return [lambda: c.deskew([rec], f, [m], leaf), lambda: c.deskew((rec, [0, n]), f, m, leaf),
            lambda: c.deskew_device(0, [0, n], stride, f, [m], 0, n, leaf), lambda: c.set_source_deskew(rec, f, m, leaf),
            lambda: c.set_source_deskew_device(0, n, stride, f, m, leaf)]


def _all_raise(f, m, match, **kw):
    for call in _calls(f, m, **kw):
        with pytest.raises(ValueError, match=match):
            call()


def rot(deg, axis=(0, 0, 1)):
    a = np.asarray(axis, np.float64)
    return exp_ref(np.r_[np.radians(deg) * a / np.linalg.norm(a), 0, 0, 0])[:3, :3]


@pytest.mark.parametrize("span", [(0.2, 0.1), (np.nan, 0.1), (0.0, np.inf), (-np.inf, 0.0)], ids=["reversed", "nan", "inf", "-inf"])
def test_spans_that_are_not_finite_and_ordered_are_refused(span):
    _all_raise(_field(), _motion(span=span), "span")
    with pytest.raises(ValueError, match="span"):
        api.sweep_motion(np.eye(3), np.zeros(3), span)


@pytest.mark.parametrize("ref", [-0.01, 1.01, np.nan, np.inf])
def test_reference_instants_outside_the_span_are_refused(ref):
    _all_raise(_field(), _motion(ref=ref), "ref")
    with pytest.raises(ValueError, match="ref"):
        api.sweep_motion(np.eye(3), np.zeros(3), None, ref)


BAD_R = {"scaled": 1.01 * np.eye(3), "sheared": np.eye(3) + np.diag([0, 2e-6, 0]), "reflection": np.diag([1.0, 1.0, -1.0]),
         "nan": np.full((3, 3), np.nan), "90 deg": rot(90.0), "120 deg": rot(120.0, (1, 1, 0)), "180 deg": rot(180.0)}


@pytest.mark.parametrize("name", sorted(BAD_R))
def test_motions_that_are_not_small_rotations_are_refused(name):
    _all_raise(_field(), _motion(R=BAD_R[name]), "rotat|finite")
    with pytest.raises(ValueError, match="rotat|finite"):
        api.sweep_motion(BAD_R[name], np.zeros(3))


def test_a_rotation_just_below_a_quarter_turn_and_an_infinite_translation():
    api.sweep_motion(rot(89.9), np.zeros(3))
    _all_raise(_field(), _motion(t=[0, np.inf, 0]), "finite")


@pytest.mark.parametrize("column,type,stride", [(2, 0, 6), (0, 0, 6), (6, 0, 6), (7, 2, 6), (5, 1, 6), (5, 3, 6), (3, 1, 4), (3, 0, 3)],
                         ids=["2", "0", "=stride", ">stride", "f64 last slot", "u64 last slot", "f64 stride 4", "stride 3"])
def test_columns_outside_the_record_are_refused(column, type, stride):
    rec = np.zeros((10, stride), np.float32)
    _all_raise(_field(column, type), _motion(), "column", rec=rec)


@pytest.mark.parametrize("type", [-1, 4, 99])
def test_unknown_types_are_refused(type):
    _all_raise(_field(type=type), _motion(), "type")
    with pytest.raises(ValueError, match="type"):
        api.time_field(3, "f16")


@pytest.mark.parametrize("scale", [0.0, -1e-9, np.nan, np.inf])
def test_scales_that_are_not_finite_and_positive_are_refused(scale):
    _all_raise(_field(scale=scale), _motion(), "scale")
    with pytest.raises(ValueError, match="scale"):
        api.time_field(3, "f32", scale)


@pytest.mark.parametrize("leaf", [0.0, np.nan, [0.1, -0.1, 0.1]])
def test_the_voxel_pass_refusals_hold_with_a_deskew(leaf):
    _all_raise(_field(), _motion(), "leaf", leaf=leaf)


def test_one_motion_per_cloud():
    c = object.__new__(api.Context)
    with pytest.raises(ValueError, match="motion"):
        c.deskew([REC, REC, REC], _field(), [_motion(), _motion()])
    with pytest.raises(ValueError, match="time_field"):
        c.deskew([REC], _motion(), [_motion()])
