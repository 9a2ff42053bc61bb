"""The path deskew without a device: `deskew_path_ref`, include/dcreg.h's rule for dcreg_deskew_path* typed out in numpy (the reference of
tests/test_gpu_deskew_path.py), checked against another grouping of the same product, against the constant-twist rule it contains and for
continuity across a knot; the arguments the path methods of Context refuse before anything reaches the library; SweepPath against the header.

The bound used throughout, max(1 float ulp, 1e-9 m): the chain is about 60 double operations on magnitudes of at most |p| + the path's extent,
so its error is below 60 x 1.1e-16 x 1 km < 1e-11 m; two roundings to float of values that close differ by at most one ulp, and an output
coordinate that happens to lie near zero has an ulp below that error, hence the absolute floor with two decimal orders of margin."""
import ctypes as C

import numpy as np
import pytest

from dcreg_amd import api
from test_api_deskew_args import BAD_R, exp_ref, log_ref, rot
from test_gpu_deskew import deskew_ref, stamps_of


def inv(T):
    o = np.eye(4)
    o[:3, :3] = T[:3, :3].T
    o[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return o


def rel(A, B):
    """A^-1 B with the translation taken as R_A^T (t_B - t_A): poses kilometres from the origin cost no precision"""
    o = np.eye(4)
    o[:3, :3] = A[:3, :3].T @ B[:3, :3]
    o[:3, 3] = A[:3, :3].T @ (B[:3, 3] - A[:3, 3])
    return o


def segment_of(st, s, left=False):
    """k(s) = the number of j in [1, K - 2] with st[j] <= s (left: < s, the segment that ENDS on a knot - only for the continuity check)"""
    return int(np.sum(st[1:-1] < s if left else st[1:-1] <= s))


def deskew_path_ref(rec, column, type, scale, st, P, t_ref, E=None, left=False, one_step=False):
    """the header's rule, literally, for one cloud: st [K] the window's stamps, P [K, 4, 4] its poses, E the extrinsic (None: identity)
    -> [n, 3] float32.  one_step: the same product in another grouping, (B(t_ref) E)^-1 (P_k Exp(u xi_k) E) applied in one step."""
    st, P = np.asarray(st, np.float64), np.asarray(P, np.float64)
    E = np.eye(4) if E is None else np.asarray(E, np.float64)
    K = len(st)
    p = rec[:, :3].astype(np.float64)
    s = stamps_of(rec, column, type, scale)
    fin = np.all(np.isfinite(p), 1) & np.isfinite(s)
    xi = [log_ref(rel(P[k], P[k + 1])) for k in range(K - 1)]
    kr = segment_of(st, t_ref)
    Xr = exp_ref((t_ref - st[kr]) / (st[kr + 1] - st[kr]) * xi[kr])            # B(t_ref) = P_kr Xr
    G = [inv(E) @ (inv(Xr) @ rel(P[kr], P[k])) for k in range(K - 1)]          # E^-1 B(t_ref)^-1 P_k
    out = np.full((len(rec), 3), np.nan, np.float32)
    for stamp in np.unique(s[fin]):
        m = fin & (s == stamp)
        k = segment_of(st, stamp, left)
        X = exp_ref((stamp - st[k]) / (st[k + 1] - st[k]) * xi[k])
        if one_step:
            M = inv(P[kr] @ Xr @ E) @ (P[k] @ X @ E)
            out[m] = (p[m] @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
            continue
        q = p[m] @ E[:3, :3].T + E[:3, 3]
        q = q @ X[:3, :3].T + X[:3, 3]
        out[m] = (q @ G[k][:3, :3].T + G[k][:3, 3]).astype(np.float32)
    return out


def within_bound(a, b):
    """NaN in the same places and |a - b| <= max(1 float ulp, 1e-9 m) everywhere else -> (ok, worst excess over the bound)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False, np.inf
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    bound = np.maximum(np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b))).astype(np.float64), 1e-9)
    ex = np.where(nan, -np.inf, d - bound)
    return bool(np.all(ex <= 0.0)), float(ex.max()) if ex.size else 0.0


def test_the_bound_admits_one_ulp_and_refuses_two():
    b = np.array([[1.5, -40.0, 1e-12], [np.nan, 3.0, 0.0]], np.float32)
    one = np.nextafter(b, np.float32(np.inf))
    assert within_bound(one, b)[0]
    assert not within_bound(np.nextafter(one, np.float32(np.inf)), b)[0]
    two = b.copy()
    two[1, 0] = 1.0
    assert not within_bound(two, b)[0]


def random_path(rng, K, origin=0.0, epoch=1.7e9, span=0.1):
    """K knots over [epoch, epoch + span] at uneven stamps: a random start pose `origin` metres out, then steps of up to 0.05 rad and 0.3 m
    per tenth of the span scaled so that the whole path stays a few metres long"""
    st = epoch + np.sort(rng.uniform(0, span, K))
    st[0], st[-1] = epoch, epoch + span
    P = [exp_ref(np.r_[rng.uniform(-0.3, 0.3, 3), rng.uniform(-1, 1, 3)])]
    P[0][:3, 3] += origin
    for k in range(K - 1):
        P.append(P[-1] @ exp_ref(np.r_[rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.3, 0.3, 3)] * (st[k + 1] - st[k]) / span * K / 2))
    return st, np.array(P)


def random_extrinsic(rng):
    return exp_ref(np.r_[rng.uniform(-1, 1, 3) * 0.5, rng.uniform(-1, 1, 3)])


def f64_records(rng, n, seconds):
    """x y z and an f64 stamp over slots 4, 5 of 6"""
    rec = np.zeros((n, 6), np.float32)
    rec[:, :3] = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    u = np.asarray(seconds, np.float64).view(np.uint64)
    w = rec.view(np.uint32)
    w[:, 4], w[:, 5] = (u & 0xFFFFFFFF).astype(np.uint32), (u >> 32).astype(np.uint32)
    return rec


@pytest.mark.parametrize("K", [2, 3, 21, 41])
@pytest.mark.parametrize("origin", [0.0, 1e4, 1e5], ids=["0 km", "10 km", "100 km"])
@pytest.mark.parametrize("ext", [False, True], ids=["identity", "extrinsic"])
def test_the_rule_agrees_with_another_grouping_of_the_same_product(K, origin, ext):
    rng = np.random.default_rng(1000 * K + int(origin) + ext)
    st, P = random_path(rng, K, origin)
    E = random_extrinsic(rng) if ext else None
    rec = f64_records(rng, 400, 1.7e9 + rng.uniform(-0.01, 0.11, 400))
    t_ref = 1.7e9 + rng.uniform(0, 0.1)
    a = deskew_path_ref(rec, 4, "f64", 1.0, st, P, t_ref, E)
    b = deskew_path_ref(rec, 4, "f64", 1.0, st, P, t_ref, E, one_step=True)
    assert np.all(np.isfinite(a))
    ok, ex = within_bound(a, b)
    assert ok, ex


@pytest.mark.parametrize("ref", [0.0, 0.3, 0.5, 1.0])
@pytest.mark.parametrize("origin", [0.0, 1e5], ids=["0 km", "100 km"])
def test_a_two_knot_path_is_the_constant_twist_rule(ref, origin):
    """identity extrinsic, motion = P_0^-1 P_1, span = the two stamps, ref = (t_ref - s[0]) / (s[1] - s[0]): the new rule contains the old"""
    rng = np.random.default_rng(int(100 * ref) + int(origin))
    st, P = random_path(rng, 2, origin)
    rec = f64_records(rng, 400, 1.7e9 + rng.uniform(-0.01, 0.11, 400))
    rec[::37, 1] = np.nan
    t_ref = st[0] + ref * (st[1] - st[0])
    a = deskew_path_ref(rec, 4, "f64", 1.0, st, P, t_ref)
    b = deskew_ref(rec, 4, "f64", 1.0, rel(P[0], P[1]), (st[0], st[1]), (t_ref - st[0]) / (st[1] - st[0]))
    ok, ex = within_bound(a, b)
    assert ok, ex


@pytest.mark.parametrize("K", [3, 21, 41])
@pytest.mark.parametrize("ext", [False, True], ids=["identity", "extrinsic"])
def test_the_rule_is_continuous_across_a_knot(K, ext):
    """every point stamped on an inner knot: the segment that starts there (u = 0) and the one that ends there (u = 1) give the same point"""
    rng = np.random.default_rng(K + ext)
    st, P = random_path(rng, K, 1e4)
    E = random_extrinsic(rng) if ext else None
    rec = f64_records(rng, 40 * (K - 2), np.repeat(st[1:-1], 40))
    t_ref = 1.7e9 + 0.033
    a = deskew_path_ref(rec, 4, "f64", 1.0, st, P, t_ref, E)
    b = deskew_path_ref(rec, 4, "f64", 1.0, st, P, t_ref, E, left=True)
    ok, ex = within_bound(a, b)
    assert ok, ex


def test_the_path_block_matches_the_header():
    assert [f[0] for f in api.SweepPath._fields_] == ["first_knot", "n_knots", "reserved_", "t_ref", "ext_R", "ext_t"]
    assert C.sizeof(api.SweepPath) == 8 + 4 + 4 + 8 + 8 * 12
    assert api.SweepPath.first_knot.offset == 0 and api.SweepPath.n_knots.offset == 8 and api.SweepPath.t_ref.offset == 16
    assert api.SweepPath.ext_R.offset == 24 and api.SweepPath.ext_t.offset == 96
    assert api.load().dcreg_sizeof(b"dcreg_sweep_path") == C.sizeof(api.SweepPath)
    E = exp_ref(np.array([0.1, -0.2, 0.3, 1.0, 2.0, 3.0]))
    b = api.sweep_path(5, 41, 0.05, E)
    assert (b.first_knot, b.n_knots, b.t_ref) == (5, 41, 0.05)
    assert list(b.ext_R) == list(E[:3, :3].reshape(9)) and list(b.ext_t) == list(E[:3, 3])
    b = api.sweep_path(0, 2, 1.7e9)
    assert list(b.ext_R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(b.ext_t) == [0, 0, 0]


# ---- refusals: every rule raises ValueError in every wrapper (and in sweep_path where it can tell)
REC = np.zeros((10, 6), np.float32)
ST = np.array([0.0, 0.025, 0.05, 0.075, 0.1])
POSES = np.array([exp_ref(np.array([0, 0, 0.01 * k, 0.25 * k, 0, 0])) for k in range(5)])


def _field(column=3, type=0, scale=1.0):
    f = api.TimeField()
    f.column, f.type, f.scale = column, type, scale
    return f


def _block(first=0, n=5, t_ref=0.05, R=np.eye(3), t=np.zeros(3)):
    b = api.SweepPath()
    b.first_knot, b.n_knots, b.t_ref = first, n, t_ref
    b.ext_R[:] = list(np.asarray(R, np.float64).reshape(9))
    b.ext_t[:] = list(np.asarray(t, np.float64).reshape(3))
    return b


def _calls(f, st, P, b, rec=REC, leaf=None):
    c = object.__new__(api.Context)          # no device: the checks come first
    n, stride = rec.shape
    return [lambda: c.deskew_path([rec], f, st, P, [b], leaf), lambda: c.deskew_path((rec, [0, n]), f, st, P, b, leaf),
            lambda: c.deskew_path_device(0, [0, n], stride, f, st, P, [b], 0, n, leaf), lambda: c.set_source_deskew_path(rec, f, st, P, b, leaf),
            lambda: c.set_source_deskew_path_device(0, n, stride, f, st, P, b, leaf)]


def _all_raise(match, f=None, st=ST, P=POSES, b=None, **kw):
    for call in _calls(f or _field(), st, P, b or _block(), **kw):
        with pytest.raises(ValueError, match=match):
            call()


def _poses_with(k, R=None, t=None):
    P = POSES.copy()
    if R is not None:
        P[k, :3, :3] = R
    if t is not None:
        P[k, :3, 3] = t
    return P


@pytest.mark.parametrize("first,n", [(0, 6), (1, 5), (5, 2), (-1, 3), (0, 1), (2, 0), (0, -2)],
                         ids=["too long", "past the end", "from the end", "negative start", "one knot", "no knot", "negative count"])
def test_windows_outside_the_table_or_below_two_knots_are_refused(first, n):
    _all_raise("window|knots", b=_block(first, n, 0.05))
    if first < 0 or n < 2:
        with pytest.raises(ValueError, match="knots"):
            api.sweep_path(first, n, 0.05)


def test_a_table_whose_stamps_and_poses_differ_in_length_is_refused():
    _all_raise("knot table", st=ST[:4])
    _all_raise("knot table", P=POSES[:, :3, :3])


@pytest.mark.parametrize("k,v", [(2, 0.025), (2, 0.02), (1, np.nan), (4, np.inf), (0, -np.inf)],
                         ids=["equal", "decreasing", "nan", "inf", "-inf"])
def test_stamps_that_are_not_finite_and_strictly_increasing_are_refused(k, v):
    st = ST.copy()
    st[k] = v
    _all_raise("stamps|t_ref", st=st)


def test_only_the_knots_inside_a_window_are_checked():
    st, P = ST.copy(), POSES.copy()
    st[0], P[4, :3, :3] = np.nan, np.diag([1.0, 1.0, -1.0])
    for call in _calls(_field(), st, P, _block(1, 3, 0.05)):
        with pytest.raises(AttributeError):          # past the checks: this Context has no library
            call()


@pytest.mark.parametrize("name", sorted(BAD_R))
def test_knot_poses_and_extrinsics_that_are_not_rotations_are_refused(name):
    """as a knot pose, as the extrinsic, and (the quarter turn and beyond, which are rotations) as the rotation of one segment"""
    R = BAD_R[name]
    if "deg" in name:
        _all_raise("segment rotates", P=_poses_with(2, R=POSES[1, :3, :3] @ R))
        api.sweep_path(0, 5, 0.05, np.block([[R, np.zeros((3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]]))      # an extrinsic may turn
        return
    _all_raise("rotation|finite", P=_poses_with(2, R=R))
    _all_raise("rotation|finite", b=_block(R=R))
    E = np.eye(4)
    E[:3, :3] = R
    with pytest.raises(ValueError, match="rotation|finite"):
        api.sweep_path(0, 5, 0.05, E)


def test_non_finite_translations_and_a_segment_just_below_a_quarter_turn():
    _all_raise("finite", P=_poses_with(3, t=[0, np.inf, 0]))
    _all_raise("finite", b=_block(t=[np.nan, 0, 0]))
    P = _poses_with(2, R=POSES[1, :3, :3] @ rot(89.9))
    P[3:, :3, :3] = P[2, :3, :3]
    for call in _calls(_field(), ST, P, _block()):
        with pytest.raises(AttributeError):          # accepted: past the checks
            call()


@pytest.mark.parametrize("t_ref", [-1e-9, 0.1 + 1e-9, np.nan, np.inf, -np.inf])
def test_reference_instants_outside_the_window_are_refused(t_ref):
    _all_raise("t_ref", b=_block(t_ref=t_ref))
    _all_raise("t_ref", b=_block(1, 3, 0.0 if not t_ref > 0 else 0.1))          # inside the table, outside the block's window
    if not np.isfinite(t_ref):
        with pytest.raises(ValueError, match="t_ref"):
            api.sweep_path(0, 5, t_ref)


@pytest.mark.parametrize("column,type,stride", [(2, 0, 6), (6, 0, 6), (5, 1, 6), (5, 3, 6), (3, 0, 3)],
                         ids=["2", "=stride", "f64 last slot", "u64 last slot", "stride 3"])
def test_the_time_field_refusals_hold(column, type, stride):
    _all_raise("column", f=_field(column, type), rec=np.zeros((10, stride), np.float32))


def test_unknown_types_bad_scales_and_bad_leaves_are_refused():
    _all_raise("type", f=_field(type=7))
    _all_raise("scale", f=_field(scale=0.0))
    _all_raise("leaf", leaf=[0.1, -0.1, 0.1])


def test_one_block_per_cloud():
    c = object.__new__(api.Context)
    with pytest.raises(ValueError, match="block"):
        c.deskew_path([REC, REC, REC], _field(), ST, POSES, [_block(), _block()])
    with pytest.raises(ValueError, match="sweep_path"):
        c.deskew_path([REC], _field(), ST, POSES, [api.SweepMotion()])
    with pytest.raises(ValueError, match="time_field"):
        c.deskew_path([REC], _block(), ST, POSES, [_block()])
