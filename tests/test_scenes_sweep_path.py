"""scenes.lidar_sweep_path, the sweep of a sensor carried along a sampled path: on a constant twist it is lidar_sweep_moving bit for bit, and
end to end (generator, the path rule of include/dcreg.h in numpy, a first-point voxel, the oracle's registration) a sweep deskewed along its
path registers onto the floor of a static sweep where a constant twist between the same end poses does not.  No device needed."""
import numpy as np

import helpers as h
from dcreg_amd import api, scenes
from oracle import pyoracle as po
from test_api_deskew_args import exp_ref
from test_api_deskew_path_args import deskew_path_ref, inv
from test_gpu_deskew import deskew_ref

PERIOD = 0.1
FACTOR = 3.96          # half the ratio measured in rotation between the constant-twist and the path run (7.93), and not below 2
MOUNT = h.pose6d_matrix(0.3, 0.0, 0.2, 0.0, np.radians(10.0), 0.0)          # sensor on the body: 0.3 m forward, 0.2 m up, pitched 10 deg


def turn_in_scene(T_sensor_ref, alpha=30.0, v0=10.0, dec=8.0, rate=400.0):
    """the motion of the end-to-end tests: yaw accelerating from 0 at alpha rad/s^2, 10 m/s decelerating at 8 m/s^2, placed so that the
    SENSOR is at T_sensor_ref at mid-sweep -> (body_poses_at, knot stamps at `rate` Hz over the sweep, knot poses [K, 4, 4])"""
    Rm, tm = scenes.turn_in_path(np.eye(4), alpha, v0, dec)(np.array([0.5 * PERIOD]))
    mid = np.eye(4)
    mid[:3, :3], mid[:3, 3] = Rm[0], tm[0]
    at = scenes.turn_in_path(T_sensor_ref @ inv(MOUNT) @ inv(mid), alpha, v0, dec)
    st = np.arange(int(round(PERIOD * rate)) + 1) / rate
    R, t = at(st)
    P = np.tile(np.eye(4), (len(st), 1, 1))
    P[:, :3, :3], P[:, :3, 3] = R, t
    return at, st, P


def test_on_a_constant_twist_it_is_lidar_sweep_moving_bit_for_bit():
    tgt, _ = h.scene_parkinglot()
    gt = h.pose6d_matrix(**h.PK01_GT)
    M = exp_ref(np.array([0.002, -0.001, 0.052, 1.0, 0.05, 0.01]))
    xi = api.se3_log(M)

    def poses_at(s):                   # pose_begin Exp(s / period Log(motion)), the way lidar_sweep_moving evaluates it
        R, t = scenes._se3_exp_many(np.outer(s / PERIOD, xi))
        return gt[:3, :3][None] @ R, (gt[:3, :3] @ t.T + gt[:3, 3][:, None]).T

    for ref, seed in ((0.5, 5), (0.0, 6), (1.0, 7)):
        want, T_want = h.lidar_sweep_moving(tgt, gt, M, PERIOD, ref, rings=32, cols=1024, seed=seed)
        got, T_got = h.lidar_sweep_path(tgt, poses_at, np.eye(4), PERIOD, ref * PERIOD, rings=32, cols=1024, seed=seed)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.isfinite(got[:, 0]).sum() > 5000
        assert np.array_equal(T_got, T_want)


def test_the_returned_pose_is_the_body_pose_times_the_extrinsic():
    tgt, _ = h.scene_parkinglot()
    at, st, P = turn_in_scene(h.pose6d_matrix(**h.PK01_GT))
    for t_ref in (0.0, 0.0123, 0.05, 0.1):
        _, T = h.lidar_sweep_path(tgt, at, MOUNT, PERIOD, t_ref, rings=8, cols=256, seed=1)
        R, t = at(np.array([t_ref]))
        B = np.eye(4)
        B[:3, :3], B[:3, 3] = R[0], t[0]
        assert np.allclose(T, B @ MOUNT, rtol=0, atol=1e-12)
    _, T = h.lidar_sweep_path(tgt, at, MOUNT, PERIOD, 0.05, rings=8, cols=256, seed=1)
    assert np.allclose(T, h.pose6d_matrix(**h.PK01_GT), rtol=0, atol=1e-9)


def voxel_first(xyz, leaf):
    """the first point of every occupied voxel, in input order (finite points only)"""
    xyz = xyz[np.all(np.isfinite(xyz), 1)]
    _, i = np.unique(np.floor(xyz.astype(np.float64) / leaf).astype(np.int64), axis=0, return_index=True)
    return xyz[np.sort(i)]


def test_a_sweep_deskewed_along_its_path_registers_onto_the_floor_of_a_static_sweep():
    """The end-to-end scene of tests/test_gpu_deskew_path.py at reduced size (scene_prior_map of 4 M points at extent 120 m cropped to 75 m, a
    64 x 1024 sweep to 70 m, 0.2 m first-point voxel), through deskew_path_ref and the oracle's engine: a 0.1 s sweep while the yaw rate ramps
    from 0 to 3 rad/s and the speed falls from 10 m/s at 8 m/s^2, the sensor mounted 0.3 m forward, 0.2 m up, pitched 10 deg; body poses at
    400 Hz (41 knots) as the table, t_ref mid-sweep.  Four registrations from one start pose, errors at the reference instant, measured:
        raw (stamps ignored)                            15.7 cm / 1.310 deg
        constant twist between the sweep's true end poses   17.6 cm / 0.746 deg
        path, 41 knots                                  5.46 cm / 0.094 deg
        static sweep at the reference pose (the floor)  5.51 cm / 0.090 deg
    Asserted: the path run within 0.5 cm / 0.02 deg of the floor; the constant-twist run at least 3.96 times worse than the path run in
    rotation (half the measured ratio of 7.93; first-order expectation of that run alpha T^2 / 24 = 0.72 deg)."""
    gt = h.pose6d_matrix(**h.PK01_GT)
    tgt, _ = h.scene_prior_map(n_map=4_000_000, n_frame=10, extent=120.0)
    d = tgt[:, :2] - gt[:2, 3].astype(np.float32)
    world = np.ascontiguousarray(tgt[np.einsum("ij,ij->i", d, d) < np.float32(75.0 ** 2)])
    del tgt
    at, st, P = turn_in_scene(gt)
    rec, T_ref = h.lidar_sweep_path(world, at, MOUNT, PERIOD, 0.5 * PERIOD, rings=64, cols=1024, max_range=70.0, seed=1)
    assert np.allclose(T_ref, gt, rtol=0, atol=1e-9)
    static = h.lidar_sweep(world, gt, rings=64, cols=1024, max_range=70.0, seed=1)
    S0, S1 = P[0] @ MOUNT, P[-1] @ MOUNT                       # the sweep's true end poses of the SENSOR: what a constant twist can be given
    clouds = {"raw": rec[:, :3],
              "constant twist": deskew_ref(rec, 3, "f32", 1.0, inv(S0) @ S1, (0.0, PERIOD), 0.5),
              "path": deskew_path_ref(rec, 3, "f32", 1.0, st, P, 0.5 * PERIOD, MOUNT),
              "static": static}
    tree = po.KdTree(world)
    cfg = po.default_config(search_radius=1.0, max_iterations=30, thresh_rot=1e-6, thresh_trans=1e-4, use_weight_derivative=1, gt=gt.reshape(16))
    T0 = gt @ h.pose6d_matrix(0.1, -0.05, 0.02, 0.0, 0.0, 0.01)
    errs = {}
    for name, cloud in clouds.items():
        res, _ = po.icp_run(tree, voxel_first(cloud, 0.2), T0, "Ours", cfg)
        T = np.eye(4)
        T[:3, :3] = np.array(res.R[:]).reshape(3, 3)
        T[:3, 3] = res.t[:]
        errs[name] = po.pose_error(gt, T)
    print("path deskew end to end on the CPU (trans m, rot deg):", errs)
    fl, pa, ct = errs["static"], errs["path"], errs["constant twist"]
    assert pa[0] <= fl[0] + 0.005 and pa[1] <= fl[1] + 0.02, errs
    assert ct[1] >= FACTOR * pa[1], errs

