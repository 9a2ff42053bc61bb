"""Clouds and poses of the benchmark workloads: the reference's simulated-cylinder fixture (its own data file), seeded synthetic
scenes of the BASELINE configs (cylinder + floor, corridor, ground plane + poles, the PK01 parking-lot stand-in) and minimal PCD I/O.
Used by bench.py, the Monte-Carlo driver, scripts/ and the tests."""
import os

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
# DCReg/dataset/icp_results/target_clouds.pcd of the reference (7562 points; its simulated experiment uses it as source AND target)
FIXTURE_PCD = os.path.join(DATA, "cylinder_7562.pcd")


def read_pcd_xyz(path):
    """Minimal PCD v0.7 reader (binary / ascii, float32 fields) -> float32 [n,3]."""
    with open(path, "rb") as f:
        fields, sizes, counts, npts, data_kind = [], [], [], 0, None
        while True:
            line = f.readline().decode("ascii", "replace").strip()
            if line.startswith("FIELDS"):
                fields = line.split()[1:]
            elif line.startswith("SIZE"):
                sizes = [int(v) for v in line.split()[1:]]
            elif line.startswith("COUNT"):
                counts = [int(v) for v in line.split()[1:]]
            elif line.startswith("POINTS"):
                npts = int(line.split()[1])
            elif line.startswith("DATA"):
                data_kind = line.split()[1]
                break
        if not counts:
            counts = [1] * len(fields)
        rec = sum(s * c for s, c in zip(sizes, counts))
        if data_kind == "binary":
            raw = np.frombuffer(f.read(rec * npts), dtype=np.uint8).reshape(npts, rec)
            off = {}
            o = 0
            for name, s, c in zip(fields, sizes, counts):
                off[name] = o
                o += s * c
            cols = [raw[:, off[k]:off[k] + 4].copy().view(np.float32)[:, 0] for k in ("x", "y", "z")]
            return np.stack(cols, axis=1).astype(np.float32)
        txt = np.loadtxt(f, dtype=np.float64).reshape(npts, -1)
        ix = [fields.index(k) for k in ("x", "y", "z")]
        return txt[:, ix].astype(np.float32)


def cylinder_cloud():
    return read_pcd_xyz(FIXTURE_PCD)


def deg2rad(d):
    return d * np.pi / 180.0


# initial poses of the two committed trace families (complete_log.txt of each run)
RELEASE_INIT = dict(x=0.01, y=0.01, z=0.01, roll=0.0, pitch=0.0, yaw=0.0)
PAPER_INIT = dict(x=0.2, y=0.8, z=0.5, roll=deg2rad(0.1), pitch=deg2rad(0.1), yaw=deg2rad(2.0))


def pose6d_matrix(x, y, z, roll, pitch, yaw):
    """T * Rz(yaw) * Ry(pitch) * Rx(roll)  (utils.hpp:452-460)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [x, y, z]
    return T


# ------------------------------------------------------------------ synthetic scenes (seeded)
def scene_cylinder(n, seed=0, radius=40.0, height=20.0, noise=0.0):
    """Cylinder wall + floor disk, like the reference's simulated scene, jittered (no exact ties)."""
    rng = np.random.default_rng(seed)
    n_wall = n // 2
    n_floor = n - n_wall
    th = rng.uniform(0, 2 * np.pi, n_wall)
    z = rng.uniform(0, height, n_wall)
    wall = np.stack([radius * np.cos(th), radius * np.sin(th), z], 1)
    r = radius * np.sqrt(rng.uniform(0, 1, n_floor))
    th2 = rng.uniform(0, 2 * np.pi, n_floor)
    floor = np.stack([r * np.cos(th2), r * np.sin(th2), rng.normal(0, 1e-3, n_floor)], 1)
    pts = np.concatenate([wall, floor], 0)
    if noise > 0:
        pts = pts + rng.normal(0, noise, pts.shape)
    rng.shuffle(pts)
    return pts.astype(np.float32)


def scene_corridor(n, seed=0, length=200.0, width=4.0, height=3.0, noise=0.005):
    """Two walls + floor + ceiling along x: translational degeneracy along the axis."""
    rng = np.random.default_rng(seed)
    per = 2 * (width + height)
    u = rng.uniform(0, per, n)
    x = rng.uniform(-length / 2, length / 2, n)
    y = np.empty(n)
    z = np.empty(n)
    a = u < width                                   # floor
    b = (u >= width) & (u < width + height)         # wall y=+w/2
    c = (u >= width + height) & (u < 2 * width + height)  # ceiling
    d = u >= 2 * width + height                     # wall y=-w/2
    y[a] = u[a] - width / 2; z[a] = 0.0
    y[b] = width / 2; z[b] = u[b] - width
    y[c] = width / 2 - (u[c] - width - height); z[c] = height
    y[d] = -width / 2; z[d] = height - (u[d] - 2 * width - height)
    pts = np.stack([x, y, z], 1) + rng.normal(0, noise, (n, 3))
    return pts.astype(np.float32)


def scene_planes(n, seed=0, extent=60.0, noise=0.01):
    """Ground plane + sparse vertical poles: X-Y-yaw weakly constrained (parking-lot stand-in)."""
    rng = np.random.default_rng(seed)
    n_poles = max(n // 20, 1)
    n_ground = n - n_poles
    g = np.stack([rng.uniform(-extent, extent, n_ground), rng.uniform(-extent, extent, n_ground),
                  np.zeros(n_ground)], 1)
    centers = rng.uniform(-extent, extent, (16, 2))
    k = rng.integers(0, 16, n_poles)
    ang = rng.uniform(0, 2 * np.pi, n_poles)
    p = np.stack([centers[k, 0] + 0.3 * np.cos(ang), centers[k, 1] + 0.3 * np.sin(ang),
                  rng.uniform(0, 4, n_poles)], 1)
    pts = np.concatenate([g, p], 0) + rng.normal(0, noise, (n, 3))
    rng.shuffle(pts)
    return pts.astype(np.float32)


# ------------------------------------------------------------------ PK01 stand-in (BASELINE config 3)
# The reference's parking-lot pair (config/icp_pk01.yaml:13-14: parkinglot_raw_2415_frame.pcd / target_prior_map.pcd) is
# not in the repository (Google-Drive link only, README.md:69).  Stand-in: a planar prior map around the yaml's ground-truth
# position (ground + sparse poles + a few low kerbs: X-Y-yaw weakly constrained, README.md:96) and one LiDAR frame cut out
# of it, expressed in the sensor frame by gt^-1 and perturbed by range noise.  Poses = the yaml's own numbers.
PK01_GT = dict(x=-109.831089, y=-395.052129, z=-1.025780, roll=deg2rad(-2.635654), pitch=deg2rad(-4.141885), yaw=deg2rad(117.972711))
PK01_INIT = dict(x=-109.979288618688, y=-395.174034820224, z=-0.900523132121, roll=deg2rad(-2.650863295637),
                 pitch=deg2rad(-2.836418366839), yaw=deg2rad(120.142832419935))


def scene_parkinglot(n_map=200_000, n_frame=8_000, seed=7, extent=45.0, frame_range=30.0, noise=0.02):
    """-> (target map [n_map,3] float32 in the map frame, source frame [n_frame,3] float32 in the sensor frame)."""
    rng = np.random.default_rng(seed)
    T_gt = pose6d_matrix(**PK01_GT)
    c = T_gt[:3, 3]
    n_pole, n_kerb = n_map // 25, n_map // 50
    n_ground = n_map - n_pole - n_kerb
    # ground: a gently tilted plane through the sensor's footprint
    gx, gy = rng.uniform(-extent, extent, n_ground), rng.uniform(-extent, extent, n_ground)
    ground = np.stack([c[0] + gx, c[1] + gy, c[2] - 1.8 + 0.01 * gx - 0.005 * gy + rng.normal(0, 0.01, n_ground)], 1)
    # lamp poles / tree trunks: 24 thin vertical cylinders
    pc = rng.uniform(-extent * 0.8, extent * 0.8, (24, 2))
    k = rng.integers(0, 24, n_pole)
    ang = rng.uniform(0, 2 * np.pi, n_pole)
    pz = rng.uniform(0, 4.0, n_pole)
    poles = np.stack([c[0] + pc[k, 0] + 0.15 * np.cos(ang), c[1] + pc[k, 1] + 0.15 * np.sin(ang),
                      c[2] - 1.8 + 0.01 * pc[k, 0] - 0.005 * pc[k, 1] + pz], 1)
    # kerbs: 3 low (0.4 m) vertical strips, 12 m long, random heading
    kc = rng.uniform(-extent * 0.7, extent * 0.7, (3, 2))
    kh = rng.uniform(0, np.pi, 3)
    j = rng.integers(0, 3, n_kerb)
    s = rng.uniform(-6, 6, n_kerb)
    kx, ky = kc[j, 0] + s * np.cos(kh[j]), kc[j, 1] + s * np.sin(kh[j])
    kerbs = np.stack([c[0] + kx, c[1] + ky, c[2] - 1.8 + 0.01 * kx - 0.005 * ky + rng.uniform(0, 0.4, n_kerb)], 1)
    tgt = np.concatenate([ground, poles, kerbs], 0) + rng.normal(0, 0.005, (n_map, 3))
    rng.shuffle(tgt)
    tgt = tgt.astype(np.float32)
    # one frame: map points within range of the sensor, in the sensor frame, with range noise
    d = np.linalg.norm(tgt[:, :2].astype(np.float64) - c[:2], axis=1)
    near = np.flatnonzero(d < frame_range)
    sel = rng.choice(near, size=min(n_frame, len(near)), replace=False)
    Rg, tg = T_gt[:3, :3], T_gt[:3, 3]
    body = (tgt[sel].astype(np.float64) - tg) @ Rg          # R^T (p - t)
    body += rng.normal(0, noise, body.shape)
    return tgt, body.astype(np.float32)


def scene_prior_map(n_map=50_000_000, n_frame=8_000, seed=11, extent=350.0, frame_range=30.0, noise=0.02):
    """A LARGE prior map around the PK01 ground-truth position and one LiDAR frame cut out of it - the regime the reference publishes its
    timings in (1 - 10 k-point frames against 53 - 241 M-point prior maps: README tables 6 / 7, results/long_duration experiments/table3_4).
    Map: 2 * extent metres square - tilted, gently undulating ground (~ 93 % of the points), building facades (vertical planes 8 m high,
    ~ 5 %), poles (~ 2 %); at the defaults ~ 100 points per square metre of ground.  Built in float32 blocks (a 50 M-point map is 600 MB;
    no global shuffle - the index sorts the points anyway).  -> (map [n_map,3] float32 in the map frame, frame [n_frame,3] float32 in the
    sensor frame); poses = PK01_GT / PK01_INIT."""
    rng = np.random.default_rng(seed)
    T_gt = pose6d_matrix(**PK01_GT)
    c = T_gt[:3, 3].astype(np.float32)
    n_wall, n_pole = n_map // 20, n_map // 50
    n_ground = n_map - n_wall - n_pole
    tgt = np.empty((n_map, 3), np.float32)
    e = np.float32(extent)

    def height(x, y):           # ground height above c.z - 1.8 at offsets (x, y) from the sensor's footprint
        return np.float32(0.01) * x - np.float32(0.005) * y + np.float32(0.15) * np.sin(x * np.float32(0.05)) * np.cos(y * np.float32(0.04))

    blk = 1 << 22
    for i0 in range(0, n_ground, blk):
        m = min(blk, n_ground - i0)
        gx = (rng.random(m, dtype=np.float32) * 2 - 1) * e
        gy = (rng.random(m, dtype=np.float32) * 2 - 1) * e
        tgt[i0:i0 + m, 0] = c[0] + gx
        tgt[i0:i0 + m, 1] = c[1] + gy
        tgt[i0:i0 + m, 2] = c[2] - np.float32(1.8) + height(gx, gy) + rng.standard_normal(m, dtype=np.float32) * np.float32(0.01)
    # facades: 64 vertical planes per 700 m x 700 m (the count grows with the map's area, so that a larger map is more of the same map and not
    # the same facades with more points on each), 20 - 60 m long, 8 m high, random position / heading (a dozen of them within the frame's range)
    area = max(1.0, (float(extent) / 350.0) ** 2)
    nf = int(round(64 * area))
    fc = ((rng.random((nf, 2), dtype=np.float32) * 2 - 1) * e * np.float32(0.9))
    fc[:12] = (rng.random((12, 2), dtype=np.float32) * 2 - 1) * np.float32(frame_range * 0.9)
    fh = rng.random(nf, dtype=np.float32) * np.float32(np.pi)
    fl = np.float32(20.0) + rng.random(nf, dtype=np.float32) * np.float32(40.0)
    j = rng.integers(0, nf, n_wall)
    sw = (rng.random(n_wall, dtype=np.float32) - np.float32(0.5)) * fl[j]
    wx, wy = fc[j, 0] + sw * np.cos(fh[j]), fc[j, 1] + sw * np.sin(fh[j])
    o = n_ground
    tgt[o:o + n_wall, 0] = c[0] + wx
    tgt[o:o + n_wall, 1] = c[1] + wy
    tgt[o:o + n_wall, 2] = c[2] - np.float32(1.8) + height(wx, wy) + rng.random(n_wall, dtype=np.float32) * np.float32(8.0)
    # poles: 400 thin vertical cylinders per 700 m x 700 m (two dozen within the frame's range)
    npc = int(round(400 * area))
    pc = (rng.random((npc, 2), dtype=np.float32) * 2 - 1) * e * np.float32(0.95)
    pc[:24] = (rng.random((24, 2), dtype=np.float32) * 2 - 1) * np.float32(frame_range * 0.9)
    k = rng.integers(0, npc, n_pole)
    ang = rng.random(n_pole, dtype=np.float32) * np.float32(2 * np.pi)
    o += n_wall
    tgt[o:o + n_pole, 0] = c[0] + pc[k, 0] + np.float32(0.15) * np.cos(ang)
    tgt[o:o + n_pole, 1] = c[1] + pc[k, 1] + np.float32(0.15) * np.sin(ang)
    tgt[o:o + n_pole, 2] = c[2] - np.float32(1.8) + height(pc[k, 0], pc[k, 1]) + rng.random(n_pole, dtype=np.float32) * np.float32(4.0)
    tgt[n_ground:] += rng.standard_normal((n_wall + n_pole, 3), dtype=np.float32) * np.float32(0.005)
    # one frame: map points within range of the sensor, in the sensor frame, with range noise
    dx, dy = tgt[:, 0] - c[0], tgt[:, 1] - c[1]
    near = np.flatnonzero(dx * dx + dy * dy < np.float32(frame_range * frame_range))
    sel = rng.choice(near, size=min(n_frame, len(near)), replace=False)
    Rg, tg = T_gt[:3, :3], T_gt[:3, 3]
    body = (tgt[sel].astype(np.float64) - tg) @ Rg          # R^T (p - t)
    body += rng.normal(0, noise, body.shape)
    return tgt, body.astype(np.float32)


def scene_sparse_map(extent=300.0, spacing=1.4, n_frame=4_000, frame_range=20.0, seed=23, offset=(0.0, 0.0, 0.0), noise=0.02):
    """A SPARSE map for the edges of the window index: jittered grid points about `spacing` metres apart (at the defaults ~ 1.4 m, about 190
    thousand points) on a gently undulating ground 2 * extent metres square, on 40 vertical walls (20 - 50 m long, 6 m high) and
    on 30 poles, and a frame cut out of it by map_frames at the sensor pose (sensor 1.8 m above the ground at the square's centre + offset).
    Every query's 5th neighbour lies a metre or more away, so a window whose box is off by a fraction of a metre at the frame's edge
    changes the neighbours of the queries there.  -> (map [n, 3] float32, frame [m, 3] float32 in the sensor frame, sensor pose 4x4)."""
    rng = np.random.default_rng(seed)
    o = np.asarray(offset, np.float64)
    g = np.arange(-extent, extent + 1e-9, spacing)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    gx = gx.ravel() + rng.uniform(-0.3, 0.3, gx.size) * spacing
    gy = gy.ravel() + rng.uniform(-0.3, 0.3, gy.size) * spacing

    def height(x, y):
        return 0.01 * x - 0.004 * y + 0.3 * np.sin(x * 0.07) * np.cos(y * 0.05)

    parts = [np.stack([gx, gy, height(gx, gy) + rng.normal(0, 0.02, gx.size)], 1)]
    for k in range(40):
        c = rng.uniform(-0.9 * extent, 0.9 * extent, 2) if k >= 8 else rng.uniform(-0.8 * frame_range, 0.8 * frame_range, 2)
        L, hd = rng.uniform(20.0, 50.0), rng.uniform(0.0, np.pi)
        s_, z_ = np.meshgrid(np.arange(-L / 2, L / 2, spacing), np.arange(0.0, 6.0, spacing), indexing="ij")
        s_, z_ = s_.ravel() + rng.uniform(-0.2, 0.2, s_.size), z_.ravel() + rng.uniform(-0.2, 0.2, z_.size)
        wx, wy = c[0] + s_ * np.cos(hd), c[1] + s_ * np.sin(hd)
        parts.append(np.stack([wx, wy, height(wx, wy) + z_], 1))
    for k in range(30):
        c = rng.uniform(-0.9 * extent, 0.9 * extent, 2) if k >= 10 else rng.uniform(-0.8 * frame_range, 0.8 * frame_range, 2)
        z_ = np.arange(0.0, 5.0, 0.5 * spacing)
        a = rng.uniform(0, 2 * np.pi, z_.size)
        parts.append(np.stack([c[0] + 0.2 * np.cos(a), c[1] + 0.2 * np.sin(a), height(c[0], c[1]) + z_], 1))
    tgt = (np.concatenate(parts, 0) + o).astype(np.float32)
    T = pose6d_matrix(o[0], o[1], o[2] + height(0.0, 0.0) + 1.8, 0.0, 0.0, 0.0)
    frame = map_frames(tgt, [T], n_frame, seed=seed + 1, frame_range=frame_range, noise=noise)[0]
    return tgt, frame, T


def map_frames(tgt, poses, n_frame=8_000, seed=0, frame_range=30.0, noise=0.02):
    """Frames cut out of an existing map at given sensor poses, with the recipe of the frame of scene_parkinglot / scene_prior_map: for pose
    T (4x4, sensor -> map), up to n_frame map points within frame_range metres (in x-y) of T's position, expressed in the sensor frame by
    T^-1 and perturbed by Gaussian range noise.  n_frame may be one number or one per pose.  -> list of [n_i, 3] float32 arrays."""
    rng = np.random.default_rng(seed)
    tgt = np.asarray(tgt, np.float32)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    sizes = np.broadcast_to(np.asarray(n_frame, np.int64), (len(poses),))
    out = []
    for T, m in zip(poses, sizes):
        R, t = T[:3, :3], T[:3, 3]
        dx, dy = tgt[:, 0] - np.float32(t[0]), tgt[:, 1] - np.float32(t[1])
        near = np.flatnonzero(dx * dx + dy * dy < np.float32(frame_range * frame_range))
        sel = rng.choice(near, size=min(int(m), len(near)), replace=False)
        body = (tgt[sel].astype(np.float64) - t) @ R          # R^T (p - t)
        body += rng.normal(0, noise, body.shape)
        out.append(body.astype(np.float32))
    return out


def drive(world, n_keyframes, step=1.5, n_frame=8_000, seed=0, start=None, heading=0.0, yaw_rate=0.01, frame_range=30.0, noise=0.02):
    """A drive through `world` for a growing map: n_keyframes sensor poses (4x4, sensor -> map) `step` metres apart along a gently curving
    path (heading in radians, yaw_rate radians per keyframe) from `start` (x, y; default: frame_range / 2 inside the world's x minimum, at
    its y centre), the sensor 1.8 m above the world's median height - a path that leaves the box of its first frames - and the frames cut
    from `world` there by map_frames.  -> (poses, frames)"""
    world = np.asarray(world, np.float32)
    lo, hi = world.min(0).astype(np.float64), world.max(0).astype(np.float64)
    x, y = (lo[0] + 0.5 * frame_range, 0.5 * (lo[1] + hi[1])) if start is None else (float(start[0]), float(start[1]))
    z = float(np.median(world[:, 2])) + 1.8
    poses = []
    yaw = heading
    for _ in range(n_keyframes):
        poses.append(pose6d_matrix(x, y, z, 0.0, 0.0, yaw))
        x += step * np.cos(yaw)
        y += step * np.sin(yaw)
        yaw += yaw_rate
    frames = map_frames(world, poses, n_frame, seed=seed, frame_range=frame_range, noise=noise)
    return poses, frames


def revisits(world, poses, n_revisits, max_offset=1.5, n_frame=8_000, seed=0, frame_range=30.0, noise=0.02):
    """Revisits of a drive for place recognition: n_revisits sweeps taken later near keyframes drawn without replacement from `poses`, each up
    to max_offset metres off its keyframe's position (uniform over the disc) and at a random yaw, cut from `world` by map_frames.
    -> (the keyframe each revisit is near [n] ascending, the revisits' sensor poses, their frames)"""
    rng = np.random.default_rng(seed)
    near = np.sort(rng.choice(len(poses), n_revisits, replace=False))
    out = []
    for kf in near:
        r, a = max_offset * np.sqrt(rng.uniform()), rng.uniform(0.0, 2 * np.pi)
        yaw = rng.uniform(0.0, 2 * np.pi)
        T = np.array(poses[kf], np.float64)
        T[:3, 3] += [r * np.cos(a), r * np.sin(a), 0.0]
        Rz = np.eye(4)
        Rz[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        out.append(T @ Rz)
    return near, out, map_frames(world, out, n_frame, seed=seed + 100, frame_range=frame_range, noise=noise)


def scan_pairs(tgt, poses, n_frame=8_000, seed=0, mode="submap", n_submap=100_000, submap_radius=40.0, frame_range=30.0, noise=0.02):
    """Scan pairs cut out of an existing map at sensor poses (4x4, sensor -> map), sources made by map_frames.  mode "submap": pair k = the
    frame at poses[k] against a submap crop - up to n_submap map points within submap_radius metres (in x-y) of poses[k]'s position, in
    the map frame (loop-closure verification against a submap).  mode "scan": pair k = the frame at poses[k + 1] against the frame at
    poses[k] (scan-to-scan odometry of a recorded drive: len(poses) - 1 pairs).  -> (sources, targets, T_true) with T_true[k] the 4x4 pose
    that maps source k into target k's frame."""
    rng = np.random.default_rng(seed + 1)
    tgt = np.asarray(tgt, np.float32)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    frames = map_frames(tgt, poses, n_frame, seed=seed, frame_range=frame_range, noise=noise)
    if mode == "scan":
        return frames[1:], frames[:-1], [np.linalg.inv(poses[k]) @ poses[k + 1] for k in range(len(poses) - 1)]
    if mode != "submap":
        raise ValueError("scan_pairs: mode is 'submap' or 'scan', got %r" % (mode,))
    targets = []
    for T in poses:
        dx, dy = tgt[:, 0] - np.float32(T[0, 3]), tgt[:, 1] - np.float32(T[1, 3])
        near = np.flatnonzero(dx * dx + dy * dy < np.float32(submap_radius * submap_radius))
        if len(near) > n_submap:
            near = np.sort(rng.choice(near, size=n_submap, replace=False))
        targets.append(np.ascontiguousarray(tgt[near]))
    return frames, targets, [T.copy() for T in poses]


def write_pcd_xyzi(path, xyz):
    """Binary PCD v0.7, fields x y z intensity (float32), like pcl::io::savePCDFileBinary<PointXYZI>."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = xyz
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
                 "COUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (n, n)).encode("ascii"))
        f.write(rec.tobytes())


def lidar_sweep(world, pose, rings=128, cols=1024, fov_up=22.5, fov_down=-22.5, min_range=0.5, max_range=80.0, noise=0.01, seed=0):
    """An ORGANISED sweep of a spinning LiDAR (rings x cols beams, e.g. 128 x 1024 = 131 k points) at the sensor pose `pose` (4x4, sensor ->
    map) over the points of `world`: each beam returns the nearest world point that falls in its pixel (azimuth column, elevation ring),
    placed on the beam's centre direction at that range plus Gaussian range noise; a beam with no point in range has no return and its row
    is NaN, as in an organised cloud.  -> [rings * cols, 3] float32 in the sensor frame, ring after ring."""
    rng = np.random.default_rng(seed)
    T = np.asarray(pose, np.float64)
    body = (np.asarray(world, np.float32).astype(np.float64) - T[:3, 3]) @ T[:3, :3]      # R^T (p - t)
    r = np.linalg.norm(body, axis=1)
    ok = (r > min_range) & (r < max_range)
    body, r = body[ok], r[ok]
    az = np.arctan2(body[:, 1], body[:, 0])
    el = np.degrees(np.arcsin(body[:, 2] / r))
    col = np.minimum((az + np.pi) / (2 * np.pi) * cols, cols - 1).astype(np.int64)
    ring = np.floor((fov_up - el) / (fov_up - fov_down) * rings).astype(np.int64)
    inside = (ring >= 0) & (ring < rings)
    pix, r = ring[inside] * cols + col[inside], r[inside]
    order = np.lexsort((r, pix))                       # nearest point of each pixel first
    first = order[np.r_[True, pix[order][1:] != pix[order][:-1]]] if len(order) else order
    rng_px = np.full(rings * cols, np.nan)
    rng_px[pix[first]] = r[first] + rng.normal(0.0, noise, len(first))
    jr, jc = np.divmod(np.arange(rings * cols), cols)
    a = (jc + 0.5) / cols * 2 * np.pi - np.pi
    e = np.radians(fov_up - (jr + 0.5) * (fov_up - fov_down) / rings)
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], 1)
    return (d * rng_px[:, None]).astype(np.float32)


def _se3_exp_many(xi):
    """SE(3) exponential of many twists [m, 6] = (w, v) (include/dcreg.h's formula) -> (R [m, 3, 3], t [m, 3])"""
    w, v = xi[:, :3], xi[:, 3:]
    th2 = np.einsum("ij,ij->i", w, w)
    th = np.sqrt(th2)
    small = th < 1e-3
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1 - th2 / 6 + th2 * th2 / 120, np.sin(ths) / ths)
    B = np.where(small, 0.5 - th2 / 24 + th2 * th2 / 720, (1 - np.cos(ths)) / ths ** 2)
    Cc = np.where(small, 1 / 6 - th2 / 120 + th2 * th2 / 5040, (ths - np.sin(ths)) / ths ** 3)
    W = np.zeros((len(xi), 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    W2 = W @ W
    eye = np.eye(3)[None]
    R = eye + A[:, None, None] * W + B[:, None, None] * W2
    V = eye + B[:, None, None] * W + Cc[:, None, None] * W2
    return R, np.einsum("mij,mj->mi", V, v)


def lidar_sweep_moving(world, pose_begin, motion, period=0.1, ref=0.5, rings=128, cols=1024, fov_up=22.5, fov_down=-22.5, min_range=0.5,
                       max_range=80.0, noise=0.01, seed=0):
    """lidar_sweep of a MOVING sensor: column j is measured at s_j = (j + 0.5) / cols * period seconds from the sensor pose
    T(s_j) = pose_begin Exp(s_j / period Log(motion)) (motion = the pose at the end of the sweep in the frame of the pose at its start: a
    constant twist over the sweep).  Each world point is assigned to the column whose pose sees it in that column (a fixed point found per
    point: a few vectorised passes over the world, not one per column); then, as lidar_sweep, each beam returns the nearest point of its pixel
    on the beam's centre direction plus range noise, NaN where there is none.  -> (records [rings * cols, 4] float32 = x y z in the sensor
    frame of the column's instant and the stamp s_j in seconds, ring after ring; the true sensor pose at the reference instant ref * period,
    4x4)."""
    from .api import se3_log, se3_exp
    rng = np.random.default_rng(seed)
    T0 = np.asarray(pose_begin, np.float64)
    xi = se3_log(motion)
    p = np.asarray(world, np.float32).astype(np.float64)
    d0 = p - T0[:3, 3]
    p = p[np.einsum("ij,ij->i", d0, d0) < (max_range + np.linalg.norm(xi[3:]) + 1.0) ** 2]
    stamps = (np.arange(cols) + 0.5) / cols * period
    Rc, tc = _se3_exp_many(np.outer(stamps / period, xi))
    Rc, tc = T0[:3, :3][None] @ Rc, T0[:3, :3] @ tc.T + T0[:3, 3][:, None]       # column poses in the world
    tc = tc.T

    def column_of(j):
        body = np.einsum("mji,mj->mi", Rc[j], p - tc[j])          # R_j^T (p - t_j)
        az = np.arctan2(body[:, 1], body[:, 0])
        return np.minimum((az + np.pi) / (2 * np.pi) * cols, cols - 1).astype(np.int64), body

    Rm, tm = T0[:3, :3] @ se3_exp(0.5 * xi)[:3, :3], T0[:3, :3] @ se3_exp(0.5 * xi)[:3, 3] + T0[:3, 3]
    body = (p - tm) @ Rm
    j = np.minimum((np.arctan2(body[:, 1], body[:, 0]) + np.pi) / (2 * np.pi) * cols, cols - 1).astype(np.int64)
    for _ in range(6):                                            # the column's own pose sees the point in that column
        jn, body = column_of(j)
        if np.array_equal(jn, j):
            break
        j = jn
    jn, body = column_of(j)
    keep = jn == j
    body, col = body[keep], j[keep]
    r = np.linalg.norm(body, axis=1)
    ok = (r > min_range) & (r < max_range)
    body, r, col = body[ok], r[ok], col[ok]
    el = np.degrees(np.arcsin(body[:, 2] / r))
    ring = np.floor((fov_up - el) / (fov_up - fov_down) * rings).astype(np.int64)
    inside = (ring >= 0) & (ring < rings)
    pix, r = ring[inside] * cols + col[inside], r[inside]
    order = np.lexsort((r, pix))
    first = order[np.r_[True, pix[order][1:] != pix[order][:-1]]] if len(order) else order
    rng_px = np.full(rings * cols, np.nan)
    rng_px[pix[first]] = r[first] + rng.normal(0.0, noise, len(first))
    jr, jc = np.divmod(np.arange(rings * cols), cols)
    a = (jc + 0.5) / cols * 2 * np.pi - np.pi
    e = np.radians(fov_up - (jr + 0.5) * (fov_up - fov_down) / rings)
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], 1)
    rec = np.empty((rings * cols, 4), np.float32)
    rec[:, :3] = d * rng_px[:, None]
    rec[:, 3] = stamps[jc]
    return rec, T0 @ se3_exp(ref * xi)


def lidar_sweep_path(world, body_poses_at, extrinsic, period=0.1, t_ref=0.05, rings=128, cols=1024, fov_up=22.5, fov_down=-22.5, min_range=0.5,
                     max_range=80.0, noise=0.01, seed=0):
    """lidar_sweep_moving along a PATH: column j is measured at s_j = (j + 0.5) / cols * period seconds from the sensor pose B(s_j) E, with
    B = body_poses_at(stamps [m]) -> (R [m, 3, 3], t [m, 3]) the poses of the body in the world (a vectorised callable, used as it answers:
    no interpolation here) and E = extrinsic the pose of the sensor in the body frame (4x4).  Same fixed-point column assignment, beam model
    and record layout as lidar_sweep_moving.  -> (records [rings * cols, 4] float32 = x y z in the sensor frame of the column's instant and
    the stamp s_j, ring after ring; the true sensor pose B(t_ref) E, 4x4)."""
    rng = np.random.default_rng(seed)
    E = np.asarray(extrinsic, np.float64)

    def sensor_poses(s):
        Rb, tb = body_poses_at(np.asarray(s, np.float64))
        return Rb @ E[:3, :3][None], Rb @ E[:3, 3] + tb

    stamps = (np.arange(cols) + 0.5) / cols * period
    Rc, tc = sensor_poses(stamps)                                 # column poses in the world
    Rm, tm = sensor_poses(np.array([0.5 * period]))
    Rm, tm = Rm[0], tm[0]
    p = np.asarray(world, np.float32).astype(np.float64)
    d0 = p - tm
    p = p[np.einsum("ij,ij->i", d0, d0) < (max_range + np.linalg.norm(tc - tm, axis=1).max() + 1.0) ** 2]

    def column_of(j):
        body = np.einsum("mji,mj->mi", Rc[j], p - tc[j])          # R_j^T (p - t_j)
        az = np.arctan2(body[:, 1], body[:, 0])
        return np.minimum((az + np.pi) / (2 * np.pi) * cols, cols - 1).astype(np.int64), body

    body = (p - tm) @ Rm
    j = np.minimum((np.arctan2(body[:, 1], body[:, 0]) + np.pi) / (2 * np.pi) * cols, cols - 1).astype(np.int64)
    for _ in range(6):                                            # the column's own pose sees the point in that column
        jn, body = column_of(j)
        if np.array_equal(jn, j):
            break
        j = jn
    jn, body = column_of(j)
    keep = jn == j
    body, col = body[keep], j[keep]
    r = np.linalg.norm(body, axis=1)
    ok = (r > min_range) & (r < max_range)
    body, r, col = body[ok], r[ok], col[ok]
    el = np.degrees(np.arcsin(body[:, 2] / r))
    ring = np.floor((fov_up - el) / (fov_up - fov_down) * rings).astype(np.int64)
    inside = (ring >= 0) & (ring < rings)
    pix, r = ring[inside] * cols + col[inside], r[inside]
    order = np.lexsort((r, pix))
    first = order[np.r_[True, pix[order][1:] != pix[order][:-1]]] if len(order) else order
    rng_px = np.full(rings * cols, np.nan)
    rng_px[pix[first]] = r[first] + rng.normal(0.0, noise, len(first))
    jr, jc = np.divmod(np.arange(rings * cols), cols)
    a = (jc + 0.5) / cols * 2 * np.pi - np.pi
    e = np.radians(fov_up - (jr + 0.5) * (fov_up - fov_down) / rings)
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], 1)
    rec = np.empty((rings * cols, 4), np.float32)
    rec[:, :3] = d * rng_px[:, None]
    rec[:, 3] = stamps[jc]
    Rr, tr = sensor_poses(np.array([float(t_ref)]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rr[0], tr[0]
    return rec, T


def turn_in_path(pose_begin, alpha=30.0, v0=10.0, dec=8.0):
    """A body path a constant twist cannot express, as lidar_sweep_path takes it: planar motion from pose_begin (4x4, body -> world at s = 0)
    with constant angular acceleration in yaw (yaw = alpha s^2 / 2) and speed v0 - dec s along the heading; the position is the integral of
    the velocity by 16-point Gauss-Legendre quadrature over [0, s] (exact to rounding for s of a sweep).
    -> callable stamps [m] -> (R [m, 3, 3], t [m, 3])"""
    T0 = np.asarray(pose_begin, np.float64)
    x16, w16 = np.polynomial.legendre.leggauss(16)

    def at(stamps):
        s = np.asarray(stamps, np.float64).reshape(-1)
        tau = 0.5 * s[:, None] * (x16 + 1.0)
        wt = 0.5 * s[:, None] * w16
        speed, yaw = v0 - dec * tau, 0.5 * alpha * tau ** 2
        local = np.zeros((len(s), 3))
        local[:, 0], local[:, 1] = np.sum(wt * speed * np.cos(yaw), 1), np.sum(wt * speed * np.sin(yaw), 1)
        c, sn = np.cos(0.5 * alpha * s ** 2), np.sin(0.5 * alpha * s ** 2)
        Rl = np.zeros((len(s), 3, 3))
        Rl[:, 0, 0], Rl[:, 0, 1], Rl[:, 1, 0], Rl[:, 1, 1], Rl[:, 2, 2] = c, -sn, sn, c, 1.0
        return T0[:3, :3][None] @ Rl, local @ T0[:3, :3].T + T0[:3, 3]

    return at
