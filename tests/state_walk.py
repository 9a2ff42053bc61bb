"""Seeded random call sequences against a context: the model of what a caller can know, the operations, the generator, the probes and a
fake context (tests/test_state_walk_model.py runs all of it without a device, tests/test_gpu_state_walk.py on one).

The MODEL holds the map (float32, index order), the radius hint of the last set_target, the source, the options, the kept normals of map,
source and loaded frames (by `keep` with its parameters or by `set` with the array), the parameters of the kept voxel map (`vm`: whether
a keep keeps a voxel at all is tests/voxels_ref.py's answer), the clouds added to the places database and to the keyframe store, and
whether a gate is pending.  The options hold the robust kernel, its scales, gicp_epsilon and the voxel mode too: they change results, are
read at every launch, and go into context B with the rest.  Every transition rule is one sentence of include/dcreg.h (cited as `h:LINE`) or of
include/dcreg_debug.h (`d:LINE`).  Expected clouds come from the bitwise numpy references the suite already has (transform and crop_ref of
test_gpu_map_update.py, voxel_ref, outliers_ref, visibility_ref, keyframes_ref); the deskew forms, specified to one ulp only, take theirs
from the cloud form on a helper context (`Model.deskew`: h:417-418 promises that the two are bitwise equal).  The calls of the
global-alignment chain (descriptors, matching, the sampler, the consensus graph) change no state: their whole ANSWER is compared, bitwise,
with that of a context that has done nothing else (`alone`, `Model.fresh`), and the probe "desc" reads the map form of the descriptors.

An OPERATION is a function op_NAME(m, c, **args): it reads its precondition from the model, derives the call's concrete arguments from
the scene and the model, predicts the return code (0, or the refusal the header names), makes the call on the context c (None: the model
alone), checks the code and, for an accepted call, applies the rule to the model.  Arguments are small literals, so a walk prints as a
literal that `replay` accepts."""
import ctypes as C
import functools
import hashlib
import re

import numpy as np

import align_scenes as als
import consensus_scenes as cs
import keyframes_ref as kr
import normal_icp_scenes as S
import outliers_ref as orf
import visibility_ref as vr
import voxels_ref as vx
import voxels_scenes as vxs
from dcreg_amd import api
from test_gpu_map_update import crop_ref, transform
from test_gpu_normals import OPTS_WINDOW
from test_gpu_voxel import voxel_ref

OK, E_INVALID, E_STATE = 0, -1, -4
RADIUS = S.RADIUS
FRAME_SIZES = (1, 63, 257, 1000)
WINDOW_OFF = [("max_table_entries", 1 << 30), ("roi_index", 1), ("roi_margin", 20.0)]     # the defaults (h:165, h:190, h:185)
TOGGLES = {"normals_follow": (0, 1), "map_update": (0, 1), "warm_start": (0, 1), "use_certificates": (0, 1), "one_wave": (0, 1, 2),
           "advance": (0, 1, 2), "team_pass": (0, 1, 2), "dispatch_order": (0, 1), "gap_field": (0, 1),
           # the options that DO change results, each read at every launch (h:182-192, h:1129-1133): the model carries them into context B
           "robust_kernel": (0, 1, 2, 3), "voxels_source_cov": (0, 1), "robust_scale": (0.05, 0.3), "gicp_robust_scale": (0.7, 2.0),
           "gicp_epsilon": (1e-3, 1e-2)}
DEFAULTS = dict({"normals_follow": 0, "map_update": 1, "warm_start": 1, "use_certificates": 1, "one_wave": 1, "advance": 1, "team_pass": 1,
                 "dispatch_order": 1, "gap_field": 1, "robust_kernel": 0, "voxels_source_cov": 0, "robust_scale": 0.1, "gicp_robust_scale": 1.0,
                 "gicp_epsilon": 1e-3}, **dict(WINDOW_OFF))
# values that dcreg_set_option refuses with DCREG_E_INVALID, the old value staying (h:186-187, h:189, h:1130, h:182)
REFUSED_OPTIONS = (("robust_kernel", 4), ("robust_scale", 0), ("voxels_source_cov", 2), ("gicp_epsilon", 2))
VOXEL_PARAMS = ((1.0, 1e-3, 6), (1.0, 1e-3, 3), (0.5, 1e-2, 3))         # (leaf, epsilon, min_points) of dcreg_target_voxels_keep
SPAN_LEAF = 1e-7                                                        # a leaf at which every map here spans 2^21 voxels or more (h:1125)
PLACE = dict(n_rings=8, n_sectors=24, max_range=12.0, min_range=0.0, z_offset=2.0)
VIS = dict(rows=16, cols=128, elev_min=-0.5, elev_max=0.5, min_range=0.3, max_range=30.0, margin_abs=0.2, margin_rel=0.01, window=1)
TWIST = (0.002, -0.001, 0.02, 0.3, 0.05, 0.01)
ICP_ITERS = 8


class Unexpected(Exception):
    """a call returned a code the model did not expect"""


# ---- the scene: normal_icp_scenes.lot(), a 4000-point map with a 523-point source; nothing is larger
@functools.lru_cache(maxsize=None)
def poses():
    return list(S.walk()) + [S.lot()["GT"]]


def cloud(key):
    """the cloud a literal key names: ("src",), ("frame", n), ("tgt", n), ("pool", start, n) and, around any of them, ("nan", key): one
    coordinate NaN, ("allnan", n): no finite point, ("two", key): two columns only (a bad stride)"""
    kind = key[0]
    if kind == "src":
        return S.lot()["src"]
    if kind == "frame":
        return S.sized_source(key[1])
    if kind == "tgt":
        return S.lot()["tgt"][:key[1]]
    if kind == "pool":
        return np.ascontiguousarray(S.sized_source(1000)[key[1]:key[1] + key[2]])
    if kind == "nan":
        a = np.array(cloud(key[1]), np.float32)
        a[len(a) // 2, 1] = np.nan
        return a
    if kind == "allnan":
        return np.full((key[1], 3), np.nan, np.float32)
    if kind == "two":
        return np.ascontiguousarray(cloud(key[1])[:, :2])
    raise KeyError(key)


def sweep_records(key):
    """the cloud with a float32 stamp in [0, 0.1] s in a fourth column"""
    a = cloud(key)
    return np.ascontiguousarray(np.concatenate([a, np.linspace(0.0, 0.1, len(a), dtype=np.float32)[:, None]], 1))


def sweep_args(path):
    """-> (field, motion) for deskew / (field, stamps, poses, block) for deskew_path"""
    field = api.time_field(3, "f32", 1.0)
    D = api.se3_exp(list(TWIST))
    if not path:
        return field, api.sweep_motion(D[:3, :3], D[:3, 3], span=(0.0, 0.1), ref=0.5)
    half = api.se3_exp([0.5 * v for v in TWIST])
    return field, [0.0, 0.05, 0.1], np.stack([np.eye(4), half, D]), api.sweep_path(0, 3, 0.05)


def host_deskew(path, rec):
    """a stand-in for the model-only runs (the expected source of the deskew forms needs a device: GpuDeskew of test_gpu_state_walk.py)"""
    a = (rec[:, 3].astype(np.float64) - 0.05) / 0.1
    out = rec[:, :3].astype(np.float64)
    for i in range(len(out)):
        E = api.se3_exp([a[i] * v for v in TWIST])
        out[i] = E[:3, :3] @ out[i] + E[:3, 3]
    return out.astype(np.float32)


host_deskew.tag = "host"


def digest(*parts):
    h = hashlib.sha1()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
        h.update(b"|")
    return h.hexdigest()[:16]


_memo = {}


def memo(tag, fn, *parts):
    """the references are pure: a walk replayed against several contexts computes each of them once"""
    key = (tag, digest(*parts))
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def outliers_kept(xyz, p):
    return memo("out", lambda: orf.outlier_reference(xyz, **p)["kept"], xyz, sorted(p.items()))


def voxel_of(xyz, leaf):
    return memo("vox", lambda: voxel_ref(xyz, leaf), xyz, leaf)


def visibility_kept(xyz, store, members, p):
    vp = api.visibility_params(**p)
    return memo("vis", lambda: vr.filter_ref(xyz, store, members, vp)[0], xyz, [len(s) for s in store], *[s for s in store],
                [(i, digest(T)) for i, T in members], sorted(p.items()))


def thinned(ref_map, q, min_spacing):
    """h:292-295: appended unless the map as it stood has a point with float d2 < (float)(min_spacing^2), d2 as dcreg_knn computes it"""
    if min_spacing <= 0.0:
        return q
    d2 = np.min(orf.d2_f32(q, ref_map), axis=1)
    return q[~(d2 < np.float32(min_spacing * min_spacing))]


def vmap_of(xyz, p):
    """the reference voxel map of a cloud for p = (leaf, epsilon, min_points) (tests/voxels_ref.py)"""
    return memo("vmap", lambda: vx.voxel_map(xyz, *p), xyz, tuple(p))


def spans_too_far(xyz, leaf):
    """h:1124-1125: a map that spans 2^21 or more voxels on an axis"""
    v = vx.voxel_of(xyz, leaf)
    return bool(((v.max(axis=0) - v.min(axis=0)) >= 2.0 ** 21).any())


def vlin_of(vmap, src, T, mode, normals, eps, kind, scale):
    return memo("vlin", lambda: vx.linearize(vmap, src, T, mode, normals, eps, kind, scale), vmap["coords"], vmap["mean"], vmap["cov"], vmap["leaf"],
                src, np.asarray(T, np.float64), mode, None if normals is None else np.asarray(normals), eps, kind, scale)


def given_normals(n, seed):
    a = np.array(S.unit_normals(n, seed))
    a[::17, 0] = np.nan                   # h:904: a non-finite component means "this point has no normal"
    return a


class Model:
    def __init__(self, deskew=host_deskew):
        self.deskew = deskew
        self.opts = dict(DEFAULTS)
        self.map, self.radius, self.src = None, None, None
        self.tn, self.sn = None, None             # ("keep", (k, search_radius)) | ("set", array)
        self.frames, self.fn = None, None         # tuple of cloud keys | as tn
        self.places, self.kf = None, None         # list of clouds (None: not reset yet)
        self.gate = False
        self.follow_n = 0                         # dcreg_target_normals_follow_info().n_target
        self.reserved = 0
        self.vm = None                            # (leaf, epsilon, min_points) of the last accepted keep that kept a voxel
        self.fresh, self.fresh_tag = None, ""     # makes a context that has done nothing yet (run_walk: the chain's answers are compared with its)

    # ---- the rules
    def new_target(self, xyz, radius):
        """h:195-197 the map and its radius hint; h:906-908 + h:947-948 every set_target form drops the kept normals; h:967-971 (the
        sentence this suite added) the follow record is cleared"""
        self.map, self.radius, self.tn, self.follow_n = np.ascontiguousarray(xyz[:, :3], np.float32), radius, None, 0
        self.reserved = 0                         # h:251 dcreg_set_target / dcreg_set_source drop all states
        self.vm = None                            # h:1121-1122 every call that changes the map's points drops the kept voxels

    def updated_target(self, xyz):
        """h:270-272 the map is the updated cloud; h:957 an update that changes nothing leaves normals and info; h:942-947 the kept
        normals follow when the option is on and they came from keep, h:906-908 otherwise they are dropped; h:967 n_target; h:1121-1122
        the kept voxels are dropped whatever normals_follow says ("Nothing follows the map")"""
        if len(xyz) == len(self.map) and np.array_equal(xyz.view(np.uint32), self.map.view(np.uint32)):
            return
        self.map, self.follow_n = np.ascontiguousarray(xyz, np.float32), len(xyz)
        self.reserved = 0                         # h:273-274 an update that changes the map drops what dcreg_set_target drops
        self.vm = None
        if not (self.tn and self.tn[0] == "keep" and self.opts["normals_follow"]):
            self.tn = None

    def new_source(self, xyz):
        """h:204-209 the source; h:995-996 every set_source form drops the kept source normals"""
        self.src, self.sn, self.reserved = np.ascontiguousarray(xyz[:, :3], np.float32), None, 0     # (h:251)

    def loaded(self, keys, normals=None):
        """d:168-172 the frames of one call stay on the device; d:206 every load drops their normals (h:1226-1228: the gicp form keeps its own)"""
        self.frames, self.fn = tuple(keys), normals

    def window_live(self):
        return self.opts["roi_index"] == 2 and self.map is not None and self.src is not None

    def members(self, spec):
        return [(i, poses()[p]) for i, p in spec]

    def vmap(self):
        """the reference's kept voxels of the map (None: no member)"""
        return None if self.vm is None else vmap_of(self.map, self.vm)

    def voxels_ready(self):
        """h:1147-1148 what dcreg_linearize_voxels needs: target, source, kept voxels and in mode 1 kept source normals"""
        return bool(self.map is not None and self.src is not None and self.vm and (not self.opts["voxels_source_cov"] or self.sn))


def rc_of(e):
    m = re.search(r"failed \((-?\d+)\)", str(e))
    return int(m.group(1)) if m else None


def call(m, c, want, fn):
    """the call on the context (c None: the model alone), its return code checked against the model's"""
    if m.gate and want == OK:
        raise AssertionError("the generator queued a call behind a pending gate")
    if c is None:
        return None
    try:
        out, rc = fn(), OK
    except api.DcregError as e:
        out, rc = None, rc_of(e)
    if rc != want:
        raise Unexpected("expected %d, got %r" % (want, rc))
    return out


def cfg_of(iters=ICP_ITERS):
    return api.default_config(search_radius=RADIUS, max_iterations=iters, gt_matrix=S.lot()["GT"].reshape(16))


def np_params(p):
    return api.normal_params(k=p[0], search_radius=p[1])


# ---- the operations.  Each returns the code it expects; CLASS says how the generator weighs it.
OPS, CLASS = {}, {}


def op(cls):
    def reg(fn):
        OPS[fn.__name__[3:]] = fn
        CLASS[fn.__name__[3:]] = cls
        return fn
    return reg


def no_target(m):
    return m.map is None


@op("target")
def op_set_target(m, c, key=("tgt", 4000), radius=RADIUS):
    want = E_INVALID if key[0] in ("nan", "two") else OK             # h:202 a refused cloud leaves the clouds as they were
    call(m, c, want, lambda: c.set_target(cloud(key), radius))
    if want == OK:
        m.new_target(cloud(key), radius)
    return want


@op("target")
def op_set_target_voxel(m, c, key=("tgt", 4000), leaf=0.3):
    want = E_INVALID if key[0] == "allnan" else OK                   # h:348-350 no point left after the pass
    call(m, c, want, lambda: c.set_target_voxel(cloud(key), RADIUS, leaf))
    if want == OK:
        m.new_target(voxel_of(cloud(key), leaf), RADIUS)             # h:347-348 exactly as set_target of the output
    return want


OUT_RADIUS = dict(mode="radius", radius=0.5, min_neighbors=3)
OUT_STAT = dict(mode="statistical", k=8, std_mul=2.0, search_radius=0.0)
OUT_NONE = dict(mode="statistical", k=8, std_mul=1.0e6, search_radius=0.0)      # keeps every point


@op("target")
def op_set_target_outliers(m, c, key=("tgt", 4000), stat=0):
    p = OUT_STAT if stat else OUT_RADIUS
    want = E_INVALID if key[0] == "allnan" else OK                   # h:631-632 no point left
    call(m, c, want, lambda: c.set_target_outliers(cloud(key), RADIUS, api.outlier_params(**p)))
    if want == OK:
        m.new_target(outliers_kept(cloud(key), p), RADIUS)           # h:630 bitwise as set_target of the filtered cloud
    return want


@op("target")
def op_set_target_keyframes(m, c, spec=((0, 5),), leaf=None, bad=0):
    if m.kf is None:
        want = E_STATE                                               # h:693-694 any call but _reset / _count before the first _reset
    elif bad:
        spec, want = ((len(m.kf), 5),), E_INVALID                    # h:691-692 an id outside [0, count)
    elif not m.kf:
        return None
    else:
        want = OK
    call(m, c, want, lambda: c.set_target_keyframes(m.members(spec), RADIUS, leaf=leaf))
    if want == OK:
        m.new_target(kr.submaps_ref(m.kf, [m.members(spec)], leaf)[0][0], RADIUS)        # h:686-688
    return want


@op("source")
def op_set_source(m, c, key=("src",)):
    want = E_INVALID if key[0] in ("nan", "two") else OK             # h:208 non-finite coordinates are refused
    call(m, c, want, lambda: c.set_source(cloud(key)))
    if want == OK:
        m.new_source(cloud(key))
    return want


@op("source")
def op_set_source_voxel(m, c, key=("frame", 1000), leaf=0.2):
    want = E_INVALID if key[0] == "allnan" else OK                   # h:348-350
    call(m, c, want, lambda: c.set_source_voxel(cloud(key), leaf))
    if want == OK:
        m.new_source(voxel_of(cloud(key), leaf))
    return want


@op("source")
def op_set_source_outliers(m, c, key=("frame", 1000), stat=1):
    p = OUT_STAT if stat else OUT_RADIUS
    want = E_INVALID if key[0] == "allnan" else OK                   # h:631-632
    call(m, c, want, lambda: c.set_source_outliers(cloud(key), api.outlier_params(**p)))
    if want == OK:
        m.new_source(outliers_kept(cloud(key), p))
    return want


@op("source")
def op_set_source_deskew(m, c, key=("src",)):
    want = E_INVALID if key[0] == "nan" else OK                      # h:417-418 a point that comes out non-finite refuses the call
    field, motion = sweep_args(False)
    call(m, c, want, lambda: c.set_source_deskew(sweep_records(key), field, motion))
    if want == OK:
        m.new_source(memo("deskew", lambda: m.deskew(False, sweep_records(key)), key, m.deskew.tag))
    return want


@op("source")
def op_set_source_deskew_path(m, c, key=("frame", 257)):
    want = E_INVALID if key[0] == "nan" else OK                      # h:461-463 the behaviour of dcreg_set_source_deskew
    field, st, P, block = sweep_args(True)
    call(m, c, want, lambda: c.set_source_deskew_path(sweep_records(key), field, st, P, block))
    if want == OK:
        m.new_source(memo("deskew_path", lambda: m.deskew(True, sweep_records(key)), key, m.deskew.tag))
    return want


@op("update")
def op_insert(m, c, key=("pool", 0, 100), pose=5, spacing=0.0, dup=0):
    """dup: the first points of the map itself at the identity: with a spacing every one of them is thinned away (h:295 changes nothing)"""
    T = np.eye(4) if dup else poses()[pose]
    xyz = (np.ascontiguousarray(m.map[:dup]) if dup and m.map is not None else cloud(key))
    want = E_STATE if no_target(m) else E_INVALID if key[0] == "nan" else OK           # h:275-277
    call(m, c, want, lambda: c.insert(xyz, T, spacing))
    if want == OK:
        m.updated_target(np.concatenate([m.map, thinned(m.map, transform(xyz, T), spacing)]))     # h:292-295
    return want


@op("update")
def op_insert_source(m, c, pose=5, spacing=0.0):
    want = E_STATE if no_target(m) or m.src is None else OK          # h:276-277 no target, no source for _insert_source
    call(m, c, want, lambda: c.insert_source(poses()[pose], spacing))
    if want == OK:
        m.updated_target(np.concatenate([m.map, thinned(m.map, transform(m.src, poses()[pose]), spacing)]))     # h:300
    return want


def crop_box(m, axis, side, frac):
    lo, hi = m.map.min(0).astype(np.float64) - 1.0, m.map.max(0).astype(np.float64) + 1.0
    if frac >= 2.0:                                                  # a box beside the map: keeps nothing
        lo[axis] = hi[axis] + 1.0
        hi[axis] = lo[axis] + 1.0
    elif frac > 0.0:
        span = float(m.map[:, axis].max() - m.map[:, axis].min())
        if side:
            hi[axis] = float(m.map[:, axis].max()) - frac * span
        else:
            lo[axis] = float(m.map[:, axis].min()) + frac * span
    return lo, hi


@op("update")
def op_crop(m, c, axis=0, side=0, frac=0.1):
    """frac 0 keeps everything (changes nothing), frac 2 keeps nothing (refused)"""
    if no_target(m):
        lo, hi, want = np.zeros(3), np.ones(3), E_STATE
    else:
        lo, hi = crop_box(m, axis, side, frac)
        want = E_INVALID if len(crop_ref(m.map, lo, hi)) == 0 else OK                  # h:276 a crop that would keep no point
    call(m, c, want, lambda: c.crop(lo, hi))
    if want == OK:
        m.updated_target(crop_ref(m.map, lo, hi))                    # h:302
    return want


@op("update")
def op_remove_outliers(m, c, kind=0):
    p = (OUT_RADIUS, OUT_STAT, OUT_NONE)[kind]
    want = E_STATE if no_target(m) else OK                           # h:646
    if want == OK and len(outliers_kept(m.map, p)) == 0:
        want = E_INVALID                                             # h:645-646 a call that would remove every point is refused
    call(m, c, want, lambda: c.remove_outliers(api.outlier_params(**p)))
    if want == OK:
        m.updated_target(outliers_kept(m.map, p))                    # h:642-645
    return want


@op("update")
def op_remove_dynamic(m, c, spec=((0, 5),), min_votes=1):
    """min_votes 100: no point gathers as many, the call removes nothing (h:766)"""
    want = E_STATE if m.kf is None or no_target(m) else OK           # h:770-771 no store, no target
    if not m.kf:
        return None                                                  # (the binding asks the store for its size first: never generated)
    p = dict(VIS, min_votes=min_votes)
    if want == OK and len(visibility_kept(m.map, m.kf, m.members(spec), p)) == 0:
        want = E_INVALID                                             # h:766-767
    call(m, c, want, lambda: c.remove_dynamic(m.members(spec), api.visibility_params(**p)))
    if want == OK:
        m.updated_target(visibility_kept(m.map, m.kf, m.members(spec), p))             # h:763-765
    return want


@op("member")
def op_keep_target_normals(m, c, k=5, radius=0.0):
    want = E_STATE if no_target(m) else OK                           # h:910
    call(m, c, want, lambda: c.keep_target_normals(np_params((k, radius))))
    if want == OK:
        m.tn = ("keep", (k, radius))                                 # h:900-901
    return want


@op("member")
def op_set_target_normals(m, c, seed=3, short=0):
    n = 0 if no_target(m) else len(m.map)
    want = E_STATE if no_target(m) else E_INVALID if short else OK   # h:909-910 n different from the map's size
    call(m, c, want, lambda: c.set_target_normals(given_normals(max(n - short, 1), seed)))
    if want == OK:
        m.tn = ("set", given_normals(n, seed))                       # h:902-903
    return want


@op("member")
def op_drop_target_normals(m, c):
    call(m, c, OK, lambda: c.drop_target_normals())
    m.tn = None                                                      # h:905
    return OK


@op("member")
def op_keep_source_normals(m, c, k=5, radius=0.0):
    want = E_STATE if m.src is None else OK                          # h:999
    call(m, c, want, lambda: c.keep_source_normals(np_params((k, radius))))
    if want == OK:
        m.sn = ("keep", (k, radius))                                 # h:988-989
    return want


@op("member")
def op_set_source_normals(m, c, seed=5, short=0):
    n = 0 if m.src is None else len(m.src)
    want = E_STATE if m.src is None else E_INVALID if short else OK  # h:998-999
    call(m, c, want, lambda: c.set_source_normals(given_normals(max(n - short, 1), seed)))
    if want == OK:
        m.sn = ("set", given_normals(n, seed))                       # h:990-991
    return want


@op("member")
def op_drop_source_normals(m, c):
    call(m, c, OK, lambda: c.drop_source_normals())
    m.sn = None                                                      # h:994
    return OK


@op("member")
def op_keep_target_voxels(m, c, p=(1.0, 1e-3, 3), span=0):
    """span: the leaf SPAN_LEAF, at which the map spans more voxels than the pass allows: refused, the member as it was (h:1124-1125)"""
    if span:
        p = (SPAN_LEAF,) + tuple(p[1:])
    want = E_STATE if no_target(m) else E_INVALID if spans_too_far(m.map, p[0]) else OK        # h:1126 no target
    if bool(span) != (want == E_INVALID):
        return None                                                  # (a map too small, or too wide, for the form asked for)
    info = call(m, c, want, lambda: c.keep_target_voxels(api.voxel_map_params(*p)))
    if want == OK:
        n_kept = vmap_of(m.map, p)["n_kept"]
        if info is not None and info["n_kept"] != n_kept:
            raise AssertionError("keep_target_voxels%r kept %d voxels, the reference %d" % (tuple(p), info["n_kept"], n_kept))
        m.vm = tuple(p) if n_kept else None                          # h:1114 a keep that keeps no voxel succeeds and leaves no member
    return want


@op("member")
def op_drop_target_voxels(m, c):
    call(m, c, OK, lambda: c.drop_target_voxels())
    m.vm = None                                                      # h:1114 _drop frees the member
    return OK


def frame_keys(sizes):
    return tuple(("frame", n) for n in sizes)


def frames_of(keys):
    return [cloud(k) for k in keys]


@op("member")
def op_frames_load(m, c, sizes=(63, 257, 1000), bad=0):
    keys = frame_keys(sizes)
    if bad:
        keys = keys[:-1] + (("nan", keys[-1]),)
    want = E_INVALID if bad else OK                                  # h:1201 non-finite coordinates in any frame
    call(m, c, want, lambda: c.frames_load(frames_of(keys)))
    if want == OK:
        m.loaded(keys)
    else:
        m.fn = None                                                  # d:206 (the sentence this suite added): a refused load drops them too
    return want


@op("member")
def op_frames_normals_keep(m, c, k=5, radius=0.0):
    want = E_STATE if not m.frames else OK                           # d:209 without loaded frames
    call(m, c, want, lambda: c.frames_normals_keep(np_params((k, radius))))
    if want == OK:
        m.fn = ("keep", (k, radius))                                 # d:202-204
    return want


@op("member")
def op_frames_normals_set(m, c, seed=7, short=0):
    n = sum(len(f) for f in frames_of(m.frames)) if m.frames else 0
    want = E_STATE if not m.frames else E_INVALID if short else OK   # d:207-209 a point count that is not the load's
    call(m, c, want, lambda: c.frames_normals_set(given_normals(max(n - short, 1), seed)))
    if want == OK:
        m.fn = ("set", given_normals(n, seed))                       # d:204-205
    return want


@op("member")
def op_places_reset(m, c):
    call(m, c, OK, lambda: c.places_reset(api.place_params(**PLACE)))
    m.places = []                                                    # h:535
    return OK


@op("member")
def op_places_add_clouds(m, c, keys=(("frame", 257),)):
    if m.places is None:
        return None                                                  # (refused by the binding, not by the library: never generated)
    call(m, c, OK, lambda: c.places_add_clouds([cloud(k) for k in keys]))
    m.places += [cloud(k) for k in keys]                             # h:541
    return OK


@op("member")
def op_places_add_source(m, c):
    if m.places is None:
        return None
    want = E_STATE if m.src is None else OK                          # h:511-512 a _source form without a source
    call(m, c, want, lambda: c.places_add_source())
    if want == OK:
        m.places.append(m.src)                                       # h:545
    return want


@op("member")
def op_keyframes_reset(m, c):
    call(m, c, OK, lambda: c.keyframes_reset())
    m.kf = []                                                        # h:702
    return OK


@op("member")
def op_keyframes_add(m, c, keys=(("pool", 0, 500),)):
    want = E_STATE if m.kf is None else E_INVALID if any(k[0] == "nan" for k in keys) else OK      # h:693-694, h:661-663
    if want == OK and len(m.kf) + len(keys) > 4:
        return None                                                  # (the scene: at most 4 keyframes)
    call(m, c, want, lambda: c.keyframes_add([cloud(k) for k in keys]))
    if want == OK:
        m.kf += [cloud(k) for k in keys]                             # h:656-657
    return want


@op("member")
def op_keyframes_add_source(m, c):
    want = E_STATE if m.kf is None or m.src is None else OK          # h:693-694 _add_source without a source
    if want == OK and (len(m.kf) + 1 > 4 or len(m.src) > 500):
        return None
    call(m, c, want, lambda: c.keyframes_add_source())
    if want == OK:
        m.kf.append(m.src)                                           # h:664-665
    return want


@op("member")
def op_reserve_warm_states(m, c, n=3):
    if m.src is None:
        return None                                                  # (h:243 a state is sized by the source: reserved once there is one)
    call(m, c, OK, lambda: c.reserve_warm_states(n))                 # h:241-250 results are identical with or without states
    m.reserved = n                                                   # h:243-244 ids 0 <= id < n_states
    return OK


@op("member")
def op_reset_warm_state(m, c, state=-1):
    if state >= 0 and state >= m.reserved:
        return None                                                  # (h:244 only a reserved id; h:251 set_target / set_source drop them)
    call(m, c, OK, lambda: c.reset_warm_state(state))                # h:246-250
    return OK


@op("option")
def op_set_option(m, c, key="normals_follow", value=1):
    want = E_INVALID if (key, value) in REFUSED_OPTIONS else OK      # (REFUSED_OPTIONS has the lines): the old value stays
    call(m, c, want, lambda: c.set_option(key, value))               # h:144 results are identical whatever their values - but for those of
    if want == OK:                                                   # TOGGLES' second line, which the model carries into context B
        m.opts[key] = value
    return want


@op("option")
def op_set_window(m, c, on=1):
    for k, v in (OPTS_WINDOW if on else WINDOW_OFF):                 # h:182-192 the same neighbours and bitwise the same sums
        call(m, c, OK, lambda: c.set_option(k, v))
        m.opts[k] = 1 << 20 if k == "max_table_entries" and on else v
    return OK


# ---- the cloud forms: they use the context's scratch and change nothing (h:316, h:590-591, h:842-843, h:505-507, h:695-696)
@op("scratch")
def op_voxel_downsample(m, c):
    call(m, c, OK, lambda: c.voxel_downsample([cloud(("frame", 1000)), cloud(("frame", 63))], 0.25))
    return OK


@op("scratch")
def op_normals(m, c):
    call(m, c, OK, lambda: c.normals(cloud(("frame", 1000)), np_params((8, 0.0))))
    return OK


@op("scratch")
def op_normals_clouds(m, c):
    call(m, c, OK, lambda: c.normals_clouds(frames_of(frame_keys(FRAME_SIZES)), np_params((5, 0.5))))
    return OK


@op("scratch")
def op_outlier_filter(m, c):
    call(m, c, OK, lambda: c.outlier_filter(cloud(("tgt", 3000)), api.outlier_params(**OUT_STAT)))
    return OK


@op("scratch")
def op_visibility_filter(m, c, spec=((0, 5),)):
    if not m.kf:
        return None
    call(m, c, OK, lambda: c.visibility_filter(cloud(("tgt", 2000)), m.members(spec), api.visibility_params(**dict(VIS, min_votes=1))))
    return OK


@op("scratch")
def op_place_descriptors(m, c):
    call(m, c, OK, lambda: c.place_descriptors([cloud(("src",)), cloud(("frame", 257))], api.place_params(**PLACE)))
    return OK


@op("scratch")
def op_keyframe_submaps(m, c, spec=((0, 5),), leaf=0.3):
    if not m.kf:
        return None
    call(m, c, OK, lambda: c.keyframe_submaps([m.members(spec), m.members(spec[:1])], leaf=leaf))
    return OK


# ---- the global-alignment chain: descriptors, matching, the sampler and the consensus graph.  Scratch users too - they share the outlier
# scratch and its index, the normal scratch, the sort's and each other's (c->feat, c->algn) - and each promises an answer that depends on
# its inputs only and is bitwise the same on another context (h:1674-1675 + h:1686-1687, h:1742, h:1786-1790, h:1847-1848, h:1924-1925).
# So the WHOLE answer is compared with that of a context that has done nothing else, obtained once per argument set.
def frozen(x):
    """an answer - nested dicts, lists, arrays and numbers - as comparable items, arrays and floats by their bits"""
    if isinstance(x, dict):
        return [(k, frozen(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [frozen(v) for v in x]
    return None if x is None else bits(np.asarray(x))


def alone(m, c, tag, parts, fn):
    got = call(m, c, OK, lambda: fn(c))
    if c is None or m.fresh is None:
        return OK

    def first():
        b = m.fresh()
        try:
            return frozen(fn(b))
        finally:
            b.close()
    if frozen(got) != memo("alone %s %s" % (tag, m.fresh_tag), first, *parts):
        raise AssertionError("%s%r does not answer as a context that has done nothing else" % (tag, tuple(parts)))
    return OK


CHAIN_NORMALS = (8, 0.0)


@op("scratch")
def op_fpfh(m, c, n=1000, k=16, radius=0.0):
    """the normals are estimated in the call (h:1680-1682) and returned with the descriptors"""
    return alone(m, c, "fpfh", (n, k, radius), lambda x: x.fpfh(cloud(("frame", n)), None, np_params(CHAIN_NORMALS),
                                                                 api.fpfh_params(k=k, search_radius=radius), want_normals=True))


@op("scratch")
def op_fpfh_radius(m, c, n=1000, radius=0.9, cap=65535):
    return alone(m, c, "fpfh_radius", (n, radius, cap), lambda x: x.fpfh_radius(cloud(("frame", n)), None, np_params(CHAIN_NORMALS),
                                                                                  api.fpfh_radius_params(radius, cap), want_normals=True))


@functools.lru_cache(maxsize=None)
def feature_rows(n, seed):
    """n seeded rows of 33 floats in 0 .. 100, every 29th with a NaN (h:1780: neither a query nor a candidate)"""
    a = np.random.default_rng(5200 + seed + n).uniform(0.0, 100.0, (n, 33)).astype(np.float32)
    a[::29, n % 33] = np.nan
    a.setflags(write=False)
    return a


@op("scratch")
def op_feature_match(m, c, n_a=257, n_b=1000):
    return alone(m, c, "feature_match", (n_a, n_b), lambda x: x.feature_match(feature_rows(n_a, 1), feature_rows(n_b, 2)))


@op("scratch")
def op_align_correspondences(m, c, pairs=400, seed=1):
    a, b, ca, cb = als.synthetic(pairs, 0.3, 0.02, 60 + pairs)[:4]
    p = dict(n_hypotheses=2000, seed=seed, inlier_distance=0.1, edge_similarity=0.9, n_best=2, refine_iterations=3)
    return alone(m, c, "align_correspondences", (pairs, seed), lambda x: x.align_correspondences(a, b, ca, cb, api.align_params(**p)))


@op("scratch")
def op_consensus_correspondences(m, c, pairs=400):
    a, b, ca, cb = cs.scene(pairs, 0.1, 70 + pairs)[:4]
    return alone(m, c, "consensus_correspondences", (pairs,),
                 lambda x: x.consensus_correspondences(a, b, ca, cb, api.consensus_params(**cs.SETTINGS), want_members=True, want_weights=True))


# ---- history makers: the engines and the batched calls.  They leave warm states, window and scratch behind, and no result depends on it.
def bad_pose():
    T = np.array(poses()[0])
    T[1, 3] = np.nan
    return T


def ready(m):
    return m.map is not None and m.src is not None


@op("history")
def op_linearize(m, c, pose=0, bad=0):
    if not ready(m):
        return None
    T = bad_pose() if bad else poses()[pose]
    want = E_INVALID if bad else OK                                  # h:213-215 a NaN pose: warm states, window and gate stay
    call(m, c, want, lambda: c.linearize(T[:3, :3], T[:3, 3], api.default_lin_params(RADIUS)))
    return want


@op("history")
def op_linearize_normals(m, c, pose=0):
    want = OK if ready(m) and m.tn else E_STATE                      # h:933 no target, no source, no kept normals
    call(m, c, want, lambda: c.linearize_normals(poses()[pose], api.default_lin_params(RADIUS)))
    return want


@op("history")
def op_linearize_gicp(m, c, pose=0):
    want = OK if ready(m) and m.tn and m.sn else E_STATE             # h:1028
    call(m, c, want, lambda: c.linearize_gicp(poses()[pose], api.default_lin_params(RADIUS)))
    return want


@op("history")
def op_icp_run(m, c, pose=0, bad=0):
    if not ready(m):
        return None
    want = E_INVALID if bad else OK                                  # h:213-215 the engines' initial poses
    call(m, c, want, lambda: c.icp_run(bad_pose() if bad else poses()[pose], "Ours", cfg_of()))
    return want


@op("history")
def op_icp_run_normals(m, c, pose=0):
    if not ready(m):
        return None
    want = OK if m.tn else E_STATE                                   # h:1113-1114
    call(m, c, want, lambda: c.icp_run_normals(poses()[pose], "Ours", cfg_of()))
    return want


@op("history")
def op_icp_run_gicp(m, c, pose=0):
    if not ready(m):
        return None
    want = OK if m.tn and m.sn else E_STATE                          # h:1121-1122
    call(m, c, want, lambda: c.icp_run_gicp(poses()[pose], "Ours", cfg_of()))
    return want


def frame_poses(n, first=0):
    return np.stack([poses()[(first + i) % len(poses())] for i in range(n)])


@op("history")
def op_register_frames(m, c, sizes=(63, 257, 1), first=0, bad=0):
    keys = frame_keys(sizes)
    if bad:
        keys = (("nan", keys[0]),) + keys[1:]
    want = E_STATE if no_target(m) else E_INVALID if bad else OK     # h:1201-1202
    call(m, c, want, lambda: c.register_frames(frames_of(keys), frame_poses(len(keys), first), "Ours", cfg_of(), slots=2))
    if want == OK:
        m.loaded(keys)
    elif want == E_INVALID:
        m.fn = None                                                  # d:206
    return want


@op("history")
def op_register_frames_normals(m, c, sizes=(63, 257, 1), first=0):
    keys = frame_keys(sizes)
    want = OK if m.map is not None and m.tn else E_STATE             # h:1214-1215 results (and the frames) are left untouched
    call(m, c, want, lambda: c.register_frames_normals(frames_of(keys), frame_poses(len(keys), first), "Ours", cfg_of(), slots=2))
    if want == OK:
        m.loaded(keys)
    return want


@op("history")
def op_register_frames_gicp(m, c, sizes=(63, 257, 1), first=0, k=5):
    keys = frame_keys(sizes)
    want = OK if m.map is not None and m.tn else E_STATE             # h:1233
    call(m, c, want, lambda: c.register_frames_gicp(frames_of(keys), frame_poses(len(keys), first), "Ours", cfg_of(), np_params((k, 0.0)), slots=2))
    if want == OK:
        m.loaded(keys, ("keep", (k, 0.0)))                           # h:1226-1228 kept beside the frames' points
    return want


@op("history")
def op_register_pairs(m, c, bad=0):
    src = [cloud(("frame", 63)), cloud(("frame", 257)), cloud(("nan", ("src",))) if bad else cloud(("src",))]
    tgt = [cloud(("tgt", 600)), cloud(("tgt", 1500)), cloud(("tgt", 2000))]
    want = E_INVALID if bad else OK                                  # h:1252-1254 leaves target, source, states, frames and window
    call(m, c, want, lambda: c.register_pairs(src, tgt, frame_poses(3, 2), "Ours", cfg_of(), slots=2))
    return want


@op("history")
def op_icp_run_trials(m, c, first=0, bad=0):
    if not ready(m):
        return None
    T = frame_poses(4, first)
    if bad:
        T[2, 0, 3] = np.inf
    want = E_INVALID if bad else OK                                  # h:213-215 of any of its n_poses
    call(m, c, want, lambda: c.icp_run_trials(T, "Ours", cfg_of()))
    return want


@op("history")
def op_icp_run_trials_normals(m, c, first=0):
    if not ready(m):
        return None
    want = OK if m.tn else E_STATE                                   # h:1214-1215
    call(m, c, want, lambda: c.icp_run_trials_normals(frame_poses(4, first), "Ours", cfg_of()))
    return want


@op("history")
def op_icp_run_trials_gicp(m, c, first=0):
    if not ready(m):
        return None
    want = OK if m.tn and m.sn else E_STATE                          # h:1233-1234
    call(m, c, want, lambda: c.icp_run_trials_gicp(frame_poses(4, first), "Ours", cfg_of()))
    return want


# ---- the fourth engine (h:1128-1149, h:1263-1268, h:1383-1404) and the pair forms of the second and third (h:1428-1446)
@op("history")
def op_linearize_voxels(m, c, pose=0):
    want = OK if m.voxels_ready() else E_STATE                       # h:1147-1148 no target, no source, no kept voxels, mode 1: no source normals
    call(m, c, want, lambda: c.linearize_voxels(poses()[pose], api.default_lin_params(RADIUS)))
    return want


@op("history")
def op_icp_run_voxels(m, c, pose=0):
    if not ready(m):
        return None
    want = OK if m.voxels_ready() else E_STATE                       # h:1263-1264 dcreg_target_voxels_keep first; mode 1: kept source normals too
    call(m, c, want, lambda: c.icp_run_voxels(poses()[pose], "Ours", cfg_of()))
    return want


@op("history")
def op_icp_run_trials_voxels(m, c, first=0, bad=0):
    if not ready(m):
        return None
    T = frame_poses(4, first)
    if bad:
        T[2, 0, 3] = np.inf
    want = E_STATE if not m.voxels_ready() else E_INVALID if bad else OK       # h:1397-1401; h:226-228 a non-finite pose of any of its n_poses
    call(m, c, want, lambda: c.icp_run_trials_voxels(T, "Ours", cfg_of()))
    return want


@op("history")
def op_register_frames_voxels(m, c, sizes=(63, 257, 1), first=0, bad=0):
    """mode 1 ("voxels_source_cov" as the call finds it, h:1394): the frames' normals are estimated behind the load with k = 5"""
    keys = frame_keys(sizes)
    if bad:
        keys = (("nan", keys[0]),) + keys[1:]
    mode = m.opts["voxels_source_cov"]
    want = E_STATE if no_target(m) or not m.vm else E_INVALID if bad else OK   # h:1400-1401, before the load; h:1386-1387 non-finite coordinates
    call(m, c, want, lambda: c.register_frames_voxels(frames_of(keys), frame_poses(len(keys), first), "Ours", cfg_of(),
                                                      frame_normals=np_params((5, 0.0)) if mode else None, slots=2))
    if want == OK:
        m.loaded(keys, ("keep", (5, 0.0)) if mode else None)         # h:1402-1403 replaces the frames and their kept normals; h:1396-1397
    elif want == E_INVALID:
        m.fn = None                                                  # d:206
    return want


def _pairs(bad):
    src = [cloud(("frame", 63)), cloud(("frame", 257)), cloud(("nan", ("src",))) if bad else cloud(("src",))]
    return src, [cloud(("tgt", 600)), cloud(("tgt", 1500)), cloud(("tgt", 2000))]


@op("history")
def op_register_pairs_normals(m, c, bad=0):
    src, tgt = _pairs(bad)
    want = E_INVALID if bad else OK                                  # h:1441-1446 leaves target, normals, source, states, frames and window
    call(m, c, want, lambda: c.register_pairs_normals(src, tgt, frame_poses(3, 2), "Ours", cfg_of(), np_params((5, 0.0)), slots=2))
    return want


@op("history")
def op_register_pairs_gicp(m, c, bad=0):
    src, tgt = _pairs(bad)
    want = E_INVALID if bad else OK                                  # h:1441-1446
    call(m, c, want, lambda: c.register_pairs_gicp(src, tgt, frame_poses(3, 2), "Ours", cfg_of(), np_params((5, 0.0)), np_params((5, 0.0)), slots=2))
    return want


# ---- the gate: _gated_begin, one other call (refused with DCREG_E_STATE, h:221-226, changing nothing), then _gate_abort or _gate_open
GATED_OTHERS = ("set_source", "set_target", "knn", "keep_target_normals", "frames_load", "reset_warm_state", "insert",
                "keep_target_voxels", "linearize_voxels")            # h:1126, h:1148 a linearisation in flight


@op("gate")
def op_gated_begin(m, c):
    if not ready(m) or m.gate:
        return None
    call(m, c, OK, lambda: c.linearize_gated_begin(api.default_lin_params(RADIUS)))     # h:230-236
    m.gate = True
    return OK


@op("gate")
def op_gated_other(m, c, which="knn"):
    if not m.gate:
        return None
    fn = {"set_source": lambda: c.set_source(cloud(("frame", 63))), "set_target": lambda: c.set_target(cloud(("tgt", 600)), RADIUS),
          "knn": lambda: c.knn(cloud(("frame", 63)), k=1), "keep_target_normals": lambda: c.keep_target_normals(np_params((5, 0.0))),
          "frames_load": lambda: c.frames_load([cloud(("frame", 63))]), "reset_warm_state": lambda: c.reset_warm_state(-1),
          "insert": lambda: c.insert(cloud(("pool", 0, 50)), poses()[5]),
          "keep_target_voxels": lambda: c.keep_target_voxels(api.voxel_map_params(*VOXEL_PARAMS[1])),
          "linearize_voxels": lambda: c.linearize_voxels(poses()[0], api.default_lin_params(RADIUS))}[which]
    call(m, c, E_STATE, fn)                                          # h:221-226; d:206 a load refused for a launch in flight drops nothing
    return E_STATE


@op("gate")
def op_gate_end(m, c, open=0, pose=2):
    if not m.gate:
        return None
    m.gate = False
    if open and not m.window_live():                                 # h:187-188: behind a window a queued launch may be called off
        T = poses()[pose]
        call(m, c, OK, lambda: (c.gate_open(T[:3, :3], T[:3, 3]), c.linearize_end(0)))
    else:
        call(m, c, OK, lambda: c.gate_abort())                       # h:232-233 returns without touching results or warm state
    return OK


STATE_CLASSES = ("target", "source", "update", "member", "option")
PROBE_KINDS = ("map", "flags", "lin", "nlin", "glin", "knn", "p2p", "normals", "frames", "frames_n", "frames_g", "batch", "icp", "places", "submaps",
               "voxels", "vlin", "icp_v", "frames_v", "trials_v", "vbatch", "pairs", "desc")
LAUNCHING = tuple(k for k in PROBE_KINDS if k not in ("map", "flags", "normals", "voxels", "desc"))      # the probes that launch an engine's kernels


def apply(m, c, step):
    name, args = step
    return OPS[name](m, c, **args)


def replay(c, ops, m=None, deskew=host_deskew):
    """applies a list of (operation, arguments) to the context and to a model -> the model"""
    m = m or Model(deskew)
    for step in ops:
        if apply(m, c, step) is None:
            raise AssertionError("%r: its precondition does not hold at this point of the list" % (step,))
    return m


# ---- the generator
def _draw_args(rng, name, m):
    """one accepted form, and where the operation has a refusal one refused form, both as literals: -> (accepted, refused or None)"""
    r = lambda seq: seq[int(rng.integers(len(seq)))]
    i = lambda lo, hi: int(rng.integers(lo, hi + 1))
    kf_n = len(m.kf) if m.kf else 0
    spec = tuple((i(0, kf_n - 1), r((2, 5))) for _ in range(i(1, 2))) if kf_n else ((0, 5),)
    patch = ("pool", i(0, 700), i(50, 300))
    t = {
        "set_target": (dict(key=("tgt", r((4000, 3000))), radius=r((0.5, 1.0))), dict(key=r((("nan", ("tgt", 4000)), ("two", ("tgt", 4000)))))),
        "set_target_voxel": (dict(key=("tgt", 4000), leaf=r((0.3, 0.5))), dict(key=("allnan", 40))),
        "set_target_outliers": (dict(key=("tgt", r((4000, 2500))), stat=i(0, 1)), dict(key=("allnan", 40))),
        "set_target_keyframes": (dict(spec=spec, leaf=r((None, 0.25))), dict(bad=1)),
        "set_source": (dict(key=r((("src",), ("frame", 257), ("frame", 1000), ("frame", 63)))), dict(key=r((("nan", ("src",)), ("two", ("src",)))))),
        "set_source_voxel": (dict(key=("frame", 1000), leaf=r((0.2, 0.4))), dict(key=("allnan", 30))),
        "set_source_outliers": (dict(key=r((("frame", 1000), ("src",))), stat=i(0, 1)), dict(key=("allnan", 30))),
        "set_source_deskew": (dict(key=r((("src",), ("frame", 257)))), dict(key=("nan", ("src",)))),
        "set_source_deskew_path": (dict(key=r((("frame", 257), ("src",)))), dict(key=("nan", ("frame", 257)))),
        "insert": (r((dict(key=patch, pose=r((2, 5))), dict(key=patch, pose=5, spacing=0.05), dict(dup=i(50, 300), spacing=0.05))),
                   dict(key=("nan", patch))),
        "insert_source": (dict(pose=r((2, 5)), spacing=r((0.0, 0.05))), None),
        "crop": (dict(axis=i(0, 1), side=i(0, 1), frac=r((0.0, 0.05, 0.1))), dict(axis=i(0, 2), frac=2.0)),
        "remove_outliers": (dict(kind=i(0, 2)), None),
        "remove_dynamic": (dict(spec=spec, min_votes=r((1, 100))), None),
        "keep_target_normals": (dict(k=r((5, 8)), radius=r((0.0, 0.5))), None),
        "set_target_normals": (dict(seed=i(1, 9)), dict(seed=1, short=1)),
        "drop_target_normals": ({}, None),
        "keep_source_normals": (dict(k=r((5, 6)), radius=0.0), None),
        "set_source_normals": (dict(seed=i(1, 9)), dict(seed=1, short=2)),
        "drop_source_normals": ({}, None),
        "frames_load": (dict(sizes=r(((63, 257, 1000), (1, 63), (257, 1, 1000, 63)))), dict(bad=1)),
        "frames_normals_keep": (dict(k=r((5, 6))), None),
        "frames_normals_set": (dict(seed=i(1, 9)), dict(seed=1, short=1)),
        "places_reset": ({}, None),
        "places_add_clouds": (dict(keys=r(((("frame", 257),), (("frame", 63), ("frame", 1000))))), None),
        "places_add_source": ({}, None),
        "keyframes_reset": ({}, None),
        "keyframes_add": (dict(keys=r(((("pool", 0, 500),), (("pool", 500, 500), ("frame", 257))))), dict(keys=(("nan", ("frame", 63)),))),
        "keyframes_add_source": ({}, None),
        "reserve_warm_states": (dict(n=i(1, 4)), None),
        "reset_warm_state": (dict(state=r((-1, 0))), None),
        # (walk_ops takes key and value of an accepted set_option off OPTION_DECK)
        "set_option": (dict(key="normals_follow", value=1), dict(zip(("key", "value"), r(REFUSED_OPTIONS)))),
        "keep_target_voxels": (dict(p=r(VOXEL_PARAMS)), dict(p=VOXEL_PARAMS[1], span=1)),
        "drop_target_voxels": ({}, None),
        "linearize_voxels": (dict(pose=i(0, 5)), None),
        "icp_run_voxels": (dict(pose=r((0, 2))), None),
        "icp_run_trials_voxels": (dict(first=i(0, 5)), dict(bad=1)),
        "register_frames_voxels": (dict(sizes=r(((63, 257, 1), (1000, 63))), first=i(0, 5)), dict(bad=1)),
        "register_pairs_normals": ({}, dict(bad=1)),
        "register_pairs_gicp": ({}, dict(bad=1)),
        "set_window": (dict(on=r((1, 1, 0))), None),
        # the chain: two sizes each, so that a large call is followed by a small one and the other way round on the same scratch
        "fpfh": (r((dict(n=1000, k=16), dict(n=257, k=9, radius=0.7), dict(n=63, k=32))), None),
        "fpfh_radius": (r((dict(n=1000, radius=0.9), dict(n=257, radius=1.2, cap=30))), None),
        "feature_match": (r((dict(n_a=257, n_b=1000), dict(n_a=1000, n_b=63))), None),
        "align_correspondences": (dict(pairs=r((400, 150)), seed=i(1, 2)), None),
        "consensus_correspondences": (dict(pairs=r((400, 150))), None),
        "visibility_filter": (dict(spec=spec), None),
        "keyframe_submaps": (dict(spec=spec, leaf=r((None, 0.3))), None),
        "linearize": (dict(pose=i(0, 5)), dict(bad=1)),
        "linearize_normals": (dict(pose=i(0, 5)), None),
        "linearize_gicp": (dict(pose=i(0, 5)), None),
        "icp_run": (dict(pose=r((0, 2, 3))), dict(bad=1)),
        "icp_run_normals": (dict(pose=r((0, 2))), None),
        "icp_run_gicp": (dict(pose=r((0, 2))), None),
        "register_frames": (dict(sizes=r(((63, 257, 1), (1000, 63))), first=i(0, 5)), dict(bad=1)),
        "register_frames_normals": (dict(first=i(0, 5)), None),
        "register_frames_gicp": (dict(first=i(0, 5), k=r((5, 6))), None),
        "register_pairs": ({}, dict(bad=1)),
        "icp_run_trials": (dict(first=i(0, 5)), dict(bad=1)),
        "icp_run_trials_normals": (dict(first=i(0, 5)), None),
        "icp_run_trials_gicp": (dict(first=i(0, 5)), None),
    }
    return t.get(name, ({}, None))


WEIGHTS = {"target": 1, "source": 1, "update": 2, "member": 1, "option": 3, "scratch": 1, "history": 1, "gate": 2}
# (OPTION_DECK has twice the values it had when "option" got its 3; the sampler and the consensus stage share c->algn, and only a walk that
# holds both, the sampler first, can tell whether the second reads what the first left: twice each, so that either order occurs)
NAME_WEIGHTS = {"set_option": 8, "align_correspondences": 2, "consensus_correspondences": 2}
# every value of every option but its default, and normals_follow, the robust kernel and the voxel mode off again (a context warmed under a
# kernel answers under none): one fixed shuffle, entered where the seed says
OPTION_DECK = ([(k, v) for k in sorted(TOGGLES) for v in TOGGLES[k] if v != DEFAULTS[k]] +
               [("normals_follow", 0), ("robust_kernel", 0), ("voxels_source_cov", 0)])
PROLOGUE = ("keyframes_reset", "places_reset", "set_target", "set_source", "keyframes_add", "places_add_clouds")
STATE_REFUSALS = ("insert_source", "keep_target_normals", "keep_source_normals", "frames_normals_keep", "places_add_source",
                  "keyframes_add_source", "keyframes_add", "linearize_normals", "linearize_gicp", "icp_run_normals", "icp_run_gicp",
                  "register_frames_normals", "register_frames_gicp", "icp_run_trials_normals", "icp_run_trials_gicp", "set_target_keyframes",
                  "remove_outliers", "remove_dynamic", "insert", "register_frames", "keep_target_voxels", "linearize_voxels", "icp_run_voxels",
                  "icp_run_trials_voxels", "register_frames_voxels")


def refusable():
    """the operations for which the header names a refusal that a walk can reach"""
    m, rng = Model(), np.random.default_rng(0)
    return sorted(set(n for n in OPS if _draw_args(rng, n, m)[1] is not None) | set(STATE_REFUSALS) | {"gated_other"})


def clone(m):
    import copy
    n = copy.copy(m)
    n.opts = dict(m.opts)
    n.places = None if m.places is None else list(m.places)
    n.kf = None if m.kf is None else list(m.kf)
    return n


def _repairs(m):
    out = []
    if m.map is None:
        return ["set_target"]
    if m.src is None:
        return ["set_source"]
    if not m.tn:
        return ["keep_target_normals", "set_target_normals", "set_target_normals"]
    if not m.sn:
        out += ["keep_source_normals", "set_source_normals"]
    if not m.vm:
        out.append("keep_target_voxels")
    if m.opts["roi_index"] != 2:
        out.append("set_window")
    if not m.opts["normals_follow"]:
        out.append(("set_option", dict(key="normals_follow", value=1)))
    if not m.opts["robust_kernel"]:
        out.append(("set_option", dict(key="robust_kernel", value=1 + len(m.map) % 3)))
    return out


def _deck(rng, names):
    d = list(names)
    rng.shuffle(d)
    return d


def walk_ops(seed, n_steps):
    """a list of (operation, arguments).  Operations come off a deck that holds every operation WEIGHTS[its class] times (NAME_WEIGHTS
    where it names the operation), shuffled (so map
    updates, source changes, member changes, history makers and scratch users alternate, and a walk uses as many different operations as
    it has steps for); one whose precondition does not hold yet waits in the deck.  Between them, with fixed probabilities, a member that
    the last steps dropped is put back (so that probes meet it live) and a call that the header refuses is made - at most a fifth of the
    steps.  The option values, the calls made behind a gate and the gate's end come off decks of their own (OPTION_DECK, GATED_OTHERS),
    entered where the seed says, so that the committed seeds share them."""
    rng = np.random.default_rng(seed)
    m, ops, refused = Model(), [], 0
    every = sorted(n for n in OPS if n not in ("gated_other", "gate_end"))
    deck, bad_deck = [], []
    options = _deck(np.random.default_rng(7), OPTION_DECK)
    at = (int(seed) * 5) % len(options)
    options = options[at:] + options[:at]
    gates = [0]

    def take(name, args):
        nonlocal m, refused
        trial = clone(m)
        rc = apply(trial, None, (name, args))
        if rc is None:
            return None
        m = trial
        ops.append((name, args))
        refused += rc != OK
        return rc

    def take_accepted(name, args):
        """a keep of the voxels under a window comes right behind a single-pose launch: no probe runs between the two (a launch is not
        a state-changing step), so the window is the active index when the keep reads the map"""
        if name == "keep_target_voxels" and m.window_live() and len(ops) + 2 <= n_steps:
            take("linearize", dict(pose=int(rng.integers(6))))
        return take(name, args)

    def gate_sequence():
        turn = int(seed) * 3 + gates[0]                              # the refused call and the end in turn, from a start the seed moves
        other = int(seed) * 4 + gates[0]                             # (a step coprime to the number of calls: neighbouring seeds reach them all)
        gates[0] += 1
        for st in [("gated_begin", {}), ("gated_other", dict(which=GATED_OTHERS[other % len(GATED_OTHERS)])),
                   ("gate_end", dict(open=1 - turn % 2, pose=int(rng.integers(6))))]:
            take(*st)

    prologue = _deck(rng, PROLOGUE)                                  # an empty context first: the refusals for a missing member live here
    while len(ops) < n_steps:
        u = rng.random()
        early = bool(prologue)
        if u < (0.45 if early else 0.16) and (refused + 1) * 5 <= n_steps:
            if not bad_deck:
                names = refusable()                                  # in a fixed order from a start the seed moves: neighbouring seeds
                at = (int(seed) * 13) % len(names)                   # cover different stretches of the list
                bad_deck = names[at:] + names[:at]
            scan = list(bad_deck)
            if early:                                                # one of the refusals for a missing member, while members are missing
                now = [n for n in bad_deck if n in STATE_REFUSALS and apply(clone(m), None, (n, _draw_args(rng, n, m)[0])) not in (None, OK)]
                scan = ([now[int(rng.integers(len(now)))]] if now else []) + scan
            for name in scan:                                        # the first of the deck that is refused as things stand
                j = bad_deck.index(name)
                if name == "gated_other":
                    if not ready(m) or len(ops) + 3 > n_steps:
                        continue
                    gate_sequence()
                    del bad_deck[j]
                    break
                good, bad = _draw_args(rng, name, m)
                forms = [f for f in ((good, bad) if early else (bad, good)) if f is not None]
                hit = [f for f in forms if apply(clone(m), None, (name, f)) not in (None, OK)]
                if hit:
                    take(name, hit[0])
                    del bad_deck[j]
                    break
        elif prologue:
            for j, name in enumerate(prologue):                      # (keyframes_add waits for keyframes_reset)
                good = _draw_args(rng, name, m)[0]
                if apply(clone(m), None, (name, good)) == OK:
                    take(name, good)
                    del prologue[j]
                    break
        elif u < 0.46 and _repairs(m):
            fix = _repairs(m)
            name = fix[int(rng.integers(len(fix)))]
            if isinstance(name, tuple):
                name, good = name
            else:
                good, _ = _draw_args(rng, name, m)
            if name == "set_window":
                good = dict(on=1)
            take_accepted(name, good)
        else:
            if not deck:                                             # one shuffle for all seeds, entered where the seed says: the committed
                deck = _deck(np.random.default_rng(2024), [n for n in every for _ in range(NAME_WEIGHTS.get(n, WEIGHTS[CLASS[n]]))])      # seeds share the work
                at = (int(seed) * 17) % len(deck)
                deck = deck[at:] + deck[:at]
            for j, name in enumerate(deck):                          # the first of the deck that is accepted as things stand
                if name == "gated_begin":
                    if ready(m) and len(ops) + 3 <= n_steps and (refused + 1) * 5 <= n_steps:
                        gate_sequence()
                        del deck[j]
                        break
                    continue
                good, _ = _draw_args(rng, name, m)
                if name == "set_option":
                    key, value = options[0]
                    options = options[1:] + options[:1]
                    good = dict(key=key, value=value)
                if apply(clone(m), None, (name, good)) == OK:
                    take_accepted(name, good)
                    del deck[j]
                    if name in ("keyframes_reset", "places_reset"):  # an emptied store is filled again next
                        deck.insert(0, "keyframes_add" if name == "keyframes_reset" else "places_add_clouds")
                    break
            else:
                deck = []
    return ops[:n_steps]


# ---- what the comparison reads: the probes.  Each returns a dict of comparable values; A (warm from its history) and B (fresh) must agree
# on every key, and the entries under "model" must equal what the model says.
def bits(a):
    a = np.ascontiguousarray(a)
    return (a.dtype.str, a.shape, a.tobytes())


def fields(s, skip=()):
    """a ctypes record as comparable items, field by field (padding never compared), the timing fields left out"""
    out = []
    for name, _ in s._fields_:
        if name in skip:
            continue
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out += [(name + "." + k, x) for k, x in fields(v, skip)]
        elif isinstance(v, C.Array):
            out.append((name, bits(np.array(v[:]))))
        else:
            out.append((name, bits(np.array(v))))
    return out


TIMING = ("time_ms", "iter_time_ms")


def records(recs):
    return [(k + "[%d]" % f, v) for f, r in enumerate(recs) for k, v in fields(r, TIMING)]


def refusal(fn):
    """the value of a probe, or ("refused", code)"""
    try:
        return fn()
    except api.DcregError as e:
        return [("refused", rc_of(e))]


def sums(d):
    return [(k, bits(np.asarray(d[k]))) for k in ("H_upper", "g", "sum_r2", "sum_b2", "n_eff", "n_pt")]


def dump(d, keys):
    return [(k, bits(np.asarray(d[k]))) for k in keys]


def probe(kind, c, m, pose, fresh=False):
    """-> (items compared between A and B, items compared with the model: (key, got, expected)); fresh: c is a context built by
    build_fresh, whose map no update has changed yet (h:967-971)"""
    T = poses()[pose]
    lp = api.default_lin_params(RADIUS)
    mod = []
    if kind == "map":
        got = c.target_points() if m.map is not None else np.zeros((0, 3), np.float32)
        exp = m.map if m.map is not None else np.zeros((0, 3), np.float32)
        info = c.index_info()
        mod = [("target_points", bits(got), bits(exp)), ("n_target", int(info.n_target), len(exp)),
               ("n_source", int(info.n_source), 0 if m.src is None else len(m.src))]
        if m.map is not None:
            mod.append(("index_check", c.index_check(), {"points": 0, "table": 0, "row_words": 0, "gap": 0, "owner": 0}))
        return [], mod
    if kind == "flags":
        mod = [("target_normals_kept", c.target_normals_kept(), int(bool(m.tn))), ("source_normals_kept", c.source_normals_kept(), int(bool(m.sn))),
               ("frames_normals_kept", c.frames_normals_kept(), int(bool(m.fn))),
               ("follow.n_target", c.normals_follow_info()["n_target"], 0 if fresh else m.follow_n),
               ("places_count", c.places_count(), len(m.places or [])), ("keyframes_count", c.keyframes_count(), len(m.kf or [])),
               ("target_voxels_kept", c.target_voxels_kept(), m.vmap()["n_kept"] if m.vm else 0)]                 # h:1113
        return [], mod
    if kind == "lin":
        if not ready(m):
            return [], []
        d = c.linearize(T[:3, :3], T[:3, 3], lp, debug=True)
        return dump(d, ("nn_idx", "nn_d2", "flag", "normal", "r", "s")) + sums(d) + [("plain." + k, v) for k, v in sums(c.linearize(T[:3, :3], T[:3, 3], lp))], []
    if kind == "nlin":
        out = refusal(lambda: sums(c.linearize_normals(T, lp)))
        return out, [("nlin refusal", out[0] == ("refused", E_STATE), not (ready(m) and m.tn))]
    if kind == "glin":
        out = refusal(lambda: sums(c.linearize_gicp(T, lp)))
        return out, [("glin refusal", out[0] == ("refused", E_STATE), not (ready(m) and m.tn and m.sn))]
    if kind == "knn":
        if m.map is None:
            return [], []
        q = transform(cloud(("frame", 257)), T)
        out = []
        for k, r in ((1, 0.0), (5, 0.0), (1, 0.4), (5, 0.4)):
            idx, d2 = c.knn(q, k=k, max_radius=r)
            out += [("knn %d %g idx" % (k, r), bits(idx)), ("knn %d %g d2" % (k, r), bits(d2))]
        return out, []
    if kind == "p2p":
        if not ready(m):
            return [], []
        return [("p2p", bits(np.array(c.p2p_error(T, 0.3), np.float64)))], []
    if kind == "normals":
        out = []
        if m.tn:
            n, cur = c.kept_target_normals()
            out += [("target normals", bits(n)), ("target curvature", bits(cur))]
            if m.tn[0] == "set":
                mod.append(("given target normals", bits(n), bits(np.ascontiguousarray(m.tn[1][:, :3]))))
        if m.sn:
            n, cur = c.kept_source_normals()
            out += [("source normals", bits(n)), ("source curvature", bits(cur))]
            if m.sn[0] == "set":
                mod.append(("given source normals", bits(n), bits(np.ascontiguousarray(m.sn[1][:, :3]))))
        return out, mod
    if kind in ("frames", "frames_n", "frames_g"):
        if m.map is None or (kind != "frames" and not m.tn):
            return [], []
        keys = frame_keys((257, 63, 1000))
        fn = {"frames": lambda: c.register_frames(frames_of(keys), frame_poses(3, pose), "Ours", cfg_of(), slots=2),
              "frames_n": lambda: c.register_frames_normals(frames_of(keys), frame_poses(3, pose), "Ours", cfg_of(), slots=2),
              "frames_g": lambda: c.register_frames_gicp(frames_of(keys), frame_poses(3, pose), "Ours", cfg_of(), np_params((5, 0.0)), slots=2)}[kind]
        out = records(fn())
        m.loaded(keys, ("keep", (5, 0.0)) if kind == "frames_g" else None)          # (the probe's own load: d:206, h:1226-1228)
        return out, []
    if kind == "batch":
        # the loaded frames and their kept normals, through the device seam of the batched engines (d:179-186, d:210-216)
        if not (m.map is not None and m.tn and m.frames):
            return [], []
        ids = [f for f, k in enumerate(m.frames) if len(cloud(k)) > 0]
        Ts = frame_poses(len(ids), pose)
        out = [("batch[%d].%s" % (f, k), v) for f, d in enumerate(c.normals_batch(Ts, frame_ids=ids, params=lp)) for k, v in sums(d)]
        if m.fn:
            out += [("gbatch[%d].%s" % (f, k), v) for f, d in enumerate(c.gicp_batch(Ts, frame_ids=ids, params=lp)) for k, v in sums(d)]
        return out, []
    if kind == "icp":
        if not ready(m):
            return [], []
        res, logs = c.icp_run(T, "Ours", cfg_of())
        return fields(res, TIMING) + records(logs), []
    if kind == "places":
        if not m.places or m.src is None:
            return [], []
        idx, shift, dist, info = c.places_query_source(k=min(3, len(m.places)))
        return [("places idx", bits(idx)), ("places shift", bits(shift)), ("places dist", bits(dist)), ("places info", sorted(info.items()))], []
    if kind == "submaps":
        if not m.kf:
            return [], []
        members = [[(i, poses()[(pose + i) % 6]) for i in range(len(m.kf))], [(0, T)]]
        out = []
        for leaf in (None, 0.3):
            subs, info = c.keyframe_submaps(members, leaf=leaf)
            out += [("submap %r %d" % (leaf, g), bits(s)) for g, s in enumerate(subs)] + [("submaps info %r" % (leaf,), sorted(info.items()))]
        return out, []
    mode = m.opts["voxels_source_cov"]
    if kind == "voxels":
        # the kept records themselves: bitwise the reference's of the model's map (h:1096-1113)
        if not m.vm:
            return [], []
        got, want = c.kept_target_voxels(), m.vmap()
        return ([("voxels " + k, bits(got[k])) for k in ("coords", "count", "mean", "cov")],
                [("kept voxels " + k, bits(got[k]), bits(want[k])) for k in ("coords", "count", "mean", "cov")])
    if kind == "vlin":
        if not m.voxels_ready():                                     # h:1147-1148 (the plain call: a dump needs a source to size it)
            out = refusal(lambda: sums(c.linearize_voxels(T, lp)))
            return out, [("vlin refusal", out[0], ("refused", E_STATE))]
        got = []

        def run():
            got.append(c.linearize_voxels(T, lp, debug=True))
            return dump(got[0], vxs.DUMP_KEYS) + sums(got[0]) + [("plain." + k, v) for k, v in sums(c.linearize_voxels(T, lp))]
        out = refusal(run)
        mod = [("vlin refusal", out[0][0] == "refused", False)]
        if got:                                                      # h:1128-1144: the dump is bitwise the rule's, from what the model knows
            normals = c.kept_source_normals()[0] if mode else None   # (the normals the context itself returns: the rule starts from them)
            scale = m.opts["gicp_robust_scale"] if m.opts["robust_kernel"] else 1.0
            want = vlin_of(m.vmap(), m.src, T, mode, normals, m.opts["gicp_epsilon"], m.opts["robust_kernel"], scale)
            mod += [("vlin dump " + k, S.same_bits(np.asarray(got[0][k]), np.asarray(want[k])), True) for k in vxs.DUMP_KEYS]
            mod += [("vlin " + k, int(got[0][k]), int(want[k])) for k in ("n_eff", "n_pt")]
        return out, mod
    if kind == "icp_v":
        if not m.voxels_ready():
            return [], []
        res, logs = c.icp_run_voxels(T, "Ours", cfg_of())
        return fields(res, TIMING) + records(logs), []
    if kind == "frames_v":
        if m.map is None or not m.vm:
            return [], []
        keys = frame_keys((257, 63, 1000))
        out = records(c.register_frames_voxels(frames_of(keys), frame_poses(3, pose), "Ours", cfg_of(),
                                               frame_normals=np_params((5, 0.0)) if mode else None, slots=2))
        m.loaded(keys, ("keep", (5, 0.0)) if mode else None)         # (the probe's own load: h:1402-1403, h:1396-1397)
        return out, []
    if kind == "trials_v":
        if not m.voxels_ready():
            return [], []
        return records(c.icp_run_trials_voxels(frame_poses(4, pose), "Ours", cfg_of())), []
    if kind == "vbatch":
        # the loaded frames and their kept normals, and the own source, through the fourth engine's device seam (d:246-261)
        if not (m.map is not None and m.vm and m.frames and (not mode or m.fn)):
            return [], []
        ids = [f for f, k in enumerate(m.frames) if len(cloud(k)) > 0]
        out = [("vbatch[%d].%s" % (f, k), v) for f, d in enumerate(c.voxels_batch(frame_poses(len(ids), pose), frame_ids=ids, params=lp)) for k, v in sums(d)]
        if m.src is not None and (not mode or m.sn):
            out += [("vbatch own[%d].%s" % (f, k), v) for f, d in enumerate(c.voxels_batch(frame_poses(2, pose), frame_ids=None, params=lp)) for k, v in sums(d)]
        return out, []
    if kind == "pairs":
        # two small pairs through the three pair forms: they need nothing of the context and leave it alone (h:1422-1423, h:1443-1446)
        src, tgt = [cloud(("frame", 63)), cloud(("frame", 257))], [cloud(("tgt", 600)), cloud(("tgt", 1500))]
        Ts, p5 = frame_poses(2, pose), np_params((5, 0.0))
        return ([("pairs." + k, v) for k, v in records(c.register_pairs(src, tgt, Ts, "Ours", cfg_of(), slots=2))] +
                [("pairs_n." + k, v) for k, v in records(c.register_pairs_normals(src, tgt, Ts, "Ours", cfg_of(), p5, slots=2))] +
                [("pairs_g." + k, v) for k, v in records(c.register_pairs_gicp(src, tgt, Ts, "Ours", cfg_of(), p5, p5, slots=2))]), []
    if kind == "desc":
        # the map form of the descriptors (h:1683-1687): from the map's own index and the kept normals, whatever updates made of either
        kp, rp = api.fpfh_params(k=9, search_radius=0.7), api.fpfh_radius_params(0.9, 30)
        got = []

        def run():
            got.extend([c.target_fpfh(kp), c.target_fpfh_radius(rp)])
            return [("target_fpfh", frozen(got[0])), ("target_fpfh_radius", frozen(got[1]))]
        out = refusal(run)
        mod = [("desc refusal", out[0] == ("refused", E_STATE), m.map is None or not m.tn)]       # h:1690-1691 no target or no kept normals
        if got and m.tn[0] == "set":                                 # given normals: the cloud form of (map, normals) is the same call (h:1683-1685)
            given = np.ascontiguousarray(m.tn[1][:, :3])
            f, _, info = c.fpfh(m.map, given, params=kp)
            mod.append(("cloud form fpfh", frozen((f, info)), frozen(got[0])))
            f, _, info = c.fpfh_radius(m.map, given, params=rp)
            mod.append(("cloud form fpfh_radius", frozen((f, info)), frozen(got[1])))
        return out, mod
    raise KeyError(kind)


def build_fresh(make, m):
    """context B, from the model alone: options, set_target, set_source, the normals by keep with the remembered parameters or by set with
    the array, the kept voxels (before any launch: the whole map's index is the active one), frames_load and the frame normals, the
    places, the keyframes"""
    b = make()
    for k in sorted(m.opts):
        b.set_option(k, m.opts[k])
    if m.map is not None:
        b.set_target(m.map, m.radius)
    if m.src is not None:
        b.set_source(m.src)
    for what, keep, given in ((m.tn, b.keep_target_normals, b.set_target_normals), (m.sn, b.keep_source_normals, b.set_source_normals)):
        if what:
            keep(np_params(what[1])) if what[0] == "keep" else given(what[1])
    if m.vm:
        b.keep_target_voxels(api.voxel_map_params(*m.vm))
    if m.frames:
        b.frames_load(frames_of(m.frames))
        if m.fn:
            b.frames_normals_keep(np_params(m.fn[1])) if m.fn[0] == "keep" else b.frames_normals_set(m.fn[1])
    if m.places is not None:
        b.places_reset(api.place_params(**PLACE))
        if m.places:
            b.places_add_clouds(list(m.places))
    if m.kf is not None:
        b.keyframes_reset()
        if m.kf:
            b.keyframes_add(list(m.kf))
    return b


def check_points(ops, every):
    """the steps after which A is compared: every `every`-th step of a state-changing class, and always the last"""
    n, out = 0, []
    for s, (name, _) in enumerate(ops):
        if CLASS[name] in STATE_CLASSES:
            n += 1
            if n % every == 0:
                out.append(s)
    return sorted(set(out + [len(ops) - 1]))


def probes_at(seed, step, last):
    """the map and the flags (host reads and one index check) at every check, three more probes drawn by the seed (two of thirteen kinds
    once, three of twenty-one now: the same share), all of them at the last step"""
    if last:
        return [(k, (step + j) % 6) for j, k in enumerate(PROBE_KINDS)]
    rng = np.random.default_rng([seed, step])
    kinds = 2 + rng.choice(len(PROBE_KINDS) - 2, size=3, replace=False)
    return [("map", 0), ("flags", 0)] + [(PROBE_KINDS[int(k)], int(rng.integers(6))) for k in kinds]


def first_difference(a, b):
    ka, kb = [k for k, _ in a], [k for k, _ in b]
    if ka != kb:
        return "keys %r != %r" % (ka, kb)
    for (k, x), (_, y) in zip(a, b):
        if x != y:
            return k
    return None


def run_walk(make, seed, ops, every, deskew=host_deskew, on_check=None, make_fresh=None):
    """A takes the walk; at every check point a fresh B is built from the model and both answer the probes"""
    a, m = make(), Model(deskew)
    m.fresh = make_fresh or make
    m.fresh_tag = getattr(m.fresh, "__name__", "context")
    checks = set(check_points(ops, every))
    try:
        for s, step in enumerate(ops):
            def where(what):
                return "seed %r, step %d, %s\nreplay(ctx, %r)" % (seed, s, what, ops[:s + 1])
            try:
                rc = apply(m, a, step)
            except Unexpected as e:                                  # (not an AssertionError: the caller stops its other walks)
                raise Unexpected(where("%r: %s" % (step, e))) from None
            except AssertionError as e:                              # (an accepted call whose own answer is not the model's)
                raise AssertionError(where("%r: %s" % (step, e))) from None
            assert rc is not None, where("precondition")
            if s not in checks or m.gate:
                continue
            last = s == len(ops) - 1
            b, mb = build_fresh(make_fresh or make, m), clone(m)
            try:
                for kind, pose in probes_at(seed, s, last):
                    ga, ma = probe(kind, a, m, pose)
                    gb, mbm = probe(kind, b, mb, pose, fresh=True)
                    for key, got, exp in ma:
                        assert got == exp, where("probe %s of the walked context against the model: %s" % (kind, key))
                    for key, got, exp in mbm:
                        assert got == exp, where("probe %s of the fresh context against the model: %s" % (kind, key))
                    d = first_difference(ga, gb)
                    assert d is None, where("probe %s at pose %d: first differing key %s" % (kind, pose, d))
                    if on_check:
                        on_check(s, kind, m, bool(ga or ma))
            finally:
                b.close()
    finally:
        a.close()
    return m


# ---- a context that is nothing but the header's state rules: its answers are hashes of exactly the state an answer may depend on.
# FAULTS plants one broken rule at a time (tests/test_state_walk_model.py: the committed seeds must catch each).
FAULTS = ("set_source_voxel keeps the source normals", "crop without normals_follow keeps the target normals",
          "insert_source leaves the window's answers those of the old map", "a refused set_target forgets the source",
          "frames_load keeps the frame normals", "a crop with normals_follow on keeps the kept voxels",
          "keep_target_voxels behind a live window summarises the window's points",
          "register_frames_voxels in mode 0 keeps the previous frames' normals",
          "robust_kernel is latched by set_source instead of being read at the launch",
          "an insert with normals_follow on leaves the map's descriptors those of the old map",
          "consensus_correspondences reads the used pairs the sampler left behind")


class FakeError(api.DcregError):
    def __init__(self, rc):
        super().__init__("fake call failed (%d)" % rc)


class _Rec(C.Structure):
    _fields_ = [("h", C.c_char * 16)]


class FakeContext:
    def __init__(self, fault=None, deskew=host_deskew):
        self.fault, self.deskew = fault, deskew
        self.opts = dict(DEFAULTS)
        self.map = self.src = self.tn = self.sn = self.frames = self.fn = self.places = self.kf = None
        self.gate, self.follow_n, self.window_map = False, 0, None
        self.vm = None                          # ((leaf, epsilon, min_points), the points the keep summarised)
        self.window_active = False              # the window is the active index: the last launch was a single-pose one of the first engine
        self.latched_kernel = 0                 # (FAULTS[8])
        self.desc_map = None                    # (FAULTS[9]) the map the descriptors still see
        self.left_used = None                   # (FAULTS[10]) the used pairs of the last align_correspondences

    def close(self):
        pass

    # what the second / third and fourth engine's answers may depend on beyond the clouds and the kept members
    def _robust(self, engine):
        """the kernel, and the engine's own scale only when a kernel is on (h:1058, h:1071)"""
        kind = self.latched_kernel if self.fault == FAULTS[8] else self.opts["robust_kernel"]
        return (kind, self.opts["robust_scale" if engine == 2 else "gicp_robust_scale"]) if kind else (0,)

    def _gicp(self):
        return self._robust(3) + (self.opts["gicp_epsilon"],)        # h:182-183 read at the time of every linearisation

    def _vox(self, normals):
        """the fourth engine: the kept voxels, the mode, the kernel and, in mode 1 only, gicp_epsilon and the cloud's kept normals (h:1129-1133)"""
        mode = self.opts["voxels_source_cov"]
        return (digest(self.vm[0], self.vm[1]), mode) + self._robust(4) + ((self.opts["gicp_epsilon"], normals) if mode else ())

    def _whole(self):
        """an entry point that is not a single-pose launch of the first engine makes the whole map's index the active one"""
        self.window_active = False

    def _busy(self):
        if self.gate:
            raise FakeError(E_STATE)

    def _need(self, *things):
        if any(t is None or t is False for t in things):
            raise FakeError(E_STATE)

    @staticmethod
    def _finite(xyz):
        xyz = np.asarray(xyz)
        if xyz.ndim != 2 or xyz.shape[1] < 3 or len(xyz) == 0 or not np.isfinite(xyz[:, :3]).all():
            raise FakeError(E_INVALID)
        return np.ascontiguousarray(xyz[:, :3], np.float32)

    def set_option(self, k, v):
        if (k, v) in REFUSED_OPTIONS:
            raise FakeError(E_INVALID)
        self.opts[k] = 1 << 20 if k == "max_table_entries" and v < (1 << 20) else v
        if k.startswith("roi_"):
            self.window_map = None              # (context.hip: the window is rebuilt by the next single-pose launch)

    # the map
    def _new_target(self, xyz):
        self.map, self.tn, self.follow_n, self.window_map, self.vm, self.window_active = xyz, None, 0, None, None, False
        self.desc_map = None

    def set_target(self, xyz, radius):
        self._busy()
        try:
            self._new_target(self._finite(xyz))
        except FakeError:
            if self.fault == FAULTS[3]:
                self.src = self.sn = None
            raise

    def set_target_voxel(self, xyz, radius, leaf):
        self._busy()
        self._new_target(self._finite(voxel_of(xyz, leaf)))

    def set_target_outliers(self, xyz, radius, p):
        self._busy()
        self._new_target(self._finite(outliers_kept(xyz, _outlier_dict(p))))

    def set_target_keyframes(self, members, radius, leaf=None):
        self._busy()
        self._need(self.kf)
        if any(i >= len(self.kf) for i, _ in members):
            raise FakeError(E_INVALID)
        self._new_target(self._finite(kr.submaps_ref(self.kf, [members], leaf)[0][0]))

    def _update(self, xyz, keep_window=False, keep_normals=False, keep_voxels=False, stale_desc=False):
        if len(xyz) == 0:
            raise FakeError(E_INVALID)
        if len(xyz) == len(self.map) and np.array_equal(xyz.view(np.uint32), self.map.view(np.uint32)):
            return
        follows = self.tn and self.tn[0] == "keep" and self.opts["normals_follow"]
        self.desc_map = (self.map if self.desc_map is None else self.desc_map) if stale_desc and follows else None
        if not keep_window:
            self.window_map = None
        if not keep_voxels:
            self.vm = None
        self.window_active = False
        self.map, self.follow_n = np.ascontiguousarray(xyz), len(xyz)
        follows = self.tn and self.tn[0] == "keep" and self.opts["normals_follow"]
        if not follows and not keep_normals:
            self.tn = None

    def insert(self, xyz, T, min_spacing=0.0):
        self._busy()
        self._need(self.map)
        q = transform(self._finite(xyz), T)
        self._update(np.concatenate([self.map, thinned(self.map, q, min_spacing)]), stale_desc=self.fault == FAULTS[9])

    def insert_source(self, T, min_spacing=0.0):
        self._busy()
        self._need(self.map, self.src)
        self._update(np.concatenate([self.map, thinned(self.map, transform(self.src, T), min_spacing)]), keep_window=self.fault == FAULTS[2],
                     stale_desc=self.fault == FAULTS[9])

    def crop(self, lo, hi):
        self._busy()
        self._need(self.map)
        self._update(crop_ref(self.map, lo, hi), keep_normals=self.fault == FAULTS[1],
                     keep_voxels=self.fault == FAULTS[5] and bool(self.opts["normals_follow"]))

    def remove_outliers(self, p):
        self._busy()
        self._need(self.map)
        self._update(outliers_kept(self.map, _outlier_dict(p)))

    def remove_dynamic(self, members, p):
        self._busy()
        self._need(self.kf, self.map)
        self._update(visibility_kept(self.map, self.kf, members, _vis_dict(p)))

    # the source
    def _new_source(self, xyz, keep_normals=False):
        self.src = xyz
        self.latched_kernel = self.opts["robust_kernel"]
        if not keep_normals:
            self.sn = None

    def set_source(self, xyz):
        self._busy()
        self._new_source(self._finite(xyz))

    def set_source_voxel(self, xyz, leaf):
        self._busy()
        self._new_source(self._finite(voxel_of(xyz, leaf)), keep_normals=self.fault == FAULTS[0])

    def set_source_outliers(self, xyz, p):
        self._busy()
        self._new_source(self._finite(outliers_kept(xyz, _outlier_dict(p))))

    def set_source_deskew(self, rec, field, motion):
        self._busy()
        self._new_source(self._finite(self.deskew(False, rec)))

    def set_source_deskew_path(self, rec, field, st, P, block):
        self._busy()
        self._new_source(self._finite(self.deskew(True, rec)))

    # normals: a kept set is named by what it was computed from
    def keep_target_normals(self, p):
        self._busy()
        self._need(self.map)
        self.tn = ("keep", (p.k, p.search_radius))

    def set_target_normals(self, a):
        self._busy()
        self._need(self.map)
        if len(a) != len(self.map):
            raise FakeError(E_INVALID)
        self.tn = ("set", np.array(a))

    def drop_target_normals(self):
        self.tn = None

    def keep_source_normals(self, p):
        self._busy()
        self._need(self.src)
        self.sn = ("keep", (p.k, p.search_radius), digest(self.src))

    def set_source_normals(self, a):
        self._busy()
        self._need(self.src)
        if len(a) != len(self.src):
            raise FakeError(E_INVALID)
        self.sn = ("set", np.array(a))

    def drop_source_normals(self):
        self.sn = None

    def target_normals_kept(self):
        return int(bool(self.tn))

    def source_normals_kept(self):
        return int(bool(self.sn))

    def frames_normals_kept(self):
        return int(bool(self.fn))

    def normals_follow_info(self):
        return {"n_target": self.follow_n}

    def _tn(self):
        return None if not self.tn else digest("keep", self.tn[1], self.map) if self.tn[0] == "keep" else digest("set", self.tn[1])

    def _sn(self):
        return None if not self.sn else digest(*self.sn)

    def kept_target_normals(self):
        if self.tn and self.tn[0] == "set":
            return np.ascontiguousarray(self.tn[1][:, :3]), np.full(len(self.map), np.nan, np.float32)
        return np.frombuffer(self._tn().encode(), np.uint8), np.zeros(1)

    def kept_source_normals(self):
        if self.sn[0] == "set":
            return np.ascontiguousarray(self.sn[1][:, :3]), np.full(len(self.src), np.nan, np.float32)
        # kept by the rule: unit vectors named by what they were computed from (the voxel linearisation below starts from them)
        return np.array(S.unit_normals(len(self.src), int(self._sn(), 16) % (1 << 31))), np.zeros(len(self.src), np.float32)

    # the kept voxels: the reference's records of the points the keep summarised
    def keep_target_voxels(self, p):
        self._busy()
        self._need(self.map)
        p = (p.leaf, p.epsilon, p.min_points)
        if spans_too_far(self.map, p[0]):
            raise FakeError(E_INVALID)
        pts = self.map
        if self.fault == FAULTS[6] and self.window_active:
            pts = np.ascontiguousarray(self.map[:(len(self.map) + 1) // 2])      # (a stand-in for the points inside the window's box)
        ref = vmap_of(pts, p)
        self.vm = (p, pts) if ref["n_kept"] else None
        return {k: ref[k] for k in ("n_points", "n_voxels", "n_small", "n_degenerate", "n_kept")}

    def drop_target_voxels(self):
        self._busy()
        self.vm = None

    def target_voxels_kept(self):
        return vmap_of(self.vm[1], self.vm[0])["n_kept"] if self.vm else 0

    def kept_target_voxels(self):
        self._busy()
        self._need(self.vm)
        return vmap_of(self.vm[1], self.vm[0])

    # frames
    def frames_load(self, frames, keep_normals=False):
        self._busy()
        if self.fault != FAULTS[4] and not keep_normals:
            self.fn = None
        for f in frames:
            if len(f):
                self._finite(f)
        self.frames = [np.ascontiguousarray(f[:, :3]) for f in frames]

    def frames_normals_keep(self, p):
        self._busy()
        self._need(self.frames)
        self.fn = ("keep", (p.k, p.search_radius), digest(*self.frames))

    def frames_normals_set(self, a):
        self._busy()
        self._need(self.frames)
        if len(a) != sum(len(f) for f in self.frames):
            raise FakeError(E_INVALID)
        self.fn = ("set", np.array(a))

    # places and keyframes
    def places_reset(self, p):
        self._busy()
        self.places = []

    def places_add_clouds(self, clouds):
        self._busy()
        self.places += [digest(x) for x in clouds]

    def places_add_source(self):
        self._busy()
        self._need(self.src)
        self.places.append(digest(self.src))

    def places_count(self):
        return len(self.places or [])

    def places_query_source(self, k=1):
        self._busy()
        self._need(self.src)
        return np.frombuffer(digest(self.src, self.places, k).encode(), np.uint8), np.zeros(1), np.zeros(1), {}

    def keyframes_reset(self):
        self._busy()
        self.kf = []

    def keyframes_add(self, clouds):
        self._busy()
        self._need(self.kf)
        self.kf += [self._finite(x) for x in clouds]

    def keyframes_add_source(self):
        self._busy()
        self._need(self.kf, self.src)
        self.kf.append(self.src)

    def keyframes_count(self):
        return len(self.kf or [])

    def keyframe_submaps(self, members, leaf=None):
        self._busy()
        return [np.frombuffer(digest(leaf, [(i, digest(T), digest(self.kf[i])) for i, T in sub]).encode(), np.uint8) for sub in members], {}

    # states and scratch users: nothing an answer may depend on
    def reserve_warm_states(self, n):
        self._busy()

    def reset_warm_state(self, i):
        self._busy()

    def voxel_downsample(self, *a):
        self._busy()

    normals = normals_clouds = outlier_filter = visibility_filter = place_descriptors = voxel_downsample

    # the chain: an answer is named by its inputs (h:1674-1675, h:1786-1790, h:1847-1848, h:1924-1925)
    @staticmethod
    def _normals_id(xyz, normals, np_):
        return digest("keep", (np_.k, np_.search_radius), xyz) if normals is None else digest("set", np.ascontiguousarray(np.asarray(normals)[:, :3]))

    @staticmethod
    def _desc(rule, xyz, normals_id, p):
        p = (p.k, p.search_radius) if rule == "k" else (p.radius, p.max_neighbors)
        return np.frombuffer(digest(rule, np.ascontiguousarray(xyz), normals_id, p).encode(), np.uint8)

    def fpfh(self, xyz, normals=None, normal_params=None, params=None, want_normals=False):
        self._busy()
        nid = self._normals_id(xyz, normals, normal_params)
        return self._desc("k", xyz, nid, params), (np.frombuffer(nid.encode(), np.uint8) if want_normals else None), {}

    def fpfh_radius(self, xyz, normals=None, normal_params=None, params=None, want_normals=False):
        self._busy()
        nid = self._normals_id(xyz, normals, normal_params)
        return self._desc("radius", xyz, nid, params), (np.frombuffer(nid.encode(), np.uint8) if want_normals else None), {}

    def _target_desc(self, rule, p):
        """the map form: the map and its kept normals - a kept set is named by the map it was computed from, a given one by itself"""
        self._busy()
        self._need(self.map, self.tn or None)
        seen = self.map if self.desc_map is None else self.desc_map
        nid = digest("keep", self.tn[1], seen) if self.tn[0] == "keep" else digest("set", np.ascontiguousarray(self.tn[1][:, :3]))
        return self._desc(rule, seen, nid, p), {}

    def target_fpfh(self, p):
        return self._target_desc("k", p)

    def target_fpfh_radius(self, p):
        return self._target_desc("radius", p)

    def feature_match(self, a, b, want_second=True, want_mutual=True):
        self._busy()
        return {"idx": np.frombuffer(digest(a, b).encode(), np.uint8)}

    @staticmethod
    def _block(p):
        return [(f[0], getattr(p, f[0])) for f in p._fields_ if not f[0].startswith("reserved")]

    def align_correspondences(self, a, b, corr_a, corr_b, params=None, want_mask=True):
        self._busy()
        self.left_used = digest(a, b, corr_a, corr_b)
        return {"records": np.frombuffer(digest(a, b, corr_a, corr_b, self._block(params)).encode(), np.uint8)}

    def consensus_correspondences(self, a, b, corr_a, corr_b, params=None, want_mask=True, want_members=False, want_weights=False):
        self._busy()
        left = self.left_used if self.fault == FAULTS[10] else None
        return {"records": np.frombuffer(digest(a, b, corr_a, corr_b, self._block(params), left).encode(), np.uint8)}

    # answers
    def target_points(self):
        return self.map

    def index_info(self):
        class I:
            n_target, n_source = (0 if self.map is None else len(self.map)), (0 if self.src is None else len(self.src))
        return I

    def index_check(self):
        return {"points": 0, "table": 0, "row_words": 0, "gap": 0, "owner": 0}

    def _pose(self, *T):
        for t in T:
            if not np.isfinite(np.asarray(t, np.float64)).all():
                raise FakeError(E_INVALID)
        return digest(*[np.asarray(t, np.float64) for t in T])

    def _lin(self, pose):
        """a single-pose launch of the first engine searches through the window when there is one (h:182-188)"""
        if self.opts["roi_index"] == 2 and self.window_map is None:
            self.window_map = self.map
        self.window_active = self.opts["roi_index"] == 2
        seen = self.window_map if self.opts["roi_index"] == 2 else self.map
        return digest(seen, self.src, pose)

    def linearize(self, R, t, lp=None, debug=False):
        self._busy()
        self._need(self.map, self.src)
        h = np.frombuffer(self._lin(self._pose(R, t)).encode(), np.uint8)
        return dict(nn_idx=h, nn_d2=h, flag=h, normal=h, r=h, s=h, H_upper=h, g=h, sum_r2=0.0, sum_b2=0.0, n_eff=0, n_pt=0)

    def _sums(self, *parts):
        h = np.frombuffer(digest(*parts).encode(), np.uint8)
        return dict(H_upper=h, g=h, sum_r2=0.0, sum_b2=0.0, n_eff=0, n_pt=0)

    def linearize_normals(self, T, lp=None):
        self._busy()
        self._need(self.map, self.src, self.tn or None)
        return self._sums(self.map, self.src, self._tn(), self._robust(2), self._pose(T))

    def linearize_gicp(self, T, lp=None):
        self._busy()
        self._need(self.map, self.src, self.tn or None, self.sn or None)
        return self._sums(self.map, self.src, self._tn(), self._sn(), self._gicp(), self._pose(T))

    def _need_voxels(self):
        self._need(self.map, self.src, self.vm, (self.sn or None) if self.opts["voxels_source_cov"] else True)

    def linearize_voxels(self, T, lp=None, debug=False):
        """the rule itself (tests/voxels_ref.py) from what this context holds: the dump can be compared with the model's"""
        self._busy()
        self._pose(T)
        self._need_voxels()
        mode, kind = self.opts["voxels_source_cov"], self._robust(4)
        return vlin_of(vmap_of(self.vm[1], self.vm[0]), self.src, T, mode, self.kept_source_normals()[0] if mode else None,
                       self.opts["gicp_epsilon"], kind[0], kind[1] if kind[0] else 1.0)

    def _rec(self, *parts):
        r = _Rec()
        r.h = digest(*parts).encode()
        return r

    def icp_run(self, T, method, cfg):
        self._busy()
        self._need(self.map, self.src)
        return self._rec(self._lin(self._pose(T))), []

    def icp_run_normals(self, T, method, cfg):
        self._busy()
        self._need(self.map, self.src, self.tn or None)
        return self._rec(self.map, self.src, self._tn(), self._robust(2), self._pose(T)), []

    def icp_run_gicp(self, T, method, cfg):
        self._busy()
        self._need(self.map, self.src, self.tn or None, self.sn or None)
        return self._rec(self.map, self.src, self._tn(), self._sn(), self._gicp(), self._pose(T)), []

    def icp_run_voxels(self, T, method, cfg):
        self._busy()
        self._need_voxels()
        return self._rec(self.src, self._vox(self._sn()), self._pose(T)), []

    def icp_run_trials(self, Ts, method, cfg):
        self._busy()
        self._need(self.map, self.src)
        self._whole()
        return [self._rec(self.map, self.src, self._pose(T)) for T in Ts]

    def icp_run_trials_normals(self, Ts, method, cfg):
        self._busy()
        self._need(self.map, self.src, self.tn or None)
        return [self._rec(self.map, self.src, self._tn(), self._robust(2), self._pose(T)) for T in Ts]

    def icp_run_trials_gicp(self, Ts, method, cfg):
        self._busy()
        self._need(self.map, self.src, self.tn or None, self.sn or None)
        return [self._rec(self.map, self.src, self._tn(), self._sn(), self._gicp(), self._pose(T)) for T in Ts]

    def icp_run_trials_voxels(self, Ts, method, cfg):
        self._busy()
        self._need_voxels()
        return [self._rec(self.src, self._vox(self._sn()), self._pose(T)) for T in Ts]

    def register_frames(self, frames, Ts, method, cfg, slots=0):
        self._busy()
        self._need(self.map)
        self.frames_load(frames)
        self._whole()
        return [self._rec(self.map, f, self._pose(T)) for f, T in zip(frames, Ts)]

    def register_frames_normals(self, frames, Ts, method, cfg, slots=0):
        self._busy()
        self._need(self.map, self.tn or None)
        self.frames_load(frames)
        return [self._rec(self.map, self._tn(), f, self._robust(2), self._pose(T)) for f, T in zip(frames, Ts)]

    def register_frames_gicp(self, frames, Ts, method, cfg, p=None, slots=0):
        self._busy()
        self._need(self.map, self.tn or None)
        self.frames_load(frames)
        self.frames_normals_keep(p)
        return [self._rec(self.map, self._tn(), f, p.k, self._gicp(), self._pose(T)) for f, T in zip(frames, Ts)]

    def register_frames_voxels(self, frames, Ts, method, cfg, frame_normals=None, slots=0):
        self._busy()
        self._need(self.map, self.vm)
        mode = self.opts["voxels_source_cov"]
        self.frames_load(frames, keep_normals=self.fault == FAULTS[7] and not mode)
        if mode:
            self.frames_normals_keep(frame_normals)
        return [self._rec(f, self._vox(frame_normals.k if mode else None), self._pose(T)) for f, T in zip(frames, Ts)]

    def register_pairs(self, src, tgt, Ts, method, cfg, slots=0):
        self._busy()
        for x in list(src) + list(tgt):
            self._finite(x)
        return [self._rec(s, t, self._pose(T)) for s, t, T in zip(src, tgt, Ts)]

    def register_pairs_normals(self, src, tgt, Ts, method, cfg, target_normals=None, slots=0):
        self._busy()
        for x in list(src) + list(tgt):
            self._finite(x)
        return [self._rec(s, t, target_normals.k, self._robust(2), self._pose(T)) for s, t, T in zip(src, tgt, Ts)]

    def register_pairs_gicp(self, src, tgt, Ts, method, cfg, target_normals=None, source_normals=None, slots=0):
        self._busy()
        for x in list(src) + list(tgt):
            self._finite(x)
        return [self._rec(s, t, target_normals.k, source_normals.k, self._gicp(), self._pose(T)) for s, t, T in zip(src, tgt, Ts)]

    def normals_batch(self, Ts, frame_ids=None, params=None):
        self._busy()
        return [self._sums(self.map, self._tn(), self.frames[f], self._robust(2), self._pose(T)) for f, T in zip(frame_ids, Ts)]

    def gicp_batch(self, Ts, frame_ids=None, params=None):
        self._busy()
        fn = digest(*self.fn)
        return [self._sums(self.map, self._tn(), self.frames[f], fn, f, self._gicp(), self._pose(T)) for f, T in zip(frame_ids, Ts)]

    def voxels_batch(self, Ts, frame_ids=None, params=None):
        self._busy()
        self._need(self.map, self.vm)
        if frame_ids is None:
            self._need_voxels()
            return [self._sums(self.src, self._vox(self._sn()), self._pose(T)) for T in Ts]
        fn = digest(*self.fn) if self.opts["voxels_source_cov"] else None
        return [self._sums(self.frames[f], self._vox((fn, f)), self._pose(T)) for f, T in zip(frame_ids, Ts)]

    def knn(self, q, k=5, max_radius=0.0):
        self._busy()
        self._need(self.map)
        self._whole()
        h = np.frombuffer(digest(self.map, q, k, max_radius).encode(), np.uint8)
        return h, h

    def p2p_error(self, T, thr):
        self._busy()
        self._need(self.map, self.src)
        self._whole()
        return tuple(float(v) for v in np.frombuffer(digest(self.map, self.src, self._pose(T), thr).encode(), np.uint8)[:4])

    # the gate
    def linearize_gated_begin(self, lp=None):
        self._busy()
        self._need(self.map, self.src)
        self.gate = True

    def gate_abort(self):
        self.gate = False

    def gate_open(self, R, t):
        self._pose(R, t)
        self.gate = False

    def linearize_end(self, slot=0):
        return {}


def _outlier_dict(p):
    return (dict(mode="radius", radius=p.radius, min_neighbors=p.min_neighbors) if p.mode == 1 else
            dict(mode="statistical", k=p.k, std_mul=p.std_mul, search_radius=p.search_radius))


def _vis_dict(p):
    return {k: getattr(p, k) for k in ("rows", "cols", "elev_min", "elev_max", "min_range", "max_range", "margin_abs", "margin_rel", "window", "min_votes")}


# ---- the committed walks (tests/test_state_walk_model.py holds the conditions they were chosen to meet)
# (the first ten are as old as the module, the next five came with the fourth engine, the last four with the alignment chain: the ids stay)
SEEDS = (5, 6, 12, 13, 17, 18, 21, 22, 23, 27, 2, 7, 9, 33, 42, 173, 80, 59, 83)
N_STEPS = 72
EVERY = 1            # A is compared after every EVERY-th state-changing step
