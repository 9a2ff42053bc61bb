"""The batched forms of the second and third engine with a robust kernel on (Cauchy or Geman-McClure): dcreg_register_frames_normals /
_gicp, dcreg_icp_run_trials_normals / _gicp and dcreg_register_pairs_normals / _gicp return, record by record and bit for bit, what the
serial sequence of single calls returns on a context with the same three option values - and nothing of the options is cached in slots
or frames: the same call with the kernel off and then on gives today's records and then the kernel's."""
import functools

import numpy as np
import pytest

import gicp_scenes as gs
import helpers as h
import normal_icp_scenes as sc
import robust_scenes as rs
import test_gpu_frames_gicp as fg
import test_gpu_frames_normals as fn
import test_gpu_pairs_engines as pe
from dcreg_amd import api
from test_normal_icp_reference import cfg_pk01

pytestmark = pytest.mark.gpu

ENGINES = ["normals", "gicp"]
PARAMS_5 = api.normal_params(k=5)
SIZES = [200, 256, 301, 350, 417, 480, 512]
DIRTY = 3                                    # the contaminated frame's place among the eight


def cfg40():
    return cfg_pk01(max_iterations=40, use_weight_derivative=1)


def robust(c, kind):
    c.set_robust(kind, scale=rs.C_N, gicp_scale=rs.C_G)
    return c


@functools.lru_cache(maxsize=None)
def frames():
    """eight frames of 200 .. 523 points, the contaminated frame among them, each with a start pose of its own near INIT"""
    L = gs.lot()
    rng = np.random.default_rng(29)
    fr = [sc.sized_source(n) for n in SIZES]
    fr.insert(DIRTY, rs.contaminated()["src"])
    T0 = [sc.frozen(sc.offset(L["INIT"], *rng.uniform(-0.05, 0.05, 3), yaw=rng.uniform(-0.01, 0.01))) for _ in fr]
    return fr, T0


def context(engine, src=None):
    if engine == "normals":
        return fn.context(src)
    c = fg.context(src)
    if src is not None:
        c.keep_source_normals(PARAMS_5)
    return c


def serial(c, engine, frame, T, method, cfg):
    return fn.single_record(c, frame, T, method, cfg) if engine == "normals" else fg.single_record(c, frame, T, method, cfg, PARAMS_5)


def register(c, engine, fr, T0, method, cfg, slots):
    if engine == "normals":
        return c.register_frames_normals(fr, T0, method, cfg, slots=slots)
    return c.register_frames_gicp(fr, T0, method, cfg, PARAMS_5, slots=slots)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("kind", [2, 3])
def test_frames_are_bitwise_the_serial_loop_with_the_same_options(engine, kind):
    fr, T0 = frames()
    cfg = cfg40()
    c, d = robust(context(engine), kind), robust(context(engine), kind)
    try:
        want = [serial(d, engine, f, T, "Ours", cfg) for f, T in zip(fr, T0)]
        recs = register(c, engine, fr, T0, "Ours", cfg, 3)
        assert len(recs) == len(fr)
        for k, (tr, s) in enumerate(zip(recs, want)):
            h.assert_record(tr, s, (engine, kind, k))
        assert sum(s["status"] == 0 for s in want) >= 6 and max(s["iterations"] for s in want) > 2
        off = serial(robust(d, 0), engine, fr[DIRTY], T0[DIRTY], "Ours", cfg)          # the kernel is in the records
        assert not np.array_equal(off["H"], want[DIRTY]["H"]) and not np.array_equal(off["T"], want[DIRTY]["T"])
    finally:
        c.close(); d.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_trials_are_bitwise_single_runs_with_the_same_options(engine):
    L = gs.lot()
    rng = np.random.default_rng(31)
    T0 = [sc.offset(L["INIT"], *rng.uniform(-0.08, 0.08, 3), yaw=rng.uniform(-0.02, 0.02)) for _ in range(6)]
    cfg = cfg40()
    src = rs.contaminated()["src"]
    c, d = robust(context(engine, src), 3), robust(context(engine, src), 3)
    try:
        run = c.icp_run_trials_normals if engine == "normals" else c.icp_run_trials_gicp
        recs = run(T0, "Ours", cfg)
        assert len(recs) == 6
        for k, (tr, T) in enumerate(zip(recs, T0)):
            h.assert_record(tr, serial(d, engine, None, T, "Ours", cfg), (engine, k))
        assert all(tr.status == 0 for tr in recs) and max(tr.iterations for tr in recs) > 2
    finally:
        c.close(); d.close()


@functools.lru_cache(maxsize=None)
def pairs():
    """four pairs: frames of frames() against crops of the lot of 500, 1000 and 2000 points around the frames' place, and the whole lot"""
    L = gs.lot()
    fr, T0 = frames()
    lot = np.ascontiguousarray(L["tgt"], np.float32)
    near = np.argsort(np.linalg.norm(lot.astype(np.float64) - L["GT"][:3, 3], axis=1), kind="stable")
    tgts = [sc.frozen(lot[np.sort(near[:n])].copy()) for n in (500, 1000, 2000)] + [lot]
    pick = [DIRTY, 0, 5, 7]
    return [fr[k] for k in pick], tgts, [T0[k] for k in pick]


@pytest.mark.parametrize("engine", ENGINES)
def test_pairs_are_bitwise_the_serial_sequence_with_the_same_options(engine):
    srcs, tgts, Ts = pairs()
    cfg = cfg40()
    c, d = robust(api.Context(0), 2), robust(api.Context(0), 2)
    try:
        want = [pe.serial_record(d, engine, s, t, T, "Ours", cfg) for s, t, T in zip(srcs, tgts, Ts)]
        pe.check(pe.call(c, engine, srcs, tgts, Ts, "Ours", cfg, 2), want)
        assert [len(t) for t in tgts] == [500, 1000, 2000, 4000]
        assert sum(s["status"] == 0 and s["iterations"] >= 2 for s in want) >= 3
        off = pe.serial_record(robust(d, 0), engine, srcs[0], tgts[3], Ts[0], "Ours", cfg)
        on = pe.serial_record(robust(d, 2), engine, srcs[0], tgts[3], Ts[0], "Ours", cfg)
        assert not np.array_equal(off["H"], on["H"])
    finally:
        c.close(); d.close()


def test_the_same_call_with_the_kernel_off_and_then_on_caches_nothing():
    fr, T0 = frames()
    cfg = cfg40()
    c, plain, d = context("normals"), context("normals"), robust(context("normals"), 3)
    try:
        today = [serial(plain, "normals", f, T, "Ours", cfg) for f, T in zip(fr, T0)]          # a context that never heard of the options
        want3 = [serial(d, "normals", f, T, "Ours", cfg) for f, T in zip(fr, T0)]
        robust(c, 0)
        for k, (tr, s) in enumerate(zip(register(c, "normals", fr, T0, "Ours", cfg, 3), today)):
            h.assert_record(tr, s, ("off", k))
        robust(c, 3)
        for k, (tr, s) in enumerate(zip(register(c, "normals", fr, T0, "Ours", cfg, 3), want3)):
            h.assert_record(tr, s, ("on", k))
        robust(c, 0)
        for k, (tr, s) in enumerate(zip(register(c, "normals", fr, T0, "Ours", cfg, 3), today)):
            h.assert_record(tr, s, ("off again", k))
        assert any(not np.array_equal(a["H"], b["H"]) for a, b in zip(today, want3))
    finally:
        c.close(); plain.close(); d.close()
