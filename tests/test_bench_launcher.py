"""bench.py as the driver invokes it (`python bench.py --gpus N ...`, no external launcher): the script must spawn one
rank per GPU itself, refuse to report a smaller job under a bigger name, and gather one record per rank.
CPU part: DCREG_BENCH_DRYRUN=1 replaces the device work by a synthetic record so that launcher, rendezvous (gloo), fence,
max-over-ranks and gather run here.  GPU part (-m gpu): the real workload with two ranks sharing the box's one device over
gloo (control flow only; RCCL with one rank per GPU is what the 8-GPU node runs), both sharding modes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as h

BENCH = os.path.join(h.REPO, "bench.py")


def _bench(args, env_extra, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, BENCH] + args, cwd=h.REPO, env=env, capture_output=True, text=True, timeout=timeout)


def _json_line(p):
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])       # rank 0 prints ONE line
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_self_spawn_two_ranks_dry_run():
    p = _bench(["--gpus", "2", "--steps", "20", "--warmup", "5"], {"DCREG_BENCH_DRYRUN": "1", "DCREG_BENCH_BACKEND": "gloo"})
    assert p.returncode == 0, p.stderr[-2000:]
    j = _json_line(p)
    assert j["dry_run"] is True and j["n_gpus"] == 2 and j["steps"] == 20 and j["warmup"] == 5
    assert j["ranks"] == [0, 1] and j["rank_seeds"] == [100, 101]     # one record per rank, every rank its own pair
    assert all(t >= 0.02 for t in j["block_times_s"])                 # max over ranks: rank 1 sleeps twice as long as rank 0
    _check_c5_leg(j, 2)


def _check_c5_leg(j, world):
    """the strong-scaling leg of a multi-rank run: every trial of the 5000 ran on exactly one rank (k = rank mod world), the records of
    all ranks reached rank 0 through the one gather, the statistics are those of the whole experiment"""
    c5 = j["c5_montecarlo_5000"]
    assert c5["n_gpus"] == world and c5["scaling"] == "strong" and c5["trials"] == 5000 and c5["rccl_ranks_seen"] == world
    assert c5["iterations"] == sum(10 + k % 7 for k in range(5000)) and c5["converged_runs"] == sum(1 for k in range(5000) if k % 4)


@pytest.mark.timeout(600)
def test_self_spawn_eight_ranks_dry_run():
    """The shape the driver's scaling run has - `python bench.py --gpus 8` on one node: eight ranks rendezvous on 127.0.0.1, fence,
    take the max over ranks and gather one record each; every rank gets its own scan-pair seed and its share of the host's CPUs."""
    p = _bench(["--gpus", "8", "--steps", "20", "--warmup", "5"], {"DCREG_BENCH_DRYRUN": "1", "DCREG_BENCH_BACKEND": "gloo"}, timeout=550)
    assert p.returncode == 0, p.stderr[-2000:]
    j = _json_line(p)
    assert j["dry_run"] is True and j["n_gpus"] == 8
    assert j["ranks"] == list(range(8)) and j["rank_seeds"] == [100 + r for r in range(8)]
    assert all(t >= 0.08 for t in j["block_times_s"])                 # max over ranks: rank 7 sleeps 8 x 10 ms
    assert j["host_threads_per_rank"] >= 1 and len(set(j["host_threads"])) == 1 and j["host_threads"][0] == j["host_threads_per_rank"]
    # the share is taken from the CPUs the job was started with, not from a rank's slice of them
    from dcreg_amd import hostinfo
    assert j["host_threads_per_rank"] == hostinfo.threads_per_rank(8)
    _check_c5_leg(j, 8)


def test_refuses_a_job_it_cannot_run():
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than 2 devices")
    p = _bench(["--gpus", "2"], {})
    assert p.returncode != 0 and "--gpus 2 requested" in p.stderr and "{" not in p.stdout
    p = _bench(["--gpus", "2"], {"WORLD_SIZE": "4", "RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE=4" in p.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("sharding", ["pairs", "points"])
def test_two_ranks_on_one_device_real_workload(sharding):
    p = _bench(["--gpus", "2", "--steps", "20", "--warmup", "20", "--repeats", "3", "--min-seconds", "0", "--workload", "c2_cylinder_100k", "--sharding", sharding,
                "--no-cpu-baseline", "--no-configs", "--concurrent-pairs", "0"],
               {"DCREG_BENCH_BACKEND": "gloo", "DCREG_BENCH_LOCAL_RANK": "0"}, timeout=800)
    assert p.returncode == 0, p.stderr[-3000:]
    j = _json_line(p)
    assert j["n_gpus"] == 2 and j["steps"] == 20 and j["repeats"] == 3 and j["value"] > 0
    assert j["scaling"] == ("weak" if sharding == "pairs" else "strong")
    assert j["config"]["rank_pair_seeds"] == [100, 101]
    assert j["roofline"]["bound"] == "hbm" and 0 < j["roofline"]["frac"] < 1
    assert j["final_stats"]["mean_trans_error_m"] < 0.01
    if sharding == "points":                                          # every rank holds a slice: half the queries per launch
        assert j["roofline"]["algorithmic_bytes_per_launch"] == 72 * 50_000


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_two_ranks_run_the_montecarlo_experiment_as_one_job(tmp_path):
    """N > 1 without extra flags: after the weak-scaling measurement of the main workload the 5000-trial Monte-Carlo experiment runs ONCE
    across the ranks (trials k = rank mod N), its trial records are gathered inside the timed region and rank 0 takes the statistics -
    here with two ranks sharing the box's one device over gloo.  (The statistics are a sub-record of the leg: --full-record has them.)"""
    full = tmp_path / "record.json"
    p = _bench(["--gpus", "2", "--steps", "30", "--warmup", "30", "--repeats", "2", "--min-seconds", "0", "--workload", "c1_fixture_7562", "--no-cpu-baseline",
                "--concurrent-pairs", "0", "--full-record", str(full)], {"DCREG_BENCH_BACKEND": "gloo", "DCREG_BENCH_LOCAL_RANK": "0"}, timeout=800)
    assert p.returncode == 0, p.stderr[-3000:]
    j = _json_line(p)
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and list(j["configs"]) == ["c5_montecarlo_5000"] and "side_leg_errors" not in j
    c5 = json.loads(full.read_text())["configs"]["c5_montecarlo_5000"]
    assert j["configs"]["c5_montecarlo_5000"]["value"] == c5["value"]
    assert c5["n_gpus"] == 2 and c5["scaling"] == "strong" and c5["rccl_ranks_seen"] == 2
    st = c5["montecarlo"]["statistics"]
    assert st["total_runs"] == 5000 and 0.5 < st["success_rate"] < 0.95
    # all trials, not one rank's share: the iterations of one experiment
    assert 60_000 < c5["icp_iterations_per_step"] < 100_000 and c5["value"] > 0


def test_a_failing_montecarlo_job_becomes_an_error_record():
    """bench.py at N > 1 runs the Monte-Carlo leg as a job of its own (montecarlo_child): a job that fails - here because the box has fewer
    than two devices, so the child refuses to start - comes back as an error record for the JSON line, not as an exception that would take
    the headline measured before it along."""
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than 2 devices")
    sys.path.insert(0, h.REPO)
    import bench
    args = bench.parse_args(["--gpus", "2"])
    env_keep = {k: os.environ.pop(k) for k in ("DCREG_BENCH_BACKEND", "DCREG_BENCH_DRYRUN") if k in os.environ}
    try:
        rec = bench.montecarlo_child(args, 2, timeout_s=300.0)
    finally:
        os.environ.update(env_keep)
    assert "error" in rec and "rc" in rec["error"] and "--gpus 2 requested" in rec["stderr_tail"]


def test_the_line_stays_small_with_every_leg_failed():
    """The JSON line is all a reader of the command's output may get, and it keeps only the last few KB of it (a 30 KB line was left
    unparsed): LINE_BYTES = 4 KB, whether every leg succeeds (the committed record of a default run) or every leg fails with a long
    error - the run whose line matters most.  The headline numbers are in it unchanged, every leg's few numbers, every failure."""
    sys.path.insert(0, h.REPO)
    import bench
    assert bench.LINE_BYTES <= 4096
    full = json.load(open(os.path.join(h.REPO, "profiles", "r06_bench_line.json")))
    line = bench.compact_line(full)
    assert len(json.dumps(line)) <= bench.LINE_BYTES < len(json.dumps(full))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "repeats", "timed_seconds", "ms_per_step", "ms_per_step_median",
              "ms_per_step_min", "ms_per_step_max", "config", "final_stats", "host_threads"):
        assert line[k] == full[k], k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_us_avg", "algorithmic_bytes_per_launch"):
        assert line["roofline"][k] == full["roofline"][k], k
    assert line["roofline_valu_issue"]["frac"] == full["roofline_valu_issue"]["frac"]
    assert set(line["configs"]) == set(full["configs"])
    for name, rec in full["configs"].items():
        assert line["configs"][name] and all(line["configs"][name][k] == rec[k] for k in ("value", "ms_per_step", "ms_total") if k in rec), name
    assert line["cpu_baseline"]["value"] == full["cpu_baseline"]["value"]
    assert line["converged_run"]["iterations_per_s"] == full["converged_run"]["iterations_per_s"]
    assert line["concurrent_pairs"]["value"] == full["concurrent_pairs"]["value"]

    legs = list(full["configs"]) + ["roofline_by_regime", "converged_run", "cold_run", "concurrent_pairs", "cpu_baseline", "final_stats",
                                     "c5_by_host_threads"]
    err = {leg: "RuntimeError: dcreg_icp_run failed in %s: rc=-5 %s" % (leg, "x" * 300) for leg in legs}
    for leg in legs:
        if leg in full["configs"]:
            full["configs"][leg] = {"error": err[leg]}
        elif leg in full:
            full[leg] = {"error": err[leg]}
    full["side_leg_errors"] = err
    line = bench.compact_line(full)
    assert len(json.dumps(line)) <= bench.LINE_BYTES
    assert line["value"] == full["value"] and line["ms_per_step"] == full["ms_per_step"] and line["roofline"]["frac"] == full["roofline"]["frac"]
    assert set(line["side_leg_errors"]) == set(legs)
    assert all(err[leg].startswith(line["side_leg_errors"][leg]) and len(line["side_leg_errors"][leg]) >= 60 for leg in legs)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("workload", ["c1_fixture_7562", "c5_montecarlo_5000"])
def test_steps_are_the_timed_steps_and_the_dumped_outputs_are_the_results(workload, tmp_path):
    """--steps K times exactly K steps (one timed region) and ms_per_step is that region's time over K; --dump-outputs writes what the
    last timed step returned, in float64; the same arguments give the same outputs, bit for bit, and they are the results of the same
    work done here without bench.py: for the fixture pair the pose after 3 + 7 iterations from the bench's initial pose (the engine
    through the Python binding, and the CPU oracle), for the Monte-Carlo experiment the statistics the Python driver takes of its records."""
    args = ["--gpus", "1", "--steps", "7", "--warmup", "3", "--workload", workload, "--no-configs", "--no-regimes", "--no-cpu-baseline",
            "--concurrent-pairs", "0"]
    stats = ("total_runs", "converged_runs", "success_rate", "mean_trans_error", "std_trans_error", "min_trans_error", "max_trans_error",
             "mean_rot_error", "std_rot_error", "min_rot_error", "max_rot_error", "mean_iterations", "mean_rmse", "mean_fitness", "corr_num")
    expect = ({"R", "t", "icp_cov", "converged", "iterations", "status"} if workload == "c1_fixture_7562" else {"montecarlo_" + k for k in stats})
    dumps = []
    for run in range(2):
        out = tmp_path / ("run%d" % run)
        p = _bench(args + ["--dump-outputs", str(out)], {}, timeout=400)
        assert p.returncode == 0, p.stderr[-3000:]
        j = _json_line(p)
        assert j["steps"] == 7 and j["warmup"] == 3 and j["repeats"] == 1
        assert j["ms_per_step"] == pytest.approx(1e3 * j["timed_seconds"] / 7, rel=1e-12)
        arrays = {f.stem: np.load(f) for f in out.glob("*.npy")}
        assert set(arrays) == expect and all(a.dtype == np.float64 and np.isfinite(a).all() for a in arrays.values())
        dumps.append(arrays)
    for k in expect:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
    d = dumps[0]

    from dcreg_amd import api, montecarlo as mcm
    from oracle import pyoracle as po
    pts = h.cylinder_cloud()
    ctx = api.Context(0)
    try:
        ctx.set_target(pts, 1.0)
        ctx.set_source(pts)
        if workload == "c1_fixture_7562":
            T = h.pose6d_matrix(0.05, -0.08, 0.03, h.deg2rad(0.2), h.deg2rad(-0.1), h.deg2rad(0.5))   # bench.py's initial misalignment
            kw = dict(search_radius=1.0, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=0.0, CONVERGENCE_THRESH_TRANS=0.0,
                      use_weight_derivative=1, always_compute_schur=1)
            for n in (3, 7):                                              # warm-up, then the timed steps: two calls, as the bench makes them
                res, _ = ctx.icp_run(T, "Ours", api.default_config(max_iterations=n, **kw))
                T = np.eye(4); T[:3, :3] = np.array(res.R[:]).reshape(3, 3); T[:3, 3] = res.t[:]
            assert d["iterations"] == res.iterations == 7 and d["status"] == res.status == 0 and d["converged"] == res.converged == 0
            assert np.allclose(d["R"], T[:3, :3], rtol=0, atol=1e-12) and np.allclose(d["t"], T[:3, 3], rtol=0, atol=1e-12)
            assert np.allclose(d["icp_cov"], np.array(res.icp_cov[:]).reshape(6, 6), rtol=1e-12, atol=0)
            T0 = h.pose6d_matrix(0.05, -0.08, 0.03, h.deg2rad(0.2), h.deg2rad(-0.1), h.deg2rad(0.5))
            ocfg = po.default_config(search_radius=1.0, max_iterations=10, kappa_target=10.0, std_reg_gamma=100.0, thresh_rot=0.0,
                                     thresh_trans=0.0, use_weight_derivative=1, always_compute_schur=1, num_threads=8)
            ores, _ = po.icp_run(po.KdTree(pts), pts, T0, "Ours", ocfg)
            assert ores.iterations == 10
            assert np.allclose(d["R"], np.array(ores.R[:]).reshape(3, 3), rtol=0, atol=1e-8)
            assert np.allclose(d["t"], np.array(ores.t[:]), rtol=0, atol=1e-8)
            assert np.allclose(d["icp_cov"], np.array(ores.cov[:]).reshape(6, 6), rtol=1e-9, atol=0)
        else:
            cfg = api.default_config(search_radius=1.0, max_iterations=30, CONVERGENCE_THRESH_TRANS=1e-3, CONVERGENCE_THRESH_ROT=1e-5,
                                     KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, DEGENERACY_THRES_COND=10.0, DEGENERACY_THRES_EIG=120.0,
                                     use_weight_derivative=1, always_compute_schur=1)
            base = (0.2, 0.8, 0.5, h.deg2rad(0.1), h.deg2rad(0.1), h.deg2rad(2.0))
            _, want = mcm.run_montecarlo_native(ctx, "Ours", cfg, base, 5000, 2024, 0.5, np.deg2rad(2.0), slots=256)
            for k in stats:
                assert np.isclose(d["montecarlo_" + k], want[k], rtol=1e-12, atol=1e-300), (k, float(d["montecarlo_" + k]), want[k])
            assert d["montecarlo_total_runs"] == 5000
    finally:
        ctx.close()
