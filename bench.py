#!/usr/bin/env python
"""bench.py -- ICP iterations/s of the MI355X-native DCReg hot path (BASELINE.json metric).

A "step" is ONE ICP iteration of one scan pair: dcreg_linearize (exact 5-NN + plane fit + Jacobian/residual
+ J^T J / J^T r on the GPU, inputs resident in HBM) followed by the host 6x6 Schur analysis + PCG solve and
the SE(3) update -- exactly the reference's per-iteration loop body (icp_test_runner.cpp:1694-2004).

Default workload = BASELINE.json configs[3], the largest single-GPU configuration and the one the metric's roofline is
quoted on: 1 M x 1 M-point synthetic corridor, runs of 50 ICP iterations, method Ours (Schur detection + PCG).  The steps
are consecutive iterations of back-to-back 50-iteration runs from the same initial misalignment (a run's first iterations,
0.87 m off at the corridor ends, cost several times an aligned one: they are part of the workload and of `value`).  After
--warmup W iterations, exactly --steps K iterations are timed, as one region bracketed by barrier + synchronize (max over
ranks); --repeats R times that region R times and --min-seconds S repeats it until S seconds have been timed.  `value` = all
timed steps / all timed time, `ms_per_step` = the same mean, with median / min / max over the repeats alongside.  No HIP event is
recorded inside a timed region: `roofline.kernel_us_avg` comes from a separate, untimed pass over whole runs (kernel_pass).
--dump-outputs DIR writes what the last timed step returned to its caller (step_outputs) as DIR/<name>.npy; the inputs are seeded,
so two builds run with the same arguments can be compared output for output.
The other BASELINE configs (C1 fixture, C2 100 k cylinder, C3 PK01-like 200 k, C5 = the 5000-trial Monte-Carlo experiment end
to end) are measured briefly afterwards and reported under "configs", each with its own roofline block.

On the same line (N = 1): `roofline_by_regime` (every launch of a few whole runs timed with HIP events and bucketed by the fraction of
its points that went through the search - the launch reports it itself), `converged_run` (the same pair with the reference's
convergence thresholds on), `cold_run` (the same with the neighbour state dropped before every run = the reference's fresh
ICPContext per run, icp_test_runner.cpp:408-409), `configs.c3_pk01_8k_registration` (what ONE registration of an 8 k-point frame costs from host buffers:
dcreg_set_source + run to convergence, the reference's own metric, icp_test_runner.cpp:442-461) and the C5 experiment at 2 / 4 / all host
threads.

--gpus N: one process per GPU (RCCL); when not already under torch.distributed.run the script runs itself under it as a child process.
Every rank runs its own scan pair (weak scaling, no data-path collective) = `value`; then the 5000-trial Monte-Carlo experiment
(BASELINE configs[4]) is run ONCE across all ranks - trials k = rank mod N, the 64-double trial records gathered over RCCL inside the
timed region, statistics on rank 0 (icp_test_runner.cpp:604-664) - and reported as `configs.c5_montecarlo_5000` (strong scaling).
Rank 0 prints ONE JSON line: the headline and a few numbers per side leg, at most LINE_BYTES (compact_line); --full-record PATH writes
the whole record, the side legs' notes, lists and sub-records included, as JSON.
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
BYTES_PER_QUERY = 72           # 12 B source point + 5 x 12 B neighbours
N_SIMD, CLOCK_HZ = 1024, 2.4e9  # 256 CUs x 4 SIMDs, max shader clock (MI355X_MICROARCH.md)
MC_TRIALS, MC_SLOTS, MC_SEED = 5000, 256, 2024
MC_KERNEL_TIMING_STRIDE = 13   # kernel pass of the Monte-Carlo experiment: a HIP-event pair around every 13th batched launch (an event pair costs
                               # ~10 us of host time and the experiment is thousands of launches).  The kernel pass is a SEPARATE, untimed pass:
                               # no launch of the region `value` is computed from carries events (kernel_pass below)
LINE_BYTES = 4096              # compact_line: what the JSON line may take.  A reader of the command's output keeps only its last few KB
                               # (a 30 KB line was left unparsed), so the line stays well below that, failed legs included
LINE_STRING_CHARS = 32         # compact_line: the longest text of the roofline blocks the line carries (the prose goes to --full-record)
LINE_ERROR_CHARS = 80          # compact_line: the first characters of a failed leg's error (the whole text goes to --full-record)
LINE_LEG_KEYS = ("value", "ms_per_step", "ms_total", "iterations_per_s")   # what the line carries of a leg beside the headline

# name: scene, points, radius, iterations per ICP run, weight-derivative Jacobian, BASELINE config
WORKLOADS = {
    "c4_corridor_1m": dict(scene="corridor", n=1_000_000, radius=1.0, run_len=50, wd=1, cfg="configs[3]"),
    "c2_cylinder_100k": dict(scene="cylinder", n=100_000, radius=1.0, run_len=20, wd=1, cfg="configs[1]"),
    "c3_pk01_200k": dict(scene="parkinglot", n=200_000, radius=0.5, run_len=30, wd=0, cfg="configs[2] (stand-in, 200 k-point frame variant)"),
    "c1_fixture_7562": dict(scene="fixture", n=7562, radius=1.0, run_len=30, wd=1, cfg="configs[0]"),
    # Monte-Carlo: icp_iter.yaml's experiment as this build defines it (the reference has no RNG): 5000 trials of the fixture
    # pair from seeded initial poses, base = the paper run's, +-0.5 m / +-2 deg per DoF, max 30 iterations, convergence thresholds ON,
    # run by dcreg_icp_run_montecarlo with 256 trials in flight.  ONE step = the whole experiment of this GPU.
    "c5_montecarlo_5000": dict(scene="fixture", n=7562, radius=1.0, run_len=30, wd=1, cfg="configs[4] (one GPU's share = all 5000 trials at N = 1)"),
}


def make_pair(scene, n, seed):
    from dcreg_amd import scenes as h
    if scene == "fixture":
        pts = h.cylinder_cloud()
        return pts, pts.copy()
    if scene == "parkinglot":
        return h.scene_parkinglot(n_map=n, n_frame=n, seed=7 + seed - 100, frame_range=100.0)
    gen = {"cylinder": lambda: h.scene_cylinder(n, seed=seed, noise=0.01),
           "corridor": lambda: h.scene_corridor(n, seed=seed)}[scene]
    tgt = gen()
    rng = np.random.default_rng(seed + 1000)
    src = (tgt + rng.normal(0, 0.01, tgt.shape)).astype(np.float32)   # a second noisy scan of the same scene
    return tgt, src


def initial_pose(scene):
    from dcreg_amd import scenes as h
    if scene == "parkinglot":
        return h.pose6d_matrix(**h.PK01_INIT)          # config/icp_pk01.yaml:29-35
    # a few cm / tenths of a degree (frame-to-frame LiDAR odometry regime); over the 200 m corridor the 0.5 deg yaw is
    # 0.87 m at the ends
    return h.pose6d_matrix(0.05, -0.08, 0.03, h.deg2rad(0.2), h.deg2rad(-0.1), h.deg2rad(0.5))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=0, help="the timed region of --steps iterations is repeated this many times (0 = once, or as "
                                                             "often as --min-seconds asks)")
    ap.add_argument("--min-seconds", type=float, default=0.0,
                    help="headline only: repeat the timed region until at least this many seconds of it have been timed, so that a sampling "
                         "monitor around the command sees the device busy (each repeat is still exactly --steps steps between two fences); "
                         "0 (default) = --steps steps are timed, no more")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them returned to its caller (pose, covariance, run state; the "
                         "Monte-Carlo workload: the experiment's statistics) as DIR/<name>.npy in float64")
    ap.add_argument("--full-record", metavar="PATH", default=None,
                    help="also write the whole record as JSON to PATH: the JSON line carries the headline and only a few numbers per side "
                         "leg")
    ap.add_argument("--workload", default="c4_corridor_1m", choices=list(WORKLOADS))
    ap.add_argument("--method", default="Ours")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-configs", action="store_true", help="skip the brief measurements of the other BASELINE configs")
    ap.add_argument("--no-regimes", action="store_true", help="skip the per-regime roofline and the thresholds-on run of the main workload")
    ap.add_argument("--sharding", default="pairs", choices=["pairs", "points"],
                    help="pairs (default): one independent scan pair per GPU, no data-path collective, weak scaling; "
                         "points: ONE pair, source points split over the GPUs, one 256 B all_gather per iteration, strong scaling")
    ap.add_argument("--concurrent-pairs", type=int, default=2,
                    help="after the main (one pair at a time) measurement, also time P independent scan pairs running "
                         "CONCURRENTLY on this GPU (one context + stream + host thread each); 0 = skip")
    ap.add_argument("--prior-map-points", type=int, default=50_000_000,
                    help="configs.c3_prior_map_50m: one registration of an 8 k-point frame against a seeded prior map of this many points "
                         "(the regime of the reference's published timings); 0 = skip")
    ap.add_argument("--sub-record", action="store_true",
                    help="(internal) print the workload's summary record as the one JSON line and stop: how a job of N > 1 ranks obtains the "
                         "Monte-Carlo leg from a job of its own (montecarlo_child)")
    ap.add_argument("--prior-map-points-large", type=int, default=200_000_000,
                    help="configs.c3_prior_map_200m: the same registration against a 1.4 km x 1.4 km seeded map of this many points (the upper end of the "
                         "reference's published range; its dense cell table runs into the budget, so the frames are registered on the window index); 0 = skip")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE",
                    help="backend option (dcreg_set_option), e.g. --opt warm_start=0 --opt cell_factor=1.5 (ablations)")
    return ap.parse_args(argv)


def maybe_spawn(args):
    """`python bench.py --gpus N` with N > 1 outside a launcher: run the job under torch.distributed.run, one rank per GPU, as a child
    process, and exit with its status.
    Refuses (non-zero exit) when fewer than N devices are visible instead of reporting a smaller job as N GPUs."""
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is not None:
        if int(world_env) != args.gpus:
            sys.exit("bench.py: --gpus %d but WORLD_SIZE=%s: refusing to report a job of a different size" % (args.gpus, world_env))
        return
    if args.gpus <= 1:
        return
    shared = os.environ.get("DCREG_BENCH_BACKEND", "nccl") != "nccl"      # test hook: all ranks on one device over gloo
    if not shared and not os.environ.get("DCREG_BENCH_DRYRUN"):
        # counted in a child of its own: this process starts the ranks and must not have brought up the HIP runtime itself
        import subprocess
        p = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True)
        have = int(p.stdout.strip() or 0) if p.returncode == 0 else 0
        if have < args.gpus:
            sys.exit("bench.py: --gpus %d requested but only %d HIP device(s) visible; not running a smaller job under that name" % (args.gpus, have))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # torch.distributed.run pins OMP_NUM_THREADS=1 unless told otherwise; the Monte-Carlo path solves its 6x6 systems with OpenMP
    from dcreg_amd import hostinfo
    os.environ.setdefault("OMP_NUM_THREADS", str(hostinfo.threads_per_rank(args.gpus)))
    import subprocess
    rc = subprocess.run(cmd).returncode
    sys.exit(rc if rc >= 0 else 128 - rc)


class Dist:
    """torch.distributed plumbing: rank / world, the barrier + synchronize fence, max-over-ranks of a time."""

    def __init__(self):
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        # test hooks (control flow of the multi-rank path on a single-GPU box / on CPU): ranks share one device over gloo
        self.backend = os.environ.get("DCREG_BENCH_BACKEND", "nccl")
        if "DCREG_BENCH_LOCAL_RANK" in os.environ:
            self.local_rank = int(os.environ["DCREG_BENCH_LOCAL_RANK"])
        self.dry = bool(os.environ.get("DCREG_BENCH_DRYRUN"))
        self.cdev = "cuda" if self.backend == "nccl" else "cpu"       # device of the (tiny) collective payloads
        import torch
        self.torch = torch
        self.dist = None
        if not self.dry:
            if not torch.cuda.is_available():
                raise SystemExit("bench.py needs an MI355X: no HIP device visible and there is no CPU fallback")
            torch.cuda.set_device(self.local_rank)
        if self.world > 1:
            import torch.distributed as dist
            if self.backend == "nccl":
                dist.init_process_group("nccl", device_id=torch.device("cuda", self.local_rank))   # RCCL over xGMI
            else:
                dist.init_process_group(self.backend)
            self.dist = dist

    def fence(self):
        if not self.dry:
            self.torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()
        if not self.dry:
            self.torch.cuda.synchronize()

    def max_over_ranks(self, seconds):
        if self.dist is None:
            return seconds
        t = self.torch.tensor([seconds], dtype=self.torch.float64, device=self.cdev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather_rows(self, rec):
        t = self.torch.tensor(rec, dtype=self.torch.float64, device=self.cdev)
        if self.dist is None:
            return t.cpu().numpy()[None, :]
        allrec = [self.torch.zeros_like(t) for _ in range(self.world)]
        self.dist.all_gather(allrec, t)
        return self.torch.stack(allrec).cpu().numpy()

    def close(self):
        if self.dist is not None:
            self.dist.barrier()
            self.dist.destroy_process_group()


class Pair:
    """One scan pair on one device context, stepped through the product's engine seam."""

    def __init__(self, name, D, args, seed):
        import ctypes as C
        import dcreg_amd
        from dcreg_amd import api
        self.C, self.api, self.name = C, api, name
        w = WORKLOADS[name]
        self.w = w
        self.by_points = args.sharding == "points" and name == args.workload
        self.mc = name.startswith("c5_")
        self.tgt, src = make_pair(w["scene"], w["n"], seed)
        self.n_src_total = len(src)
        self.reducer, self.native = None, False
        self.last = None      # the IcpResult of the latest dcreg_icp_run* call (step_outputs).  It is self.res or the sharded call's result, which
                              # the next call overwrites: measure() copies it out right after the timed steps, before any other pass runs
        if self.by_points:                                        # points: the same pair everywhere, this rank's slice
            from dcreg_amd import pointshard
            lo, hi = pointshard.slice_of(len(src), D.rank, D.world)
            src = np.ascontiguousarray(src[lo:hi])
            self.native = D.backend == "nccl"        # RCCL all_gather inside the C++ engine loop; gloo hook: Python callback
            if not self.native:
                self.reducer = pointshard.make_reducer(D.dist, D.cdev)
        self.src = src
        self.ctx = dcreg_amd.Context(D.local_rank)
        for kv in args.opt:
            k, v = kv.split("=", 1)
            self.ctx.set_option(k, float(v))
        self.ctx.set_target(self.tgt, w["radius"])
        self.ctx.set_source(src)
        if self.by_points and self.native:
            from dcreg_amd import pointshard
            pointshard.init_native_exchange(self.ctx, D.dist, D.cdev)
        self.info = self.ctx.index_info()
        self.method = args.method
        self.det, self.hand = api.METHODS[args.method]
        self.cfg = api.default_config(search_radius=w["radius"], max_iterations=w["run_len"], KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0,
                                      CONVERGENCE_THRESH_ROT=0.0, CONVERGENCE_THRESH_TRANS=0.0,   # fixed-length runs
                                      use_weight_derivative=w["wd"], always_compute_schur=1)
        self.T_init = initial_pose(w["scene"])
        self.L = api.load()
        self.dp = C.POINTER(C.c_double)
        self.res = api.IcpResult()
        self.pos = 0                                             # iterations done in the current run
        self.R = np.ascontiguousarray(self.T_init[:3, :3]).reshape(9).copy()
        self.t = self.T_init[:3, 3].copy()
        self.mc_iters = 0
        if self.mc:
            from dcreg_amd import scenes as h
            self.cfg = api.default_config(search_radius=w["radius"], max_iterations=w["run_len"], CONVERGENCE_THRESH_TRANS=1e-3, CONVERGENCE_THRESH_ROT=1e-5,
                                          KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, DEGENERACY_THRES_COND=10.0, DEGENERACY_THRES_EIG=120.0,
                                          use_weight_derivative=w["wd"], always_compute_schur=1)
            self.mc_base = (0.2, 0.8, 0.5, h.deg2rad(0.1), h.deg2rad(0.1), h.deg2rad(2.0))
            self.mc_rank, self.mc_world = D.rank, D.world
            self.mc_stats, self.mc_ranks_seen, self.D = None, 0, D
            self.mc_comm, self.mc_native = False, False

    def _restart(self):
        self.pos = 0
        self.R[:] = np.ascontiguousarray(self.T_init[:3, :3]).reshape(9)
        self.t[:] = self.T_init[:3, 3]

    def run_steps(self, k):
        """k ICP iterations: consecutive iterations of back-to-back runs of run_len iterations, each run from T_init."""
        if self.mc:
            return self._run_steps_mc(k)
        api, C, L = self.api, self.C, self.L
        left = k
        while left > 0:
            n = min(self.w["run_len"] - self.pos, left)
            self.cfg.max_iterations = n
            if self.by_points:
                T = np.eye(4); T[:3, :3] = self.R.reshape(3, 3); T[:3, 3] = self.t
                if self.native:
                    out, _ = self.ctx.icp_run_sharded_rccl(T, self.method, self.cfg, self.n_src_total, log_capacity=0)
                else:
                    out, _ = self.ctx.icp_run_sharded(T, self.method, self.cfg, self.n_src_total, self.reducer, log_capacity=0)
                it, st = out.iterations, out.status
                self.R[:] = out.R[:]; self.t[:] = out.t[:]
                self.res.R[:] = out.R[:]; self.res.t[:] = out.t[:]
                self.last = out
            else:
                rc = L.dcreg_icp_run(self.ctx._h, self.R.ctypes.data_as(self.dp), self.t.ctypes.data_as(self.dp), api.DETECTION[self.det],
                                     api.HANDLING[self.hand], C.byref(self.cfg), None, 0, C.byref(self.res))
                if rc != 0:
                    raise RuntimeError("dcreg_icp_run failed: rc=%d %s" % (rc, L.dcreg_last_error(self.ctx._h)))
                it, st = self.res.iterations, self.res.status
                self.R[:] = self.res.R[:]; self.t[:] = self.res.t[:]
                self.last = self.res
            if it != n or st != 0:
                raise RuntimeError("%s: run stopped early: iterations=%d of %d status=%d" % (self.name, it, n, st))
            self.pos += n
            left -= n
            if self.pos >= self.w["run_len"]:
                self._restart()

    def _run_steps_mc(self, k):
        """k passes of the WHOLE Monte-Carlo experiment: this rank runs the trials k = rank mod world, the fixed-size trial records of all
        ranks are gathered (one all_gather: RCCL on the GPU node) and rank 0 takes the statistics (icp_test_runner.cpp:604-664) - all of
        it inside the caller's timed region.  mc_iters counts the ICP iterations of ALL trials (strong scaling: the job is fixed)."""
        from dcreg_amd import montecarlo as mcm
        D = self.D
        # the product path: ONE C-ABI call per experiment (dcreg_montecarlo_job: shard, run, ncclAllGather of the records on the ctx's
        # stream, statistics on every rank) - whenever the ranks can form an RCCL communicator, i.e. always except in the gloo test hook
        if self.mc_world == 1 or D.backend == "nccl":
            if self.mc_world > 1 and not self.mc_comm:
                from dcreg_amd import pointshard
                pointshard.init_native_exchange(self.ctx, D.dist, D.cdev)
                self.mc_comm = True
            for _ in range(k):
                _, st = self.ctx.montecarlo_job(self.mc_base, MC_SEED, MC_TRIALS, 0.5, np.deg2rad(2.0), self.method, self.cfg, slots=MC_SLOTS, want_records=False)
                self.mc_iters += int(st["iterations_total"])
                self.mc_ranks_seen = int(st["ranks_seen"])
                self.mc_native = True
                self.mc_stats = {kk: (int(v) if isinstance(v, int) else float(v)) for kk, v in st.items() if kk not in ("ranks_seen", "world", "iterations_total")}
            return
        for _ in range(k):
            mine = mcm.shard_indices(MC_TRIALS, self.mc_rank, self.mc_world)
            res = self.ctx.icp_run_montecarlo(self.mc_base, MC_SEED, self.mc_rank, self.mc_world, len(mine), 0.5, np.deg2rad(2.0), self.method, self.cfg, slots=MC_SLOTS)
            local = mcm.records_from_results(mine, res)
            recs = mcm.gather_records(local, MC_TRIALS, D.dist, D.cdev)
            self.mc_iters += int(recs[:, mcm.R_ITERS].sum())
            self.mc_ranks_seen = int(len(set((recs[:, mcm.R_TRIAL].astype(np.int64) % self.mc_world).tolist())))
            if D.rank == 0:
                self.mc_stats = mcm.method_statistics(recs)

    def close(self):
        self.ctx.close()


def kernel_pass(P, steps):
    """Mean device time of one linearisation (all kernels of a launch between one HIP-event pair on the context's stream), from a pass of its
    own: `steps` untimed steps of the same workload with the events on.  Nothing of this pass is inside a region `value` is computed from."""
    stride = MC_KERNEL_TIMING_STRIDE if P.mc else 1
    if not P.mc:
        P._restart()
    P.ctx.set_option("time_kernels", stride)
    P.ctx.kernel_time(reset=True)
    P.ctx.launch_stats(reset=True)
    P.run_steps(steps)
    kern_ms, kern_n = P.ctx.kernel_time(reset=True)
    st = P.ctx.launch_stats(reset=True)
    P.ctx.set_option("time_kernels", 0)
    if not P.mc:
        P._restart()
    return {"kernel_us": 1e3 * kern_ms / max(kern_n, 1), "launches_timed": int(kern_n),
            "points_per_launch": st["points"] / max(st["launches"], 1), "poses_per_launch": st["poses"] / max(st["launches"], 1),
            "source": "separate pass: HIP events around %s launch of %d steps (%s), outside the timed regions" % (
                "every" if stride == 1 else "every %dth" % stride, steps, "whole runs from the initial pose" if not P.mc else "one whole experiment")}


def measure(P, D, steps, warmup, repeats, min_seconds=0.0, kernel_steps=None):
    """warm-up, then `repeats` timed regions of exactly `steps` steps, each bracketed by the fence; times are max-over-ranks.  min_seconds > 0:
    the region is repeated until the timed regions add up to that much (all ranks take the count from rank 0's calibration).  No HIP event is
    recorded inside a timed region; the kernel time comes from kernel_pass afterwards.
    Returns dict(times=[s per block], outputs (step_outputs after the last timed step), kernel_us, iters_per_step, points_per_launch,
    poses_per_launch)."""
    P.run_steps(warmup)
    P.ctx.set_option("time_kernels", 0)
    mc0 = P.mc_iters
    times = []
    import gc
    gc.collect()
    gc.disable()          # (a generation-2 collection of this process - torch imported, a million-point scene in numpy - takes 30 ms and
    try:                  #  lands in whichever repeat crosses the allocation threshold: it was 7 % of the timed region at --steps 20)
        def one():
            D.fence()
            t0 = time.perf_counter()
            P.run_steps(steps)
            D.fence()
            times.append(D.max_over_ranks(time.perf_counter() - t0))
        n = max(int(repeats), 1)
        if min_seconds > 0.0:
            for _ in range(3):
                one()
            n = max(n, int(np.ceil(min_seconds / max(float(np.mean(times)), 1e-6))))      # (max-over-ranks times: the same count on every rank)
        while len(times) < n:
            one()
    finally:
        gc.enable()
    outputs = step_outputs(P)             # (before kernel_pass: it restarts the pair and steps on)
    per_step = (P.mc_iters - mc0) / float(steps * len(times)) if P.mc else 1.0
    run_len = P.w["run_len"]
    kp = kernel_pass(P, kernel_steps if kernel_steps is not None else (1 if P.mc else 3 * run_len))
    return {"times": times, "outputs": outputs, "kernel_us": kp["kernel_us"], "kernel_source": kp["source"], "iters_per_step": per_step,
            "points_per_launch": kp["points_per_launch"], "poses_per_launch": kp["poses_per_launch"]}


def step_outputs(P):
    """What the caller of the timed path received from its latest step, as float64 arrays: the pose, covariance and run state of the
    IcpResult the last dcreg_icp_run* call returned, or for the Monte-Carlo workload the statistics of the last experiment.  Wall times
    (IcpResult.time_ms, the statistics' *_time_ms) are measurements, not results, and are left out.  A few hundred bytes in all."""
    if P.mc:
        return {"montecarlo_" + k: np.float64(v) for k, v in (P.mc_stats or {}).items() if not k.endswith("time_ms")}
    r = P.last
    return {"R": np.array(r.R[:]).reshape(3, 3), "t": np.array(r.t[:]), "icp_cov": np.array(r.icp_cov[:]).reshape(6, 6),
            "converged": np.float64(r.converged), "iterations": np.float64(r.iterations), "status": np.float64(r.status)}


def write_outputs(out_dir, outputs):
    os.makedirs(out_dir, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, dtype=np.float64))


def roofline_blocks(name, n_queries_per_launch, kern_us, kern_source=None):
    """The HBM block the contract asks for + the VALU-issue block (what actually binds the kernel).  `achieved` is live:
    algorithmic bytes of the points ONE launch linearises / the HIP-event time of that launch in THIS run; `traffic` and the
    instruction count are per-launch PMC figures of the same workload read from the committed rocprofv3 summaries (labelled with
    their source file); the cycles per VALU instruction come from the committed microbenchmark (scripts/microbench) priced over the
    kernel's instruction mix (scripts/asm_mix.py)."""
    algo = BYTES_PER_QUERY * n_queries_per_launch
    achieved = algo / (kern_us * 1e-6) / 1e9 if kern_us > 0 else 0.0
    prof = profile_record(name)
    hbm = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
           "traffic": prof.get("traffic_bytes"), "traffic_source": prof.get("source"),
           "kernel": "k_lin (certificate test, exact 6-NN search where needed, plane fit, point-to-plane row, J^T J / J^T r reduction) + the advance pass "
                     "the host puts in front of it in some launches (k_advance / k_advance_team: the searches and refits in dense waves / by teams of 16 lanes) "
                     "and k_sum_tiles behind the one-wave launches (the first launches of a run); "
                     "kernel_us_avg brackets all kernels of a linearisation",
           "kernel_us_avg": kern_us, "kernel_us_source": kern_source, "points_per_launch": n_queries_per_launch, "algorithmic_bytes_per_launch": algo}
    out = {"roofline": hbm}
    mix = valu_mix()
    if prof.get("valu_insts_per_launch") and kern_us > 0 and mix:
        cyc = mix["mean_cycles_per_valu_w8"]          # the saturated issue cost (8 waves / SIMD): the floor no occupancy can beat
        floor_us = prof["valu_insts_per_launch"] * cyc / N_SIMD / CLOCK_HZ * 1e6
        out["roofline_valu_issue"] = {"bound": "valu_issue", "achieved": prof["valu_insts_per_launch"] / (kern_us * 1e-6) / 1e12,
                                      "peak": N_SIMD * CLOCK_HZ / cyc / 1e12, "unit": "T wave-instructions/s", "frac": floor_us / kern_us,
                                      "floor_us": floor_us, "valu_insts_per_launch": prof["valu_insts_per_launch"],
                                      "cycles_per_valu_inst": cyc, "cycles_per_valu_inst_at_4_waves_per_simd": mix["mean_cycles_per_valu_w4"],
                                      "cycles_source": mix["source"], "source": prof.get("source")}
    return out


def valu_mix():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_valu_mix.json")))
    if not files:
        return None
    try:
        j = json.load(open(files[-1]))
        j["source"] = os.path.relpath(files[-1], ROOT) + " (microbenchmark: " + j.get("microbench", "?") + ")"
        return j
    except Exception:
        return None


def profile_record(workload):
    """Per-launch PMC figures of k_linearize from the newest committed rocprofv3 summary of this workload
    (profiles/rNN_<workload>.json, written by scripts/summarize_profiles.py): HBM-side bytes (FETCH_SIZE x2 per the gfx950
    note in MI355X_MICROARCH.md + WRITE_SIZE, separate passes) and wave-level VALU instructions."""
    import glob
    rec = {}
    import re
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s.json" % workload))):
        if not re.fullmatch(r"r\d+_%s\.json" % re.escape(workload), os.path.basename(f)):
            continue                                  # (e.g. rNN_steady_<workload>.json: the settled launches only, another command)
        try:
            j = json.load(open(f))
        except Exception:
            continue
        t = j.get("traffic") or {}
        if t.get("bytes_fetch_x2"):
            rec["traffic_bytes"] = t["bytes_fetch_x2"]
            rec["source"] = os.path.relpath(f, ROOT)
        v = (j.get("pmc") or {}).get("SQ_INSTS_VALU_per_launch")
        if v:
            rec["valu_insts_per_launch"] = v
            rec["source"] = os.path.relpath(f, ROOT)
    return rec


def summarize(name, P, D, m, steps, n_gpus):
    times = np.array(m["times"])
    per_step_s = times / steps
    total_iters = (1 if (P.by_points or P.mc) else n_gpus) * steps * len(times) * m["iters_per_step"]
    value = total_iters / float(times.sum())
    w = WORKLOADS[name]
    rec = {"value": value, "unit": "iterations/s", "ms_per_step": 1e3 * float(times.sum()) / (steps * len(times)),
           "ms_per_step_median": 1e3 * float(np.median(per_step_s)), "ms_per_step_min": 1e3 * float(per_step_s.min()),
           "ms_per_step_max": 1e3 * float(per_step_s.max()), "repeats": int(len(times)), "steps": steps,
           "slowest_repeats": [[int(i), 1e3 * float(per_step_s[i])] for i in np.argsort(per_step_s)[::-1][:3]],
           "icp_iterations_per_step": m["iters_per_step"], "correspondence_queries_per_s": value * P.n_src_total,
           "workload": ("%s [%s]: %d-pt source x %d-pt target, radius %.2f, %d trials from seeded initial poses, <= %d ICP iterations each, thresholds on, method %s" % (
               name, w["cfg"], P.n_src_total, len(P.tgt), w["radius"], MC_TRIALS, w["run_len"], P.method)) if P.mc else
                       ("%s [%s]: %d-pt source x %d-pt target, radius %.2f, back-to-back runs of %d ICP iterations, method %s" % (
               name, w["cfg"], P.n_src_total, len(P.tgt), w["radius"], w["run_len"], P.method))}
    rec.update(roofline_blocks(name, m["points_per_launch"], m["kernel_us"], m.get("kernel_source")))
    rec["timed_seconds"] = float(times.sum())
    rec["poses_per_launch"] = m["poses_per_launch"]
    if P.mc:
        rec["n_gpus"] = n_gpus
        rec["scaling"] = "strong"
        rec["rccl_ranks_seen"] = P.mc_ranks_seen
        rec["montecarlo"] = {"trials": MC_TRIALS, "trials_per_rank": "k = rank mod %d" % n_gpus, "slots_in_flight": MC_SLOTS, "seed": MC_SEED,
                             "record_gather": ("dcreg_montecarlo_job: one ncclAllGather of the 64-double trial records on the context's stream, inside the "
                                               "C-ABI call and the timed region" if P.mc_native else
                                               "one torch.distributed all_gather of the 64-double trial records inside the timed region (gloo test hook)"),
                             "statistics": P.mc_stats}
    return rec


def regime_probe(P, runs=6):
    """Where the launches of whole runs spend their time: every launch of `runs` back-to-back runs is bracketed by HIP events and
    reports how many of its points it searched (the count travels in the launch's own result rows: dcreg_debug.h dcreg_launch_series);
    bucketed by that fraction.  all_search: >= half of the points searched (the first iterations of a run); settled: <= 1e-4 of them
    (certificates hold: the launch streams 72 B per point); transition: in between.  frac = 72 B x points / mean time / HBM peak."""
    w = P.w
    P._restart()
    P.ctx.set_option("time_kernels", 1)
    P.ctx.set_option("record_launches", 1)
    P.ctx.launch_series(reset=True)
    P.run_steps(runs * w["run_len"])
    ser = P.ctx.launch_series(reset=True)
    P.ctx.set_option("record_launches", 0)
    P.ctx.set_option("time_kernels", 0)
    P.ctx.kernel_time(reset=True)
    P._restart()
    ok = (ser["ms"] >= 0) & (ser["searched"] >= 0) & (ser["points"] > 0)
    ms, frac_s, pts = ser["ms"][ok], ser["searched"][ok] / ser["points"][ok], ser["points"][ok]
    refit = ser["refitted"][ok] / ser["points"][ok]
    out = {"runs": runs, "launches": int(ok.sum()), "source": "HIP events around every launch of %d whole runs (dcreg_launch_series); the searched / refitted "
           "counts are reported by the launches themselves" % runs,
           "bucket_rule": {"all_search": "searched >= 0.5 of the points", "transition": "1e-4 < searched < 0.5", "settled": "searched <= 1e-4"}}
    for name, sel in (("all_search", frac_s >= 0.5), ("transition", (frac_s > 1e-4) & (frac_s < 0.5)), ("settled", frac_s <= 1e-4)):
        if not sel.any():
            out[name] = {"launches": 0}
            continue
        us = 1e3 * ms[sel]
        mean_us = float(us.mean())
        algo = BYTES_PER_QUERY * float(pts[sel].mean())
        out[name] = {"launches": int(sel.sum()), "mean_us": mean_us, "min_us": float(us.min()), "max_us": float(us.max()),
                     "share_of_kernel_time": float(us.sum() / (1e3 * ms.sum())),
                     "launches_with_advance_pass": int((ser["advanced"][ok][sel] == 1).sum()), "launches_with_team_pass": int((ser["advanced"][ok][sel] == 2).sum()),
                     "launches_in_one_wave_blocks": int(ser["one_wave"][ok][sel].sum()),
                     "mean_searched_frac": float(frac_s[sel].mean()), "mean_refitted_frac": float(refit[sel].mean()),
                     "achieved_GBps": algo / (mean_us * 1e-6) / 1e9, "frac": algo / (mean_us * 1e-6) / 1e9 / HBM_PEAK_GBS}
    # the first four launches of a run, by position (the launches 0.87 m off the surface)
    per_run = w["run_len"]
    k = np.arange(int(ok.sum())) % per_run
    if ok.all() and len(ms) == runs * per_run:
        out["by_iteration_us"] = {"iter_%d" % i: float(1e3 * ms[k == i][1:].mean()) for i in (0, 1, 2, 3, 5, 10, 15, 20, 30, 49) if i < per_run}
    return out


def converged_run(P, D, repeats=10, cold=False):
    """The workload's pair with the reference's convergence test on (icp_test_runner.cpp:1957-1975; thresholds = dcreg_default_config =
    utils.hpp:139-140): runs from the same initial pose until convergence.  cold: the context's neighbour state is dropped before every
    run (dcreg_reset_warm_state(ctx, -1), outside the timed part) - the reference builds a fresh ICPContext per run
    (icp_test_runner.cpp:408-409), so nothing a previous run found is known when the next one starts; clouds and index stay resident as
    they do there (setTargetCloud is outside the reference's timed part too, :408-442).  Without it a run starts from what the previous
    run's converged pose left in the state (bounds from neighbours 0.87 m away)."""
    api, C, L = P.api, P.C, P.L
    cfg = api.default_config(search_radius=P.w["radius"], max_iterations=P.w["run_len"], KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0,
                             use_weight_derivative=P.w["wd"], always_compute_schur=1)
    R0 = np.ascontiguousarray(P.T_init[:3, :3]).reshape(9).copy()
    t0 = P.T_init[:3, 3].copy()
    res = api.IcpResult()
    its, times = [], []
    for rep in range(repeats + 1):
        if cold:
            P.ctx.reset_warm_state(-1)
        D.fence()
        ta = time.perf_counter()
        rc = L.dcreg_icp_run(P.ctx._h, R0.ctypes.data_as(P.dp), t0.ctypes.data_as(P.dp), api.DETECTION[P.det], api.HANDLING[P.hand], C.byref(cfg), None, 0, C.byref(res))
        D.fence()
        if rc != 0:
            raise RuntimeError("dcreg_icp_run failed: rc=%d" % rc)
        if rep > 0:                                            # (the first run also pays the walk back from the last pose of the bench loop)
            times.append(time.perf_counter() - ta); its.append(res.iterations)
    P._restart()
    t = np.array(times)
    return {"neighbour_state_at_start": "empty (dropped before every run: a fresh ICPContext, icp_test_runner.cpp:408-409)" if cold else
            "what the previous run left at its converged pose",
            "thresholds": {"rot_rad": cfg.CONVERGENCE_THRESH_ROT, "trans_m": cfg.CONVERGENCE_THRESH_TRANS, "source": "dcreg_default_config = DCReg/include/utils.hpp:139-140"},
            "converged": int(res.converged), "iterations_to_convergence": float(np.mean(its)), "ms_per_run": 1e3 * float(t.mean()),
            "ms_per_run_min": 1e3 * float(t.min()), "iterations_per_s": float(np.sum(its) / t.sum()), "repeats": repeats,
            "note": "runs from the bench's initial pose until |d rot| < %.0e rad and |d trans| < %.0e m; max %d iterations" % (
                cfg.CONVERGENCE_THRESH_ROT, cfg.CONVERGENCE_THRESH_TRANS, P.w["run_len"])}


def c3_registration(D, args, repeats=20, prior_map_points=0, extent=350.0):
    """prior_map_points > 0: the same registration against a LARGE seeded prior map (scenes.scene_prior_map: the regime of the reference's
    published timings, 1-10 k-point frames against 53-241 M-point maps) - map upload + index build reported beside it, once.
    What the reference itself times (icp_test_runner.cpp:442-461; paper tables 6 / 7: Parking Lot 2.11 ms per registration on 1-10 k-point
    frames): ONE registration of an 8 k-point frame against the 200 k-point map from HOST buffers - dcreg_set_source (upload, curve
    sort) + run to convergence with the yaml's thresholds; the map and its index are resident (the reference's kd-tree of the map is
    built once as well).  The CPU oracle's run of the same pair beside it (8 OpenMP threads, kd-tree of the map built beforehand)."""
    import dcreg_amd
    from dcreg_amd import api, scenes as h
    t_gen = time.perf_counter()
    tgt, src = h.scene_prior_map(prior_map_points, extent=extent) if prior_map_points else h.scene_parkinglot()
    t_gen = time.perf_counter() - t_gen
    gt, T0 = h.pose6d_matrix(**h.PK01_GT), h.pose6d_matrix(**h.PK01_INIT)
    ctx = dcreg_amd.Context(D.local_rank)
    for kv in args.opt:
        k, v = kv.split("=", 1)
        ctx.set_option(k, float(v))
    t_map = time.perf_counter()
    ctx.set_target(tgt, 0.5)
    t_map = time.perf_counter() - t_map
    info = ctx.index_info()
    cfg = api.default_config(search_radius=0.5, max_iterations=30, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, CONVERGENCE_THRESH_ROT=1e-5,
                             CONVERGENCE_THRESH_TRANS=1e-3, use_weight_derivative=0, always_compute_schur=1, gt_matrix=gt.reshape(16))
    t_src, t_tot, its = [], [], []
    res = None
    t_first = 0.0
    for rep in range(repeats + 3):
        ta = time.perf_counter()
        ctx.set_source(src)
        tb = time.perf_counter()
        res, _ = ctx.icp_run(T0, args.method, cfg, log_capacity=0)
        tc = time.perf_counter()
        if rep == 0:
            t_first = tc - ta
        if rep >= 3:
            t_src.append(tb - ta); t_tot.append(tc - ta); its.append(res.iterations)
    roi = ctx.roi_info()
    # one more registration, logged (untimed): which launches ran the small-frame pass, and what they searched
    ctx.set_option("record_launches", 1)
    ctx.launch_series(reset=True)
    ctx.set_source(src)
    ctx.icp_run(T0, args.method, cfg, log_capacity=0)
    ser = ctx.launch_series(reset=True)
    ctx.set_option("record_launches", 0)
    T = np.eye(4); T[:3, :3] = np.array(res.R[:]).reshape(3, 3); T[:3, 3] = res.t[:]
    te, re_ = api.pose_error(gt, T)
    # candidates evaluated per query by a cold search at the initial pose (debug dump, untimed): what the index costs at this map's scale
    ctx.set_source(src)
    dd = ctx.linearize(T0[:3, :3], T0[:3, 3], api.default_lin_params(0.5, 0), debug=True)
    ne = (dd["stats"] & 0xFFFF).astype(np.int64)
    cand = {"mean": float(ne.mean()), "p50": float(np.percentile(ne, 50)), "p90": float(np.percentile(ne, 90)), "p99": float(np.percentile(ne, 99)),
            "note": "target points whose distance a query's cold search at the initial pose evaluated (k_lin<1> dump)"}
    ctx.close()
    out = {"ms_total": 1e3 * float(np.mean(t_tot)), "ms_total_min": 1e3 * float(np.min(t_tot)), "ms_set_source": 1e3 * float(np.mean(t_src)),
           "ms_iterations": 1e3 * float(np.mean(t_tot) - np.mean(t_src)), "iterations": float(np.mean(its)), "converged": int(res.converged),
           "trans_error_vs_gt_m": float(te), "rot_error_vs_gt_deg": float(re_), "repeats": repeats,
           "workload": "%s: %d-pt frame vs %d-pt map, radius 0.5, method %s, thresholds 1e-5 rad / 1e-3 m, init / gt poses of config/icp_pk01.yaml; "
                       "frame from a host buffer every time (dcreg_set_source), map resident" % (
                           ("seeded prior map (scenes.scene_prior_map, %.0f m x %.0f m)" % (2 * extent, 2 * extent)) if prior_map_points else "PK01 stand-in", len(src), len(tgt), args.method),
           "candidates_per_query": cand,
           "window_index": {"active": roi["active"], "points": roi["points"], "grid_cell_m": roi["cell"], "windows_built": roi["windows_built"],
                            "box_min": roi["box_min"], "box_max": roi["box_max"], "whole_map_table_capped": roi["whole_map_capped"],
                            "ms_first_registration": 1e3 * t_first,
                            "note": "single-pose linearisations of a map whose dense cell table ran into max_table_entries search an index over the map's points in a box "
                                    "around the transformed frame (bitwise the whole map's sums); built by the first registration, kept while the pose stays inside; "
                                    "candidates_per_query above is the WHOLE map's index (debug dumps run there)"},
           "map": {"points": int(len(tgt)), "grid_cell_m": info.cell, "grid_cells": int(info.n_cells), "dims": [int(v) for v in info.dims],
                   "s_set_target_from_host": t_map, "s_scene_generation": t_gen},
           "launch_structure": {"k_lin_alone": int((ser["advanced"] == 0).sum()), "k_advance_team_then_k_lin": int((ser["advanced"] == 2).sum()),
                                "k_advance_then_k_lin": int((ser["advanced"] == 1).sum()), "searched_per_launch": [int(x) for x in ser["searched"]]},
           "reference_published_ms": 2.11, "reference_source": "paper table 6 / results/long_duration experiments/table3_4/*/dcreg/data_time.txt (Parking Lot, the authors' CPU; real data)"}
    if not args.no_cpu_baseline and len(tgt) <= 10_000_000:       # (the oracle's kd-tree of a 50 M-point map: minutes of build, 2 GB)
        from oracle import pyoracle as po
        tree = po.KdTree(tgt)
        ocfg = po.default_config(search_radius=0.5, max_iterations=30, kappa_target=10.0, std_reg_gamma=100.0, thresh_rot=1e-5, thresh_trans=1e-3,
                                 use_weight_derivative=0, always_compute_schur=1, num_threads=8, gt=gt.reshape(16))
        po.icp_run(tree, src, T0, args.method, ocfg)
        ts = []
        for _ in range(5):
            ta = time.perf_counter()
            ores, _ = po.icp_run(tree, src, T0, args.method, ocfg)
            ts.append(time.perf_counter() - ta)
        out["cpu_oracle"] = {"ms_total": 1e3 * float(np.mean(ts)), "iterations": int(ores.iterations), "cores": 8, "kind": "port"}
    return out


def c5_host_thread_sweep(D, args, counts):
    """The Monte-Carlo experiment on ONE GPU with the host steps of the engine limited to 2 / 4 / ... OpenMP threads: what a rank of an
    8-rank job on a 16-CPU box has."""
    from dcreg_amd import api
    out = {}
    Q = Pair("c5_montecarlo_5000", D, args, seed=100)
    keep = api.load().dcreg_get_host_threads()
    for n in counts:
        got = api.set_host_threads(n)
        mq = measure(Q, D, steps=1, warmup=1, repeats=3)
        r = summarize("c5_montecarlo_5000", Q, D, mq, 1, 1)
        out["threads_%d" % got] = {"host_threads": got, "value": r["value"], "unit": "iterations/s", "ms_per_experiment": r["ms_per_step"]}
    if keep:
        api.set_host_threads(keep)
    Q.close()
    return out


def concurrent_pairs(P0, D, args, steps, warmup):
    """Throughput with several independent pairs in flight on the same GPU (extra figure, not `value`): the device idles
    during every host step, so independent pairs interleave."""
    import threading
    Pn = args.concurrent_pairs
    pairs = [P0] + [Pair(P0.name, D, args, seed=100 + D.rank + 1000 * q) for q in range(1, Pn)]
    errors = []

    def worker(p, k, barrier):
        barrier.wait()
        try:
            p.run_steps(k)
        except Exception as e:
            errors.append(str(e))

    t_conc = None
    for k in (warmup, steps):
        for p in pairs:
            p._restart()
        barrier = threading.Barrier(Pn + 1)
        th = [threading.Thread(target=worker, args=(p, k, barrier)) for p in pairs]
        for t_ in th:
            t_.start()
        D.fence()
        barrier.wait()
        ta = time.perf_counter()
        for t_ in th:
            t_.join()
        D.fence()
        t_conc = D.max_over_ranks(time.perf_counter() - ta)
    for p in pairs[1:]:
        p.close()
    if errors:
        raise RuntimeError("; ".join(errors))
    n = WORKLOADS[P0.name]["n"]
    return {"pairs_per_gpu": Pn, "value": D.world * Pn * steps / t_conc, "unit": "iterations/s", "us_per_iteration_per_pair": 1e6 * t_conc / steps,
            "achieved_GBps_wall": Pn * BYTES_PER_QUERY * n * steps / t_conc / 1e9,
            "frac_of_hbm_peak_wall": Pn * BYTES_PER_QUERY * n * steps / t_conc / 1e9 / HBM_PEAK_GBS,
            "note": "%d independent %d-pt pairs in flight per GPU, one context + stream + host thread each, %d iterations each (whole runs); aggregate over all GPUs" % (Pn, n, steps)}


def montecarlo_child(args, n_gpus, timeout_s=900.0):
    """N > 1: the Monte-Carlo experiment as a job of its OWN (`bench.py --gpus N --workload c5_montecarlo_5000 --sub-record`, started by rank 0
    once every rank of this job has closed its context and left the process group).  It is the one leg whose ranks exchange data - the library's
    own RCCL communicator, dcreg_montecarlo_job's ncclAllGather - and RCCL with more than one rank has never run on hardware: whatever that path
    does (error, abort, hang), the headline measured before it (independent scan pairs, no data-path collective) still reaches the JSON line,
    with this leg's failure written into it.  Returns the leg's summary record or {"error": ...}."""
    import subprocess
    env = dict(os.environ)
    for k in list(env):       # the launcher's per-rank variables: the child starts its own ranks (maybe_spawn)
        if k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "GROUP_WORLD_SIZE", "ROLE_RANK", "ROLE_NAME",
                 "ROLE_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT") or k.startswith("TORCHELASTIC_"):
            env.pop(k)
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(n_gpus), "--workload", "c5_montecarlo_5000", "--steps", "1", "--warmup", "1",
           "--repeats", "5", "--min-seconds", "0", "--method", args.method, "--no-configs", "--no-cpu-baseline", "--no-regimes",
           "--concurrent-pairs", "0", "--sub-record"]
    for kv in args.opt:
        cmd += ["--opt", kv]
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout_s, cwd=os.path.dirname(os.path.abspath(__file__)))
    except subprocess.TimeoutExpired as e:
        return {"error": "the Monte-Carlo job of %d ranks did not finish within %.0f s" % (n_gpus, timeout_s),
                "stderr_tail": ((e.stderr or b"")[-1500:].decode("utf-8", "replace") if isinstance(e.stderr, bytes) else (e.stderr or "")[-1500:])}
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or len(lines) != 1:
        return {"error": "the Monte-Carlo job of %d ranks failed (rc %d, %d JSON lines)" % (n_gpus, p.returncode, len(lines)), "stderr_tail": p.stderr[-1500:]}
    rec = json.loads(lines[0])
    rec["job"] = "a job of its own behind the main measurement (%d ranks, %.1f s incl. start-up)" % (n_gpus, time.perf_counter() - t0)
    return rec


def dry_run(args, D):
    """DCREG_BENCH_DRYRUN=1 (CPU test hook): the launcher, rendezvous, fence, max-over-ranks and gather paths with a
    synthetic per-rank record instead of device work.  Prints a line marked "dry_run": true that is NOT a measurement."""
    from dcreg_amd import api, hostinfo
    from dcreg_amd import montecarlo as mcm
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(D.world)))
    want, _ = hostinfo.setup_rank(D.local_rank, local_world)     # share first, then the rank's slice of the CPU mask (as main())
    got = api.set_host_threads(want)                 # (overrides the OMP_NUM_THREADS=1 torch.distributed.run exports)
    times = []
    for _ in range(2):
        D.fence()
        t0 = time.perf_counter()
        time.sleep(0.01 * (1 + D.rank))
        D.fence()
        times.append(D.max_over_ranks(time.perf_counter() - t0))
    recs = D.gather_rows([float(D.rank), float(100 + D.rank), float(got), 0.0])
    # the strong-scaling leg (configs[4]): this rank's share of the trials -> synthetic records -> ONE gather inside the timed region ->
    # statistics on rank 0, exactly the calls Pair._run_steps_mc makes around the engine
    D.fence()
    t0 = time.perf_counter()
    mine = mcm.shard_indices(MC_TRIALS, D.rank, D.world)
    local = np.zeros((len(mine), mcm.REC))
    local[:, mcm.R_TRIAL] = mine
    local[:, mcm.R_ITERS] = 10 + mine % 7
    local[:, mcm.R_CONV] = (mine % 4 != 0)
    allr = mcm.gather_records(local, MC_TRIALS, D.dist, D.cdev)
    seen = int(len(set((allr[:, mcm.R_TRIAL].astype(np.int64) % D.world).tolist())))
    stats = mcm.method_statistics(allr) if D.rank == 0 else None
    D.fence()
    t_mc = D.max_over_ranks(time.perf_counter() - t0)
    if D.rank == 0:
        print(json.dumps({"dry_run": True, "metric": "ICP iterations/sec", "value": None, "n_gpus": D.world, "steps": args.steps,
                          "warmup": args.warmup, "rank_seeds": [int(r[1]) for r in recs], "ranks": [int(r[0]) for r in recs],
                          "host_threads": [int(r[2]) for r in recs], "host_threads_per_rank": want,
                          "block_times_s": times,
                          "c5_montecarlo_5000": {"n_gpus": D.world, "scaling": "strong", "trials": int(stats["total_runs"]), "rccl_ranks_seen": seen,
                                                 "iterations": int(allr[:, mcm.R_ITERS].sum()), "converged_runs": int(stats["converged_runs"]),
                                                 "seconds": t_mc}}), flush=True)
    D.close()


def compact_line(result):
    """The JSON line, at most LINE_BYTES: the headline in full except the prose of its roofline blocks; of every leg beside it the few
    numbers of LINE_LEG_KEYS; a failed leg only under side_leg_errors, its error cut to LINE_ERROR_CHARS.  Regime blocks, sub-records,
    notes and whole error texts are left to --full-record."""
    legs = ("roofline_by_regime", "converged_run", "cold_run", "concurrent_pairs", "cpu_baseline", "configs")
    line = {k: v for k, v in result.items() if k not in legs}
    for k in ("roofline", "roofline_valu_issue"):
        if k in line:
            line[k] = {kk: v for kk, v in line[k].items() if not (isinstance(v, str) and len(v) > LINE_STRING_CHARS)}
    if "side_leg_errors" in line:
        line["side_leg_errors"] = {k: v[:LINE_ERROR_CHARS] for k, v in line["side_leg_errors"].items()}

    def numbers(rec):
        return {k: rec[k] for k in LINE_LEG_KEYS if k in rec}

    for k in ("converged_run", "cold_run", "concurrent_pairs", "cpu_baseline"):
        if k in result and "error" not in result[k]:
            line[k] = numbers(result[k])
    if "configs" in result:
        line["configs"] = {name: numbers(rec) for name, rec in result["configs"].items() if "error" not in rec}
    return line


def main(argv=None):
    args = parse_args(argv)
    maybe_spawn(args)
    D = Dist()
    if D.dry:
        return dry_run(args, D)
    n_gpus = D.world
    from dcreg_amd import scenes as h
    from dcreg_amd import api, hostinfo
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(D.world)))
    # (torch.distributed.run exports OMP_NUM_THREADS=1: the batched engine's host steps get this rank's share of the usable CPUs -
    # computed before the rank is pinned to its slice of them)
    want_threads, _ = hostinfo.setup_rank(D.local_rank, local_world)
    host_threads = api.set_host_threads(want_threads)

    P = Pair(args.workload, D, args, seed=100 + (0 if args.sharding == "points" else D.rank))   # pairs: every rank its own scan pair
    m = measure(P, D, args.steps, args.warmup, args.repeats, min_seconds=args.min_seconds)
    if args.dump_outputs and D.rank == 0:
        write_outputs(args.dump_outputs, m["outputs"])
    main_rec = summarize(args.workload, P, D, m, args.steps, n_gpus)
    if args.sub_record:                         # (montecarlo_child's job: the record is all the parent wants)
        main_rec["host_threads_per_rank"] = host_threads
        if D.rank == 0:
            print(json.dumps(main_rec), flush=True)
        P.close()
        D.close()
        return

    # Everything below is reported BESIDE the headline: a leg that fails (a timeout, a device error in a side workload) is written into the
    # line as {"error": ...} and never takes the headline measured above with it.
    side_errors = {}

    def guard(name, fn, *a, **k):
        try:
            return fn(*a, **k)
        except Exception as e:           # noqa: BLE001 - whatever a side leg raises is reported, not propagated
            side_errors[name] = "%s: %s" % (type(e).__name__, str(e)[:300])
            return {"error": side_errors[name]}

    regimes = conv = cold = None
    if not P.mc and not P.by_points and n_gpus == 1 and not args.no_regimes:
        regimes = guard("roofline_by_regime", regime_probe, P)
        conv = guard("converged_run", converged_run, P, D)
        cold = guard("cold_run", lambda: converged_run(P, D, cold=True))

    # final statistics gather (the only collective): per-rank pose error / rmse / correspondences after one whole run
    try:
        P._restart()
        if not P.mc:
            P.run_steps(WORKLOADS[args.workload]["run_len"])
        T_fin = np.eye(4); T_fin[:3, :3] = np.array(P.res.R[:]).reshape(3, 3); T_fin[:3, 3] = P.res.t[:]
        gt = h.pose6d_matrix(**h.PK01_GT) if WORKLOADS[args.workload]["scene"] == "parkinglot" else np.eye(4)
        te, re_ = api.pose_error(gt, T_fin)
        last = P.ctx.linearize(T_fin[:3, :3], T_fin[:3, 3], api.default_lin_params(WORKLOADS[args.workload]["radius"], WORKLOADS[args.workload]["wd"]))
        mine = [te, re_, float(last["n_eff"]), float(100 + D.rank)]
    except Exception as e:               # noqa: BLE001 - every rank still takes part in the gather
        side_errors["final_stats"] = "%s: %s" % (type(e).__name__, str(e)[:300])
        mine = [float("nan"), float("nan"), float("nan"), float(100 + D.rank)]
    recs = D.gather_rows(mine)

    conc = None
    if args.concurrent_pairs > 1 and not P.mc and not P.by_points and n_gpus == 1:
        run_len = WORKLOADS[args.workload]["run_len"]
        conc = guard("concurrent_pairs", concurrent_pairs, P, D, args, steps=2 * run_len, warmup=run_len)

    sub = {}
    if not args.no_configs and args.sharding == "pairs":
        for name in WORKLOADS:
            if name == args.workload:
                continue
            mc = name.startswith("c5_")
            if n_gpus > 1:
                continue                        # N > 1: only the experiment that is sharded over the ranks (strong scaling) - as a job
                                                # of its own once this one's ranks are through (montecarlo_child, below)
            w = WORKLOADS[name]

            def one_config(name=name, w=w, mc=mc):
                Q = Pair(name, D, args, seed=100)
                try:
                    k = 1 if mc else w["run_len"] * 2
                    mq = measure(Q, D, steps=k, warmup=1 if mc else w["run_len"], repeats=5)
                    rec = summarize(name, Q, D, mq, k, n_gpus)
                    rec["host_threads_per_rank"] = host_threads
                    if n_gpus == 1 and not mc and not args.no_regimes:
                        rec["roofline_by_regime"] = regime_probe(Q, runs=4)
                        rec["converged_run"] = converged_run(Q, D, repeats=5)
                        rec["cold_run"] = converged_run(Q, D, repeats=5, cold=True)
                    return rec
                finally:
                    Q.close()
            sub[name] = guard(name, one_config)
        if n_gpus == 1:
            sub["c3_pk01_8k_registration"] = guard("c3_pk01_8k_registration", c3_registration, D, args)
            if args.prior_map_points > 0:
                sub["c3_prior_map_50m"] = guard("c3_prior_map_50m", c3_registration, D, args, repeats=20, prior_map_points=args.prior_map_points)
            if args.prior_map_points_large > 0:
                sub["c3_prior_map_200m"] = guard("c3_prior_map_200m", c3_registration, D, args, repeats=20, prior_map_points=args.prior_map_points_large, extent=700.0)
            usable = hostinfo.usable_cpus()
            if "error" not in sub.get("c5_montecarlo_5000", {"error": 1}):
                sub["c5_montecarlo_5000"]["by_host_threads"] = guard("c5_by_host_threads", c5_host_thread_sweep, D, args, sorted({2, 4, min(16, usable)}))
            api.set_host_threads(host_threads)

    if n_gpus > 1:
        # every rank leaves its context and the process group first; then the one leg whose ranks exchange data runs as a job of its own
        P.close()
        D.close()
        if D.rank == 0 and not args.no_configs and args.sharding == "pairs" and not P.mc:
            sub["c5_montecarlo_5000"] = montecarlo_child(args, n_gpus)
            if "error" in sub["c5_montecarlo_5000"]:
                side_errors["c5_montecarlo_5000"] = sub["c5_montecarlo_5000"]["error"]

    if D.rank == 0:
        result = {
            "metric": "ICP iterations/sec", "value": main_rec["value"], "unit": "iterations/s",
            "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "repeats": main_rec["repeats"], "timed_seconds": main_rec["timed_seconds"],
            "ms_per_step": main_rec["ms_per_step"], "ms_per_step_median": main_rec["ms_per_step_median"],
            "ms_per_step_min": main_rec["ms_per_step_min"], "ms_per_step_max": main_rec["ms_per_step_max"],
            "slowest_repeats": main_rec["slowest_repeats"],
            "higher_is_better": True, "scaling": "strong" if P.by_points else "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": main_rec["workload"] + (", ONE scan pair, source points split over the GPUs" if P.by_points else ", one scan pair per GPU"),
                       "n_src": int(P.n_src_total), "n_tgt": int(len(P.tgt)), "grid_cell_m": P.info.cell, "grid_cells": int(P.info.n_cells),
                       "parallelism": "%s x%d" % ("point-sharded" if P.by_points else "pair-sharded", n_gpus),
                       "rank_pair_seeds": [int(r[3]) for r in recs]},
            "correspondence_queries_per_s": main_rec["correspondence_queries_per_s"],
            "icp_iterations_per_step": main_rec["icp_iterations_per_step"],
            "roofline": main_rec["roofline"],
            "final_stats": {"mean_trans_error_m": float(np.mean(recs[:, 0])), "mean_rot_error_deg": float(np.mean(recs[:, 1])),
                            "mean_correspondences": float(np.mean(recs[:, 2]))},
        }
        if "roofline_valu_issue" in main_rec:
            result["roofline_valu_issue"] = main_rec["roofline_valu_issue"]
        if regimes is not None:
            result["roofline_by_regime"] = regimes
        if conv is not None:
            result["converged_run"] = conv
        if cold is not None:
            result["cold_run"] = cold
        if conc is not None:
            result["concurrent_pairs"] = conc
        if sub:
            result["configs"] = sub
        if n_gpus == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = guard("cpu_baseline", cpu_baseline, P.tgt, P.src, P.T_init, WORKLOADS[args.workload], args.method, args.cpu_seconds)
        if side_errors:
            result["side_leg_errors"] = side_errors
        result["host_threads"] = host_threads
        if args.full_record:
            with open(args.full_record, "w") as f:
                json.dump(result, f)
        print(json.dumps(compact_line(result)), flush=True)
    if n_gpus == 1:
        P.close()
        D.close()
    # a job of N ranks whose experiment did not gather records from N ranks is not a measurement of N GPUs: say so with the exit code.
    # (A Monte-Carlo job that failed outright is reported in the line - configs.c5_montecarlo_5000.error - and leaves the exit code alone:
    # the headline beside it has no data-path collective and stands by itself.)
    seen = None
    if D.rank == 0:
        seen = main_rec.get("rccl_ranks_seen") if P.mc else (sub.get("c5_montecarlo_5000") or {}).get("rccl_ranks_seen")
    if seen is not None and seen != n_gpus:
        sys.exit("bench.py: the Monte-Carlo experiment gathered records from %d rank(s), the job has %d" % (seen, n_gpus))


def _cpu_time_runs(po, tree, src, T_init, w, method, threads, budget_s):
    """iterations/s of the oracle stepping through the workload's runs with `threads` OpenMP threads, for ~budget_s seconds"""
    cfg = po.default_config(search_radius=w["radius"], max_iterations=1, thresh_rot=0.0, thresh_trans=0.0, kappa_target=10.0,
                            std_reg_gamma=100.0, use_weight_derivative=w["wd"], always_compute_schur=1, num_threads=threads)
    T = T_init.copy()
    po.icp_run(tree, src, T, method, cfg)       # warm-up (thread pool, page faults)
    n, run_len = 0, w["run_len"]
    c0, t0 = os.times(), time.perf_counter()
    while True:
        res, _ = po.icp_run(tree, src, T, method, cfg)
        T = np.eye(4); T[:3, :3] = np.array(res.R[:]).reshape(3, 3); T[:3, 3] = res.t[:]
        n += 1
        if n % run_len == 0:
            T = T_init.copy()
        el = time.perf_counter() - t0
        if el > budget_s or n >= 100 * run_len:
            break
    c1 = os.times()
    busy = ((c1.user + c1.system) - (c0.user + c0.system)) / max(el, 1e-9)
    return n / el, n, el, busy


def cpu_baseline(tgt, src, T_init, w, method, budget_s):
    """The CPU oracle (oracle/, a C/OpenMP restatement of the reference path; the reference itself needs Eigen/PCL/FLANN and cannot be
    built here) timed on this box's host cores on a bounded sample of the SAME workload, the way SURVEY 8d asks: (i) the reference's
    own configuration - ONE pair, the 8 OpenMP threads it hard-codes (:1714) - = `value`, (ii) every CPU this container may use, and
    (iii) the C1 fixture with 8 threads next to the 0.60-0.71 ms per iteration the reference published for it (fig8_5000iters/
    statistics_summary.txt:12-16), which shows the oracle is no strawman."""
    from oracle import pyoracle as po
    from dcreg_amd import hostinfo, scenes
    tree = po.KdTree(tgt)                       # kd-tree build is untimed in the reference too (:408-442)
    ncpu = os.cpu_count() or 1
    usable = hostinfo.usable_cpus()
    quota = hostinfo.cgroup_cpu_quota()
    t8 = min(8, usable)
    v8, n8, el8, busy8 = _cpu_time_runs(po, tree, src, T_init, w, method, t8, budget_s * 0.5)
    out = {"value": v8, "unit": "iterations/s", "cores": t8, "kind": "port",
           "sample": "%d ICP iterations of the same scan pair (%d-pt source, the first %d of a %d-iteration run from the same initial pose), "
                     "one pair at a time, OpenMP x%d (%.1f CPUs busy on average; the box shows %d hardware threads, usable %d, cgroup CPU "
                     "quota %s), %.1f s" % (n8, len(src), min(n8, w["run_len"]), w["run_len"], t8, busy8, ncpu, usable,
                                            ("%.1f" % quota) if quota else "none", el8)}
    if usable > t8:
        va, na, ela, busya = _cpu_time_runs(po, tree, src, T_init, w, method, usable, budget_s * 0.3)
        out["all_cores"] = {"value": va, "unit": "iterations/s", "cores": usable,
                            "sample": "%d iterations of the same runs, OpenMP x%d (%.1f CPUs busy), %.1f s" % (na, usable, busya, ela)}
    # C1 anchor: the fixture, the paper run's initial pose, 8 threads
    pts = scenes.cylinder_cloud()
    w1 = WORKLOADS["c1_fixture_7562"]
    T1 = scenes.pose6d_matrix(**scenes.PAPER_INIT)
    v1, n1, el1, busy1 = _cpu_time_runs(po, po.KdTree(pts), pts, T1, w1, method, t8, budget_s * 0.2)
    out["c1_anchor"] = {"ms_per_iteration": 1e3 / v1, "cores": t8, "reference_published_ms_per_iteration": [0.60, 0.71],
                        "reference_source": "DCReg/results/simulation/fig8_5000iters/statistics_summary.txt:12-16 (the authors' CPU, 8 OpenMP threads)",
                        "sample": "%d iterations of the 7562-pt fixture pair (30-iteration runs from the paper's initial pose), %.1f s" % (n1, el1)}
    return out


if __name__ == "__main__":
    main()
