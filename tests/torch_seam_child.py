"""Child process of tests/test_gpu_torch_seam.py: torch tensors and torch streams handed to the C-ABI.  One case per process:

    python tests/torch_seam_child.py views | side_stream | order_side | order_default

torch is imported and device 0 initialised BEFORE the library is loaded, so that both bind the one HIP runtime already mapped (torch
bundles its own libamdhip64.so.7); a process that has two of them mapped stops (EXIT_TWO_RUNTIMES) before any pointer or stream reaches
the library.  Exit status 0 = the case held; an AssertionError exits 1 with its traceback on stderr."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

EXIT_TWO_RUNTIMES = 3

import numpy as np          # noqa: E402
import torch                # noqa: E402

torch.cuda.init()
torch.zeros(1, device="cuda:0")
torch.cuda.synchronize()

from dcreg_amd import api    # noqa: E402
import helpers as h          # noqa: E402

api.load()
_maps = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
if len(_maps) != 1:
    sys.stderr.write("torch_seam_child: %d HIP runtimes mapped (%s): no pointer or stream may cross between them\n" % (len(_maps), _maps))
    sys.exit(EXIT_TWO_RUNTIMES)

CFG = dict(search_radius=1.0, max_iterations=20, KAPPA_TARGET=10.0, STD_REG_GAMMA=100.0, use_weight_derivative=1, always_compute_schur=1)
PRM = api.default_lin_params(1.0, 1)


def scene():
    tgt, src = h.scene_parkinglot()
    T = h.pose6d_matrix(**h.PK01_GT)
    poses = [T @ h.pose6d_matrix(*d) for d in ([0, 0, 0, 0, 0, 0], [0.05, -0.03, 0.02, 2e-3, -1e-3, 3e-3], [-0.2, 0.1, -0.05, -4e-3, 2e-3, 8e-3])]
    return np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32), poses


def results(ctx, poses):
    """what a caller sees: three linearisations, an ICP run, the p2p error"""
    lin = [ctx.linearize(T[:3, :3], T[:3, 3], PRM) for T in poses]
    res, logs = ctx.icp_run(poses[2], "Ours", api.default_config(**CFG))
    return dict(lin=[(o["n_eff"], o["n_pt"], o["H_upper"].tobytes(), o["g"].tobytes(), o["sum_r2"], o["sum_b2"]) for o in lin],
                icp=(res.converged, res.iterations, res.status, bytes(res.R), bytes(res.t), bytes(res.icp_cov),
                     [bytes(L.H_upper) for L in logs]),
                p2p=ctx.p2p_error(poses[1], 0.3))


def host_results(tgt, src, poses):
    c = api.Context(0)
    c.set_target(tgt, 1.0); c.set_source(src)
    r = results(c, poses)
    c.close()
    return r


def same(a, b, what):
    for k in a:
        assert a[k] == b[k], "%s: %s differs" % (what, k)


def case_views():
    """tensor views: the xyz columns of an [N, 4] tensor (stride 4), a tensor one row into its storage, a tensor from numpy"""
    tgt, src, poses = scene()
    want = host_results(tgt, src, poses)
    x = torch.full((len(tgt), 4), float("nan"), device="cuda")
    x[:, :3] = torch.from_numpy(tgt).cuda()
    v = x[:, :3]
    assert v.stride() == (4, 1) and v.data_ptr() == x.data_ptr()
    y = torch.cat([torch.full((1, 3), 1e30), torch.from_numpy(src)]).cuda()
    w = y[1:]
    assert w.stride() == (3, 1) and w.data_ptr() == y.data_ptr() + 12
    z = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    for tv, sv in ((v, w), (v, z)):
        c = api.Context(0)
        c.set_target_device(tv.data_ptr(), tv.shape[0], tv.stride(0), 1.0)
        c.set_source_device(sv.data_ptr(), sv.shape[0], sv.stride(0))
        same(results(c, poses), want, "tensor views")
        c.close()


def case_side_stream():
    """a context on a torch side stream gives bitwise the records of one on its own stream - the gated pipeline (icp_run), batched
    launches, register_frames, p2p - and set_stream(0) returns it to its own stream with the same results"""
    tgt, src, poses = scene()
    rng = np.random.default_rng(3)
    Ts = [poses[0] @ h.pose6d_matrix(*rng.uniform(-4, 4, 2), 0.0, 0.0, 0.0, h.deg2rad(rng.uniform(-10, 10))) for _ in range(5)]
    frames = h.map_frames(tgt, Ts, [6000, 200, 3000, 65, 1000], seed=4)
    cfg = api.default_config(**CFG)

    def run(ctx):
        r = results(ctx, poses)
        r["batch"] = [(o["n_eff"], o["H_upper"].tobytes(), o["g"].tobytes()) for o in ctx.linearize_batch(np.stack([T[:3, :3] for T in poses]),
                                                                                                           np.stack([T[:3, 3] for T in poses]), PRM)]
        r["frames"] = [(f.iterations, f.converged, f.status, bytes(f.final_transform), bytes(f.H_upper), f.final_rmse)
                       for f in ctx.register_frames(frames, Ts, "Ours", cfg, slots=2)]
        return r
    own = api.Context(0)
    own.set_target(tgt, 1.0); own.set_source(src)
    want = run(own)
    own.close()
    S = torch.cuda.Stream()
    assert S.cuda_stream != 0
    c = api.Context(0)
    c.set_stream(S.cuda_stream)
    c.set_target(tgt, 1.0); c.set_source(src)
    same(run(c), want, "side stream")
    c.set_stream(0)
    c.set_target(tgt, 1.0); c.set_source(src)
    same(run(c), want, "back on the own stream")
    c.close()


def sleep_cycles(ms):
    """torch.cuda._sleep cycles that take about `ms` on this device (the count's rate differs between platforms: measured here)"""
    k = 1 << 20
    for _ in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); torch.cuda._sleep(k); b.record(); b.synchronize()
        t = a.elapsed_time(b)
        if t >= 5.0:
            return max(1, int(k * ms / t))
        k *= 8
    raise AssertionError("torch.cuda._sleep did not take measurable time (%.3f ms for %d cycles)" % (t, k))


def ordering(on_side_stream):
    """cloud A in a tensor, then - queued behind ~75 ms of device sleep on the caller's stream, no host synchronise - cloud B copied into
    it: set_source_device must read B.  The event recorded after the copy must still be pending when the call is made."""
    tgt, src_b, poses = scene()
    src_a = (src_b[::-1] * np.float32(0.8) + np.float32(0.5)).copy()
    want = host_results(tgt, src_b, poses)
    cycles = sleep_cycles(75.0)
    buf = torch.from_numpy(src_a).cuda()
    b_dev = torch.from_numpy(src_b).cuda()
    S = torch.cuda.Stream() if on_side_stream else torch.cuda.current_stream()
    ctxs = []
    if on_side_stream:
        c = api.Context(0)
        c.set_stream(S.cuda_stream)
        ctxs.append(c)
    else:
        assert torch.cuda.current_stream().cuda_stream == 0
        ctxs.append(api.Context(0))                                  # never given a stream
        c = api.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)         # = 0: its own stream
        ctxs.append(c)
    for c in ctxs:
        c.set_target(tgt, 1.0)
        buf.copy_(torch.from_numpy(src_a).cuda())
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        with torch.cuda.stream(S):
            torch.cuda._sleep(cycles)
            buf.copy_(b_dev)
            ev.record(S)
        assert not ev.query(), "the copy finished before the call: the case proves nothing"
        c.set_source_device(buf.data_ptr(), buf.shape[0], 3)
        same(results(c, poses), want, "ordering on the %s stream" % ("side" if on_side_stream else "default"))
        torch.cuda.synchronize()
        c.close()


CASES = {"views": case_views, "side_stream": case_side_stream, "order_side": lambda: ordering(True), "order_default": lambda: ordering(False)}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    torch.cuda.synchronize()
    print("ok", sys.argv[1])
