"""Child process of tests/test_gpu_torch_seam.py: torch tensors and torch streams handed to the C-ABI.  One case per process:

    python tests/torch_seam_child.py views | side_stream | order_side | order_default | order_rows

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


def frozen(x):
    """a result as something == compares bitwise: arrays and floats by their bytes, containers element by element"""
    if isinstance(x, dict):
        return tuple((k, frozen(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (float, np.floating)):
        return np.float64(x).tobytes()
    return x


def case_order_rows():
    """ordering() for the device inputs that do not pass through upload_cloud - kept normals given from device memory, descriptor rows,
    correspondence arrays: the tensor holds A, B is copied into it behind ~75 ms of device sleep on the caller's stream with no host
    synchronise, and the call must answer bitwise what the host form answers for B.  On torch's default stream with a context never
    given a stream and one after set_stream(0), and on a side stream handed over with set_stream."""
    rng = np.random.default_rng(11)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # kept normals: 257 points (two blocks of the pack kernel), stride 4 with a NaN fourth column
    n = 257
    tgt = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    src = rng.uniform(-5, 5, (n, 3)).astype(np.float32)

    def unit(m):
        v = rng.normal(size=(m, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    nrm_a, nrm_b = unit(n), unit(n)
    nrm_b[5] = np.nan                                               # (a point without a normal is kept as given)
    # descriptor rows: a 65 x 33 at stride 36 (NaN padding), b 64 x 33 at stride 33; one invalid row on either side
    def rows(m, stride):
        f = np.full((m, stride), np.nan, np.float32)
        f[:, :33] = rng.uniform(0, 100, (m, 33)).astype(np.float32)
        f[m // 2, 7] = np.nan
        return f
    fa_a, fa_b, fb_a, fb_b = rows(65, 36), rows(65, 36), rows(64, 33), rows(64, 33)
    # a rigid scene of 40 points and 40 pairs, 10 of them wrong (B); A: every pair wrong
    m = 40
    pa = rng.uniform(-5, 5, (m, 3)).astype(np.float32)
    T = h.pose6d_matrix(1.0, -2.0, 0.5, 0.1, -0.2, 0.7)
    pb = (pa.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    ca_b = np.arange(m, dtype=np.int32)
    cb_b = ca_b.copy()
    cb_b[:10] = np.roll(cb_b[:10], 3)
    ca_a, cb_a = ca_b[::-1].copy(), np.roll(ca_b, 7)
    ap, cp = api.align_params(n_hypotheses=4096), api.consensus_params(n_seeds=8)

    # ---- the host forms' answers for B (and for A: the case must be able to tell them apart)
    hc = api.Context(0)
    hc.set_target(tgt, 1.0); hc.set_source(src)

    def host(na, fa, fb, ca, cb):
        hc.set_target_normals(na); hc.set_source_normals(na)
        al, co = hc.align_correspondences(pa, pb, ca, cb, ap), hc.consensus_correspondences(pa, pb, ca, cb, cp)
        return dict(target_normals=frozen(hc.kept_target_normals()), source_normals=frozen(hc.kept_source_normals()),
                    match=frozen(hc.feature_match(fa, fb)), align=frozen(al), consensus=frozen(co))
    want, other = host(nrm_b, fa_b, fb_b, ca_b, cb_b), host(nrm_a, fa_a, fb_a, ca_a, cb_a)
    hc.close()
    for k in want:
        assert want[k] != other[k], "%s: A and B give one answer: the case proves nothing" % k

    # ---- the device buffers and their late values
    x = torch.full((n, 4), float("nan"), device="cuda")
    nv = x[:, :3]
    assert nv.stride() == (4, 1)
    f_a, f_b = torch.empty((65, 36), device="cuda"), torch.empty((64, 33), device="cuda")
    d_ca, d_cb = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")
    d_pa, d_pb = dev(pa), dev(pb)
    late = dict(nrm=[(nv, dev(nrm_b))], rows=[(f_a, dev(fa_b)), (f_b, dev(fb_b))], corr=[(d_ca, dev(ca_b)), (d_cb, dev(cb_b))])
    early = dict(nrm=[(nv, dev(nrm_a))], rows=[(f_a, dev(fa_a)), (f_b, dev(fb_a))], corr=[(d_ca, dev(ca_a)), (d_cb, dev(cb_a))])
    o_idx, o_idx2 = torch.empty(65, dtype=torch.int32, device="cuda"), torch.empty(65, dtype=torch.int32, device="cuda")
    o_d, o_d2 = torch.empty(65, dtype=torch.float64, device="cuda"), torch.empty(65, dtype=torch.float64, device="cuda")
    o_mut, o_mask = torch.empty(65, dtype=torch.uint8, device="cuda"), torch.empty(m, dtype=torch.uint8, device="cuda")
    host_of = lambda t: t.cpu().numpy()
    cycles = sleep_cycles(75.0)

    def call_normals(c, which):
        getattr(c, "set_%s_normals" % which)(dev_ptr=nv.data_ptr(), n=n, stride=4)
        return frozen(getattr(c, "kept_%s_normals" % which)())

    def call_match(c):
        info = c.feature_match_device(f_a.data_ptr(), 65, 36, f_b.data_ptr(), 64, 33, o_idx.data_ptr(), o_d.data_ptr(), o_idx2.data_ptr(), o_d2.data_ptr(),
                                      o_mut.data_ptr())
        return frozen(dict(info, idx=host_of(o_idx), d=host_of(o_d), idx2=host_of(o_idx2), d2=host_of(o_d2), mutual=host_of(o_mut)))

    def call_corr(c, which, params):
        r = getattr(c, which + "_correspondences_device")(d_pa.data_ptr(), m, 3, d_pb.data_ptr(), m, 3, d_ca.data_ptr(), d_cb.data_ptr(), m, params,
                                                          dev_mask=o_mask.data_ptr())
        return frozen(dict(r, mask=host_of(o_mask)))
    calls = [("target_normals", "nrm", lambda c: call_normals(c, "target")), ("source_normals", "nrm", lambda c: call_normals(c, "source")),
             ("match", "rows", call_match), ("align", "corr", lambda c: call_corr(c, "align", ap)),
             ("consensus", "corr", lambda c: call_corr(c, "consensus", cp))]

    assert torch.cuda.current_stream().cuda_stream == 0
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    for name, S, stream_arg in (("never given a stream", torch.cuda.current_stream(), None), ("after set_stream(0)", torch.cuda.current_stream(), 0),
                                ("on a side stream", side, side.cuda_stream)):
        c = api.Context(0)
        if stream_arg is not None:
            c.set_stream(stream_arg)
        c.set_target(tgt, 1.0); c.set_source(src)
        for key, inputs, call in calls:
            for buf, val in early[inputs]:
                buf.copy_(val)
            torch.cuda.synchronize()
            ev = torch.cuda.Event()
            with torch.cuda.stream(S):
                torch.cuda._sleep(cycles)
                for buf, val in late[inputs]:
                    buf.copy_(val)
                ev.record(S)
            assert not ev.query(), "the copy finished before the call: the case proves nothing"
            got = call(c)
            assert got == want[key], "%s, context %s: the call did not read what was written before it" % (key, name)
            torch.cuda.synchronize()
        c.close()


CASES = {"views": case_views, "side_stream": case_side_stream, "order_side": lambda: ordering(True), "order_default": lambda: ordering(False),
         "order_rows": case_order_rows}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    torch.cuda.synchronize()
    print("ok", sys.argv[1])
