// TEST INFRASTRUCTURE ONLY: host replay of the verification call's per-point function (dcreg_amd/csrc/device/verify.hpp: verify_point -
// transform, the finite test, the bounded 1-NN search from HeapOne's start key, the strict gate, the integer term) on the index emul.cpp
// builds, in a library of its own (tests/emul_verify.py).  The replay's own C-ABI (emul.cpp) comes along unchanged.
#include "emul.cpp"
#include "../../dcreg_amd/csrc/device/verify.hpp"

extern "C" {

// n_poses poses (12 doubles each: R row-major, t) of the n points at pts (3 floats each), inlier distance d.  Per (pose, point), pose-major:
// inl (0 / 1), nn (the nearest map point's original index, -1 for no inlier), d2 (+inf for no inlier), e.  evals: candidates evaluated.
int emu_verify(void *idx, const float *pts, int64_t n, const double *poses, int64_t n_poses, double d, uint8_t *inl, int32_t *nn, float *d2,
               uint64_t *e, int64_t *evals) {
    EmuIndex *E = (EmuIndex *)idx;
    const GridDev &g = E->g;
    // (the bound and the rings restate normal_icp.hip one_nn_bound and scratch.hip rings_for_bound, which verify.hip calls: host code the
    // replay cannot link - keep the three in step; tests/test_gpu_verify.py's lattice case checks the library's own)
    VerifyArgs a;
    a.dd = d * d;
    float bound = (float)a.dd;
    if ((double)bound < a.dd) bound = std::nextafterf(bound, INFINITY);
    if (!(bound <= 3.0e38f)) bound = 3.0e38f;
    a.bound_f = bound;
    int kk = 1;
    while (kk < 100000) { const double sd = (double)kk * g.h * (1.0 - 1e-9); if (sd * sd * (1.0 - 1e-6) >= (double)bound) break; ++kk; }
    a.max_ring = kk < 100000 ? kk : -1;
    static thread_local RunList runs;
    threadIdx.x = 0;
    int64_t ev = 0;
    for (int64_t k = 0; k < n_poses; ++k) {
        PoseArg P{};
        std::memcpy(P.R, poses + 12 * k, sizeof(P.R)); std::memcpy(P.t, poses + 12 * k + 9, sizeof(P.t));
        for (int64_t i = 0; i < n; ++i) {
            const float4 s4{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __uint_as_float((uint32_t)i)};
            VerifyPoint o;
            const bool in = verify_point(g, runs, P, a, s4, o);
            const size_t at = (size_t)k * (size_t)n + (size_t)i;
            inl[at] = in ? 1 : 0; nn[at] = o.idx == kNoIdx ? -1 : (int32_t)o.idx; d2[at] = o.d2; e[at] = o.e;
            ev += o.n_eval;
        }
    }
    if (evals) *evals = ev;
    return 0;
}

}
