// TEST INFRASTRUCTURE ONLY: host replay of the second engine's per-point function (dcreg_amd/csrc/device/normal_icp.hpp: nlin_point - the
// 1-NN search with its warm bound, the gates, the row) on the index emul.cpp builds, in a library of its own (tests/emul_nlin.py).  The
// replay's own C-ABI (emul.cpp) comes along unchanged.
#include "emul.cpp"
#include "../../dcreg_amd/csrc/device/normal_icp.hpp"

extern "C" {

// One linearisation over the n source points at src (processing order, 3 floats each; order[i] = the point's original index).  normals4:
// float4 per map point in index order.  warm: n words in / out (the sorted positions of the last nearest neighbours), or null; use_warm 0
// searches every point cold (the words are still written).  The dump arrays are in original source order; sums: the 31 sums added in
// processing order; evals: candidates evaluated by all searches.
int emu_nlin(void *idx, const float *normals4, const float *src, const uint32_t *order, int64_t n, const double *R, const double *t, double radius,
             double w_slope, double w_min, int use_wd, uint32_t *warm, int use_warm, int32_t *nn_idx, float *nn_d2, uint8_t *flag, double *normal,
             double *r, double *s, double *row, double *sums, int64_t *evals) {
    EmuIndex *E = (EmuIndex *)idx;
    const GridDev &g = E->g;
    NlinArgs a;
    a.radius_sq = radius * radius;
    float bound = (float)a.radius_sq;
    if ((double)bound < a.radius_sq) bound = std::nextafterf(bound, INFINITY);
    if (!(bound <= 3.0e38f)) bound = 3.0e38f;
    a.bound_f = bound;
    int kk = 1;
    while (kk < 100000) { const double sd = (double)kk * g.h * (1.0 - 1e-9); if (sd * sd * (1.0 - 1e-6) >= (double)bound) break; ++kk; }
    a.max_ring = kk;
    a.w_slope = w_slope; a.w_min = w_min; a.use_wd = use_wd;
    PoseArg P{};
    std::memcpy(P.R, R, sizeof(P.R)); std::memcpy(P.t, t, sizeof(P.t));
    static thread_local RunList runs;
    threadIdx.x = 0;
    double acc[31];
    for (int k = 0; k < 31; ++k) sums[k] = 0.0;
    int64_t ev = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t oi = order[i];
        const float4 s4{src[3 * i], src[3 * i + 1], src[3 * i + 2], __uint_as_float(oi)};
        double rw[8];
        NlinPoint o;
        const uint8_t f = nlin_point(g, runs, (const float4 *)normals4, P, a, s4, (warm && use_warm) ? warm[i] : kNoIdx, rw, o);
        if (warm) warm[i] = o.pos;
        ev += o.n_eval;
        nn_idx[oi] = o.idx == kNoIdx ? -1 : (int32_t)o.idx;
        nn_d2[oi] = o.d2; flag[oi] = f;
        for (int k = 0; k < 3; ++k) normal[3 * (size_t)oi + k] = o.n[k];
        r[oi] = o.r; s[oi] = o.s;
        for (int k = 0; k < 8; ++k) row[8 * (size_t)oi + k] = rw[k];
        row_products(rw, f, acc);
        for (int k = 0; k < 31; ++k) sums[k] += acc[k];
    }
    if (evals) *evals = ev;
    return 0;
}

}
