// TEST INFRASTRUCTURE ONLY: host replay of the third engine's per-point functions (dcreg_amd/csrc/device/gicp.hpp: glin_point - the 1-NN
// search with its warm bound, the gates, the covariance, its factor and W - and glin_row) on the index emul.cpp builds, in a library of
// its own (tests/emul_glin.py).  The replay's own C-ABI (emul.cpp) comes along unchanged.
#include "emul.cpp"
#include "../../dcreg_amd/csrc/device/gicp.hpp"

extern "C" {

// One linearisation over the n source points at src (processing order, 3 floats each; order[i] = the point's original index).  normals4:
// float4 per map point in index order; src_normals4: float4 per source point in PROCESSING order.  warm: n words in / out (the sorted
// positions of the last nearest neighbours), or null; use_warm 0 searches every point cold (the words are still written).  The dump
// arrays are in original source order; sums: the 31 sums added row by row in processing order; evals: candidates evaluated.
int emu_glin(void *idx, const float *normals4, const float *src, const float *src_normals4, const uint32_t *order, int64_t n, const double *R,
             const double *t, double radius, double eps, uint32_t *warm, int use_warm, int32_t *nn_idx, float *nn_d2, uint8_t *flag,
             double *normal_map, double *normal_src, double *w, double *r, double *row, double *sums, int64_t *evals) {
    EmuIndex *E = (EmuIndex *)idx;
    const GridDev &g = E->g;
    GlinArgs a;
    a.radius_sq = radius * radius;
    float bound = (float)a.radius_sq;
    if ((double)bound < a.radius_sq) bound = std::nextafterf(bound, INFINITY);
    if (!(bound <= 3.0e38f)) bound = 3.0e38f;
    a.bound_f = bound;
    int kk = 1;
    while (kk < 100000) { const double sd = (double)kk * g.h * (1.0 - 1e-9); if (sd * sd * (1.0 - 1e-6) >= (double)bound) break; ++kk; }
    a.max_ring = kk;
    a.c = 1.0 - eps;
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
        const float4 m4{src_normals4[4 * i], src_normals4[4 * i + 1], src_normals4[4 * i + 2], src_normals4[4 * i + 3]};
        GlinPoint o;
        const uint8_t f = glin_point(g, runs, (const float4 *)normals4, P, a, s4, &m4, (warm && use_warm) ? warm[i] : kNoIdx, o);
        if (warm) warm[i] = o.pos;
        ev += o.n_eval;
        nn_idx[oi] = o.idx == kNoIdx ? -1 : (int32_t)o.idx;
        nn_d2[oi] = o.d2; flag[oi] = f;
        for (int k = 0; k < 3; ++k) {
            normal_map[3 * (size_t)oi + k] = o.n[k]; normal_src[3 * (size_t)oi + k] = o.m[k];
            for (int j = 0; j < 3; ++j) w[9 * (size_t)oi + 3 * k + j] = o.w[k][j];
        }
        for (int k = 0; k < 3; ++k) {
            double rw[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (f == 1) glin_row(P, (double)s4.x, (double)s4.y, (double)s4.z, o.w[k][0], o.w[k][1], o.w[k][2], o.e[0], o.e[1], o.e[2], rw);
            r[3 * (size_t)oi + k] = rw[7];
            for (int j = 0; j < 8; ++j) row[(3 * (size_t)oi + k) * 8 + j] = rw[j];
            row_products(rw, f, acc);
            for (int j = 0; j < 29; ++j) sums[j] += acc[j];
        }
        sums[29] += f == 1 ? 1.0 : 0.0;
        sums[30] += f != 0 ? 1.0 : 0.0;
    }
    if (evals) *evals = ev;
    return 0;
}

}
