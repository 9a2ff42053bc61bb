// TEST INFRASTRUCTURE ONLY: host replay of the second and third engine's per-point functions WITH A ROBUST KERNEL
// (dcreg_amd/csrc/device/normal_icp.hpp: nlin_point; gicp.hpp: glin_point, glin_row, glin_row_scale) on the index emul.cpp builds, in a
// library of its own (tests/emul_robust.py).  The calls are emu_nlin's and emu_glin's (emul_nlin.cpp, emul_glin.cpp) with the kernel's two
// launch arguments added: kind ("robust_kernel") and c (the scale; c * c is formed here, once, as the host forms it for a launch).
#include "emul.cpp"
#include "../../dcreg_amd/csrc/device/gicp.hpp"

namespace {
template <class Args>
void search_args(Args &a, const GridDev &g, double radius) {
    a.radius_sq = radius * radius;
    float bound = (float)a.radius_sq;
    if ((double)bound < a.radius_sq) bound = std::nextafterf(bound, INFINITY);
    if (!(bound <= 3.0e38f)) bound = 3.0e38f;
    a.bound_f = bound;
    int kk = 1;
    while (kk < 100000) { const double sd = (double)kk * g.h * (1.0 - 1e-9); if (sd * sd * (1.0 - 1e-6) >= (double)bound) break; ++kk; }
    a.max_ring = kk;
}
}  // namespace

extern "C" {

int emu_nlin_robust(void *idx, const float *normals4, const float *src, const uint32_t *order, int64_t n, const double *R, const double *t,
                    double radius, double w_slope, double w_min, int use_wd, int kind, double c, uint32_t *warm, int use_warm, int32_t *nn_idx,
                    float *nn_d2, uint8_t *flag, double *normal, double *r, double *s, double *row, double *sums, int64_t *evals) {
    EmuIndex *E = (EmuIndex *)idx;
    const GridDev &g = E->g;
    NlinArgs a;
    search_args(a, g, radius);
    a.w_slope = w_slope; a.w_min = w_min; a.use_wd = use_wd;
    a.robust = kind; a.robust_c2 = c * c;
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

int emu_glin_robust(void *idx, const float *normals4, const float *src, const float *src_normals4, const uint32_t *order, int64_t n,
                    const double *R, const double *t, double radius, double eps, int kind, double c, uint32_t *warm, int use_warm,
                    int32_t *nn_idx, float *nn_d2, uint8_t *flag, double *normal_map, double *normal_src, double *w, double *r, double *row,
                    double *sums, int64_t *evals) {
    EmuIndex *E = (EmuIndex *)idx;
    const GridDev &g = E->g;
    GlinArgs a;
    search_args(a, g, radius);
    a.c = 1.0 - eps;
    a.robust = kind; a.robust_c2 = c * c;
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
            if (f == 1) {
                glin_row(P, (double)s4.x, (double)s4.y, (double)s4.z, o.w[k][0], o.w[k][1], o.w[k][2], o.e[0], o.e[1], o.e[2], rw);
                if (a.robust) glin_row_scale(o.k, rw);
            }
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
