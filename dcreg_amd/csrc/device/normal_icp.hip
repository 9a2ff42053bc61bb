// The second engine's linearisation on the device (include/dcreg.h: dcreg_linearize_normals): 1-NN point-to-plane rows against the map's
// kept normals, with the rule of the header, bitwise the numpy reference of tests/normal_icp_ref.py.
//   k_nlin<DUMP>   one lane per source point, in the context's curve order: nlin_point (normal_icp.hpp) - transform, the ring walk of k_knn
//                  with a one-slot heap on (d2, index) keys, started from the bound the point's last nearest neighbour gives when there is
//                  one, one gather of the nearest point and one of its float4 normal, the row; then the wave's rows on the matrix cores
//                  (kernels.hpp wave_gram_mfma) and the block row in LDS, added in wave order
//   k_finalize     (kernels.hpp) the block rows in chunk order, the additions of the first engine's batched launches
// No floating-point atomics anywhere: the sums are a function of the rows and their order.  A point's row depends on the clouds, the
// normals and the pose only; the warm position decides how fast the neighbour is found, never which.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../../include/dcreg_debug.h"
#include "context.hpp"
#include "normal_icp.hpp"

namespace dcreg {
namespace {

struct NlinDump {
    int32_t *nn_idx; float *nn_d2; uint8_t *flag; double *normal, *r, *s, *row;
};

// warm_in: the positions of the last launch (null: search cold), warm_out: where this launch leaves its own (null: nowhere; the same
// array as warm_in in a plain call: a lane reads its word before it writes it, and no other lane's).  Block b
// leaves its row at partials[b]: slots 0..28 the Gram entries of gram_entry_of_slot, 29 effective points, 30 points inside the radius
template <bool DUMP>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_nlin(const float4 *__restrict__ src, uint32_t n_src, GridDev g,
                                                                     const float4 *__restrict__ normals, PoseArg P, NlinArgs a,
                                                                     const uint32_t *warm_in, uint32_t *warm_out,
                                                                     double *__restrict__ partials, NlinDump d) {
    __shared__ RunList runs[kLinBlock / kWave];
    __shared__ double gm[kLinBlock / kWave][64];
    __shared__ double cnt[kLinBlock / kWave][2];
    const int wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kLinBlock + threadIdx.x;
    double row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = 0.0;
    uint8_t flag = 0;
    if (i < n_src) {
        const float4 s4 = src[i];
        NlinPoint o;
        flag = nlin_point(g, runs[wave], normals, P, a, s4, warm_in ? warm_in[i] : kNoIdx, row, o);
        if (warm_out) warm_out[i] = o.pos;
        if constexpr (DUMP) {
            const size_t oi = __float_as_uint(s4.w);
            if (d.nn_idx) d.nn_idx[oi] = o.idx == kNoIdx ? -1 : (int32_t)o.idx;
            if (d.nn_d2) d.nn_d2[oi] = o.d2;
            if (d.flag) d.flag[oi] = flag;
            if (d.normal) { d.normal[3 * oi] = o.n[0]; d.normal[3 * oi + 1] = o.n[1]; d.normal[3 * oi + 2] = o.n[2]; }
            if (d.r) d.r[oi] = o.r;
            if (d.s) d.s[oi] = o.s;
            if (d.row) {
#pragma unroll
                for (int j = 0; j < 8; ++j) d.row[8 * oi + j] = row[j];
            }
        }
    }
    // (the wave's RunList is free now: it stages the rows; the lanes past the cloud's end carry a zero row and flag 0)
    wave_rows_to_lds(row, flag, runs[wave].stage, gm[wave], cnt);
    __syncthreads();
    if (threadIdx.x < kSlots) {
        double t = 0.0;
        if (threadIdx.x < 29) {
            const int e = gram_entry_of_slot(threadIdx.x);
#pragma unroll
            for (int w = 0; w < kLinBlock / kWave; ++w) t += gm[w][e];
        } else if (threadIdx.x < 31) {
#pragma unroll
            for (int w = 0; w < kLinBlock / kWave; ++w) t += cnt[w][threadIdx.x - 29];
        }
        partials[(size_t)blockIdx.x * kSlots + threadIdx.x] = t;
    }
}

bool finite_n(const double *v, int n) {
    for (int k = 0; k < n; ++k) if (!std::isfinite(v[k])) return false;
    return true;
}

int nlin_run(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, dcreg_lin_out *out, dcreg_nlin_debug *dbg) {
    if (!c) return DCREG_E_INVALID;
    if (!R || !t || !p || !out) { c->fail("null linearisation arguments"); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    if (p->parameterization != DCREG_PARAM_SO3) { c->fail("the normal linearisation has the SO(3) row only (parameterization %d)", p->parameterization); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->search_radius) && p->search_radius > 0.0)) { c->fail("search_radius is %g: finite and > 0 expected", p->search_radius); return DCREG_E_INVALID; }
    if (!finite_n(R, 9) || !finite_n(t, 3)) { c->fail("the pose is not finite"); return DCREG_E_INVALID; }
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    if (!c->nicp.kept) { c->fail("no kept normals: dcreg_target_normals_keep or dcreg_target_normals_set first"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    // the index a single-pose linearisation searches: the window of a capped map, as dcreg_linearize (a swap drops the warm positions)
    if (int rc = roi_ensure(c, R, t, p->search_radius)) return rc;
    dcreg_ctx::NormalIcpBufs &B = c->nicp;
    const int64_t n = c->n_src;
    const uint32_t nb = (uint32_t)((n + kLinBlock - 1) / kLinBlock);
    if (!B.warm.holds((size_t)n)) B.warm_valid = false;          // (a new array holds nothing)
    if (B.partials.ensure(c, (size_t)nb * kSlots) || B.d_out.ensure(c, kSlots) || B.warm.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
    NlinArgs a;
    a.radius_sq = p->search_radius * p->search_radius;
    float bound = (float)a.radius_sq;
    if ((double)bound < a.radius_sq) bound = std::nextafterf(bound, __builtin_inff());     // the smallest float >= R^2
    if (!(bound <= 3.0e38f)) bound = 3.0e38f;
    a.bound_f = bound;
    a.max_ring = outlier_rings(c->map.grid, bound);
    a.w_slope = p->weight_slope; a.w_min = p->weight_min; a.use_wd = p->use_weight_derivative;
    PoseArg P;
    std::memcpy(P.R, R, sizeof(P.R)); std::memcpy(P.t, t, sizeof(P.t));
    P.state = kNoIdx; P.fresh = 1;
    const GridDev &g = c->map.grid;
    if (dbg) {
        // one block of device memory for the dump, cut into its arrays (8-byte ones first)
        const size_t N = (size_t)n;
        const size_t off_normal = 0, off_r = off_normal + 24 * N, off_s = off_r + 8 * N, off_row = off_s + 8 * N, off_idx = off_row + 64 * N,
                     off_d2 = off_idx + 4 * N, off_flag = off_d2 + 4 * N, total = off_flag + N;
        if (B.dbg.ensure(c, total)) return DCREG_E_NOMEM;
        unsigned char *b = B.dbg.data();
        NlinDump d;
        d.normal = dbg->normal ? (double *)(b + off_normal) : nullptr; d.r = dbg->r ? (double *)(b + off_r) : nullptr;
        d.s = dbg->s ? (double *)(b + off_s) : nullptr; d.row = dbg->row ? (double *)(b + off_row) : nullptr;
        d.nn_idx = dbg->nn_idx ? (int32_t *)(b + off_idx) : nullptr; d.nn_d2 = dbg->nn_d2 ? (float *)(b + off_d2) : nullptr;
        d.flag = dbg->flag ? b + off_flag : nullptr;
        hipLaunchKernelGGL(k_nlin<true>, dim3(nb), dim3(kLinBlock), 0, c->stream, c->d_src.data(), (uint32_t)n, g, B.normals.data(), P, a,
                           (const uint32_t *)nullptr, (uint32_t *)nullptr, B.partials.data(), d);
        HIP_TRY(c, hipGetLastError());
        if (d.normal) HIP_TRY(c, hipMemcpyAsync(dbg->normal, d.normal, 24 * N, hipMemcpyDeviceToHost, c->stream));
        if (d.r) HIP_TRY(c, hipMemcpyAsync(dbg->r, d.r, 8 * N, hipMemcpyDeviceToHost, c->stream));
        if (d.s) HIP_TRY(c, hipMemcpyAsync(dbg->s, d.s, 8 * N, hipMemcpyDeviceToHost, c->stream));
        if (d.row) HIP_TRY(c, hipMemcpyAsync(dbg->row, d.row, 64 * N, hipMemcpyDeviceToHost, c->stream));
        if (d.nn_idx) HIP_TRY(c, hipMemcpyAsync(dbg->nn_idx, d.nn_idx, 4 * N, hipMemcpyDeviceToHost, c->stream));
        if (d.nn_d2) HIP_TRY(c, hipMemcpyAsync(dbg->nn_d2, d.nn_d2, 4 * N, hipMemcpyDeviceToHost, c->stream));
        if (d.flag) HIP_TRY(c, hipMemcpyAsync(dbg->flag, d.flag, N, hipMemcpyDeviceToHost, c->stream));
    } else {
        const bool warm = c->opt_warm && B.warm_valid;
        B.warm_valid = false;                 // (until the launch is known to have run)
        hipLaunchKernelGGL(k_nlin<false>, dim3(nb), dim3(kLinBlock), 0, c->stream, c->d_src.data(), (uint32_t)n, g, B.normals.data(), P, a,
                           warm ? B.warm.data() : (const uint32_t *)nullptr, B.warm.data(), B.partials.data(), NlinDump{});
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_finalize<false>, dim3(1), dim3(kLinBlock), 0, c->stream, B.partials.data(), nb, B.d_out.data(), 0ull, (const uint2 *)nullptr);
    HIP_TRY(c, hipGetLastError());
    double h[kSlots];
    HIP_TRY(c, hipMemcpyAsync(h, B.d_out.data(), sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (!dbg) B.warm_valid = true;
    std::memcpy(out->H_upper, h, 21 * sizeof(double));
    std::memcpy(out->g, h + 21, 6 * sizeof(double));
    out->sum_r2 = h[27]; out->sum_b2 = h[28];
    out->n_eff = (int64_t)std::llround(h[29]); out->n_pt = (int64_t)std::llround(h[30]);
    return DCREG_OK;
}

}  // namespace
}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_linearize_normals(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out) {
    return nlin_run(c, R, t, p, out, nullptr);
}
int dcreg_linearize_normals_debug(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out,
                                  dcreg_nlin_debug *dbg) {
    if (c && !dbg) { c->fail("null dump"); return DCREG_E_INVALID; }
    return nlin_run(c, R, t, p, out, dbg);
}
}
