// Verification of candidate poses against the map (include/dcreg.h: dcreg_verify_poses, _cloud, _cloud_device): P poses of one cloud
// scored in ONE launch, integer count and cost per pose, bitwise the numpy reference of tests/verify_ref.py.
//   k_verify_flag_src / _rows   the selection flags of the resident source (curve order, the original index in w) / of a caller's rows
//                               (finite and i % s == 0), n + 1 entries, the last 0; scan_u32 (scratch.hip) numbers the selected points
//   k_verify_gather_src / _rows the selected points compacted, w = the original index
//   k_verify<DETAIL>            block (x, k): 256 selected points at pose k - verify_point (verify.hpp) per lane, the wave's count by
//                               ballot + popcount, its cost by a 64-bit butterfly, the four waves in LDS, ONE pair of 64-bit integer
//                               atomics per block into acc[k] (integer adds commute: the sums are bitwise whatever the order).  The pose is
//                               read from a table through an address that depends on blockIdx.y alone: scalar loads, the twelve doubles
//                               live in scalar registers.  DETAIL: the block row of the detail pose also writes mask and nn at the
//                               points' original indices
// The rank is a host sort of the P downloaded {count, cost} pairs.  No floating-point atomics anywhere.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "context.hpp"
#include "verify.hpp"

namespace dcreg {
namespace {

constexpr int64_t kVerifyMaxPoses = DCREG_VERIFY_MAX_POSES;

// resident source: src in curve order, w = the original index; flag[n] = 0
static __global__ void k_verify_flag_src(const float4 *__restrict__ src, int64_t n, uint32_t stride, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    flag[i] = (i < n && __float_as_uint(src[i].w) % stride == 0u) ? 1u : 0u;
}
static __global__ void k_verify_gather_src(const float4 *__restrict__ src, int64_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                           float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    out[pos[i]] = src[i];
}
// a caller's rows: row i is selected when i % stride == 0 and scored when its coordinates are finite as well
static __global__ void k_verify_flag_rows(const float *__restrict__ xyz, int64_t n, int64_t row_stride, int64_t stride, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    uint32_t f = 0u;
    if (i < n && i % stride == 0) {
        const float *r = xyz + i * row_stride;
        f = finite_xyz(r[0], r[1], r[2]) ? 1u : 0u;
    }
    flag[i] = f;
}
static __global__ void k_verify_gather_rows(const float *__restrict__ xyz, int64_t n, int64_t row_stride, const uint32_t *__restrict__ flag,
                                            const uint32_t *__restrict__ pos, float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const float *r = xyz + i * row_stride;
    out[pos[i]] = make_float4(r[0], r[1], r[2], __uint_as_float((uint32_t)i));
}

// Block (x, k) of a launch over n_poses poses from `poses` (12 doubles each: R row-major, t) and the n_pts selected points at pts (w = the
// original index).  acc[2 k], acc[2 k + 1]: the pose's count and cost.  DETAIL: the blocks with blockIdx.y == detail write mask / nn (either
// may be null) at the original indices; the arrays were cleared to 0 / -1 before the launch.
template <bool DETAIL>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_verify(const float4 *__restrict__ pts, uint32_t n_pts, GridDev g,
                                                                       const double *__restrict__ poses, VerifyArgs a,
                                                                       unsigned long long *__restrict__ acc, uint32_t detail,
                                                                       uint8_t *__restrict__ mask, int32_t *__restrict__ nn) {
    __shared__ RunList runs[kLinBlock / kWave];
    __shared__ unsigned long long w_count[kLinBlock / kWave], w_cost[kLinBlock / kWave];
    const uint32_t k = blockIdx.y;
    const double *__restrict__ pk = poses + (size_t)k * 12;              // (wave-uniform: twelve scalar loads)
    PoseArg P;
#pragma unroll
    for (int j = 0; j < 9; ++j) P.R[j] = pk[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) P.t[j] = pk[9 + j];
    P.state = kNoIdx; P.fresh = 0u;
    const int wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kLinBlock + threadIdx.x;
    bool inl = false;
    unsigned long long e = 0ull;
    if (i < n_pts) {
        const float4 s4 = pts[i];
        VerifyPoint o;
        inl = verify_point(g, runs[wave], P, a, s4, o);
        e = o.e;
        if constexpr (DETAIL) {
            if (k == detail && inl) {
                const size_t oi = __float_as_uint(s4.w);
                if (mask) mask[oi] = 1;
                if (nn) nn[oi] = (int32_t)o.idx;
            }
        }
    }
    const unsigned long long votes = __ballot(inl);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) e += __shfl_xor(e, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) { w_count[wave] = (unsigned long long)__popcll(votes); w_cost[wave] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long cnt = 0ull, cost = 0ull;
#pragma unroll
        for (int w = 0; w < kLinBlock / kWave; ++w) { cnt += w_count[w]; cost += w_cost[w]; }
        if (cnt) {                                                       // (no inlier: no term either, nothing to add)
            atomicAdd(&acc[2 * (size_t)k], cnt);
            atomicAdd(&acc[2 * (size_t)k + 1], cost);
        }
    }
}

// the caller's cloud of a call (null xyz with resident: the context's source) and its detail outputs; on_device: device memory
struct VerifyIo {
    bool resident;
    const float *xyz; int64_t n, stride;
    uint8_t *mask; int32_t *nn;
    bool on_device;
};

struct VerifyLess {
    int rank_by;
    bool operator()(const dcreg_verify_record &a, const dcreg_verify_record &b) const {
        if (rank_by == 0) {
            if (a.count != b.count) return a.count > b.count;
            if (a.cost != b.cost) return a.cost < b.cost;
        } else {
            if (a.score != b.score) return a.score < b.score;
            if (a.count != b.count) return a.count > b.count;
        }
        return a.pose < b.pose;
    }
};

int verify_run(dcreg_ctx *c, const VerifyIo &io, const double *T, int64_t n_poses, int64_t pose_stride, const dcreg_verify_params *p,
               dcreg_verify_record *rec, dcreg_verify_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    // ---- every refusal of the header, before anything is queued or switched
    if (!p) { c->fail("null verify parameters"); return DCREG_E_INVALID; }
    if (!rec) { c->fail("null record buffer"); return DCREG_E_INVALID; }
    if (n_poses < 0 || n_poses > kVerifyMaxPoses) { c->fail("n_poses is %lld: 0 .. %lld expected (grid.y limit)", (long long)n_poses, (long long)kVerifyMaxPoses); return DCREG_E_INVALID; }
    if (n_poses > 0 && !T) { c->fail("null pose buffer"); return DCREG_E_INVALID; }
    if (pose_stride < 16) { c->fail("pose_stride_doubles is %lld: at least 16 expected", (long long)pose_stride); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->inlier_distance) && p->inlier_distance > 0.0)) { c->fail("inlier_distance is %g: finite and > 0 expected", p->inlier_distance); return DCREG_E_INVALID; }
    if (p->point_stride < 1) { c->fail("point_stride is %lld: at least 1 expected", (long long)p->point_stride); return DCREG_E_INVALID; }
    if (p->rank_by != 0 && p->rank_by != 1) { c->fail("rank_by is %d: 0 or 1 expected", p->rank_by); return DCREG_E_INVALID; }
    if (p->detail_pose < -1 || (int64_t)p->detail_pose >= n_poses) { c->fail("detail_pose is %d: -1 .. %lld expected", p->detail_pose, (long long)n_poses - 1); return DCREG_E_INVALID; }
    if (!io.resident) {
        if (io.stride < 3 || io.n < 0) { c->fail("invalid cloud arguments"); return DCREG_E_INVALID; }
        if (io.n > (int64_t)INT32_MAX) { c->fail("cloud too large (%lld points)", (long long)io.n); return DCREG_E_INVALID; }
        if (io.n > 0 && !io.xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    }
    for (int64_t k = 0; k < n_poses; ++k) {
        const double *Tk = T + k * pose_stride;
        if (!finite_n(Tk, 12)) { c->fail("pose %lld has a non-finite entry", (long long)k); return DCREG_E_INVALID; }
        if (!rigid_rotation(Tk)) { c->fail("the rotation block of pose %lld is not a rotation (|R^T R - I| > 1e-6 or det <= 0)", (long long)k); return DCREG_E_INVALID; }
    }
    dcreg_verify_info I;
    std::memset(&I, 0, sizeof(I));
    if (n_poses == 0) { if (info) *info = I; return DCREG_OK; }
    // (a context with a map has points in its active index, whichever of the two that is: asked before the switch, so that a refused
    // call has changed nothing)
    if (c->map.n <= 0) { c->fail("no map: dcreg_set_target first"); return DCREG_E_STATE; }
    if (io.resident && c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    (void)roi_deactivate(c);             // the poses are scored on the whole map (context.hpp, the window index)
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::VerifyBufs &V = c->verify;
    const int64_t n = io.resident ? c->n_src : io.n, s = p->point_stride;
    const size_t np = (size_t)n_poses;
    const bool detail = p->detail_pose >= 0 && (io.mask || io.nn) && n > 0;
    // ---- the selected points
    const float4 *pts = nullptr;
    int64_t n_sel = 0;
    if (io.resident) {
        n_sel = (n + s - 1) / s;
        if (s == 1) pts = c->d_src.data();
        else {
            const size_t n1 = (size_t)n + 1;
            if (V.flag.ensure(c, n1) || V.pos.ensure(c, n1) || V.sel.ensure(c, (size_t)n_sel)) return DCREG_E_NOMEM;
            hipLaunchKernelGGL(k_verify_flag_src, dim3(blocks((int64_t)n1, 256)), dim3(256), 0, c->stream, c->d_src.data(), n, (uint32_t)std::min<int64_t>(s, 0xFFFFFFFFll),
                               V.flag.data());
            if (int rc = scan_u32(c, V.flag.data(), V.pos.data(), n1, false)) return rc;
            hipLaunchKernelGGL(k_verify_gather_src, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->d_src.data(), n, V.flag.data(), V.pos.data(), V.sel.data());
            HIP_TRY(c, hipGetLastError());
            pts = V.sel.data();
        }
    } else if (n > 0) {
        const float *rows = nullptr;
        if (int rc = caller_rows<float>(c, io.xyz, n, io.stride, 3, io.on_device, V.rows, &rows)) return rc;
        const size_t n1 = (size_t)n + 1;
        if (V.flag.ensure(c, n1) || V.pos.ensure(c, n1) || V.sel.ensure(c, (size_t)((n + s - 1) / s))) return DCREG_E_NOMEM;
        hipLaunchKernelGGL(k_verify_flag_rows, dim3(blocks((int64_t)n1, 256)), dim3(256), 0, c->stream, rows, n, io.stride, s, V.flag.data());
        if (int rc = scan_u32(c, V.flag.data(), V.pos.data(), n1, false)) return rc;
        hipLaunchKernelGGL(k_verify_gather_rows, dim3(blocks(n, 256)), dim3(256), 0, c->stream, rows, n, io.stride, V.flag.data(), V.pos.data(), V.sel.data());
        HIP_TRY(c, hipGetLastError());
        uint32_t n_used = 0;
        HIP_TRY(c, hipMemcpyAsync(&n_used, V.pos.data() + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        n_sel = (int64_t)n_used;
        pts = V.sel.data();
    }
    // ---- the pose table, the sums, the detail arrays
    std::vector<double> table(12 * np);
    for (size_t k = 0; k < np; ++k) {
        const double *Tk = T + (int64_t)k * pose_stride;
        double *o = table.data() + 12 * k;
        for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) o[3 * r + q] = Tk[4 * r + q]; o[9 + r] = Tk[4 * r + 3]; }
    }
    std::vector<unsigned long long> sums(2 * np, 0ull);
    if (V.poses.ensure(c, table.size()) || V.acc.ensure(c, sums.size())) return DCREG_E_NOMEM;
    if (detail && ((io.mask && V.mask.ensure(c, (size_t)n)) || (io.nn && V.nn.ensure(c, (size_t)n)))) return DCREG_E_NOMEM;
    if (n_sel > 0) {
        const GridDev &g = c->map.grid;
        const OneNnBound b = one_nn_bound(g, p->inlier_distance);
        VerifyArgs a;
        a.dd = b.radius_sq; a.bound_f = b.bound_f; a.max_ring = b.max_ring;
        HIP_TRY(c, hipMemcpyAsync(V.poses.data(), table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(V.acc.data(), 0, sizeof(unsigned long long) * sums.size(), c->stream));
        if (detail && io.mask) HIP_TRY(c, hipMemsetAsync(V.mask.data(), 0, (size_t)n, c->stream));
        if (detail && io.nn) HIP_TRY(c, hipMemsetAsync(V.nn.data(), 0xFF, sizeof(int32_t) * (size_t)n, c->stream));
        const int64_t per = c->opt_verify_poses_per_launch > 0 ? c->opt_verify_poses_per_launch : n_poses;
        const unsigned nbx = blocks(n_sel, kLinBlock);
        for (int64_t k0 = 0; k0 < n_poses; k0 += per) {
            const int64_t nk = std::min(per, n_poses - k0);
            const bool here = detail && p->detail_pose >= k0 && p->detail_pose < k0 + nk;
            hipLaunchKernelGGL(here ? k_verify<true> : k_verify<false>, dim3(nbx, (unsigned)nk), dim3(kLinBlock), 0, c->stream, pts, (uint32_t)n_sel, g,
                               V.poses.data() + 12 * k0, a, V.acc.data() + 2 * k0, here ? (uint32_t)(p->detail_pose - k0) : kNoIdx,
                               io.mask ? V.mask.data() : nullptr, io.nn ? V.nn.data() : nullptr);
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipMemcpyAsync(sums.data(), V.acc.data(), sizeof(unsigned long long) * sums.size(), hipMemcpyDeviceToHost, c->stream));
        if (detail && io.mask) if (int rc = caller_out(c, io.mask, V.mask.data(), (size_t)n, io.on_device)) return rc;
        if (detail && io.nn) if (int rc = caller_out(c, io.nn, V.nn.data(), sizeof(int32_t) * (size_t)n, io.on_device)) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    } else if (detail) {                                                 // rows, none of them scored: an all-zero mask, nn all -1
        if (io.on_device) {
            if (io.mask) HIP_TRY(c, hipMemsetAsync(io.mask, 0, (size_t)n, c->stream));
            if (io.nn) HIP_TRY(c, hipMemsetAsync(io.nn, 0xFF, sizeof(int32_t) * (size_t)n, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        } else {
            if (io.mask) std::memset(io.mask, 0, (size_t)n);
            if (io.nn) std::memset(io.nn, 0xFF, sizeof(int32_t) * (size_t)n);
        }
    }
    // ---- the records (steps 5 to 7 of the rule)
    const double dd = p->inlier_distance * p->inlier_distance;
    for (size_t k = 0; k < np; ++k) {
        dcreg_verify_record &r = rec[k];
        std::memset(&r, 0, sizeof(r));
        const unsigned long long cnt = sums[2 * k], cost = sums[2 * k + 1];
        r.pose = (int32_t)k; r.count = (int32_t)cnt; r.cost = cost;
        r.score = cost + ((unsigned long long)n_sel - cnt) * 1048576ull;
        r.fitness = n_sel > 0 ? (double)cnt / (double)n_sel : 0.0;
        r.rmse = cnt ? std::sqrt((((double)cost / 1048576.0) * dd) / (double)cnt) : 0.0;
    }
    std::sort(rec, rec + np, VerifyLess{p->rank_by});
    I.n_poses = n_poses; I.n_points = n; I.n_scored = n_sel; I.best_pose = rec[0].pose;
    if (info) *info = I;
    return DCREG_OK;
}

}  // namespace
}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_default_verify_params(dcreg_verify_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->inlier_distance = 0.5; p->point_stride = 1; p->rank_by = 0; p->detail_pose = -1;
    return DCREG_OK;
}
int dcreg_verify_poses(dcreg_ctx *c, const double *T, int64_t n_poses, int64_t pose_stride_doubles, const dcreg_verify_params *p,
                       dcreg_verify_record *records_out, uint8_t *mask_out, int32_t *nn_out, dcreg_verify_info *info) {
    return verify_run(c, VerifyIo{true, nullptr, 0, 3, mask_out, nn_out, false}, T, n_poses, pose_stride_doubles, p, records_out, info);
}
int dcreg_verify_poses_cloud(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride_floats, const double *T, int64_t n_poses,
                             int64_t pose_stride_doubles, const dcreg_verify_params *p, dcreg_verify_record *records_out, uint8_t *mask_out,
                             int32_t *nn_out, dcreg_verify_info *info) {
    return verify_run(c, VerifyIo{false, xyz, n, stride_floats, mask_out, nn_out, false}, T, n_poses, pose_stride_doubles, p, records_out, info);
}
int dcreg_verify_poses_cloud_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride_floats, const double *T, int64_t n_poses,
                                    int64_t pose_stride_doubles, const dcreg_verify_params *p, dcreg_verify_record *records_out,
                                    uint8_t *d_mask_out, int32_t *d_nn_out, dcreg_verify_info *info) {
    return verify_run(c, VerifyIo{false, d_xyz, n, stride_floats, d_mask_out, d_nn_out, true}, T, n_poses, pose_stride_doubles, p, records_out, info);
}
}
