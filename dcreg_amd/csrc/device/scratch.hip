// The cloud preparation every feature over a caller's cloud starts with, and the small launches they share (declared in one block of
// context.hpp).  The outlier filter, the normals (one cloud and many), both FPFH forms, the visibility filter, the 1-NN engines and the
// map updates all come through here:
//   k_cloud_used + scan + k_cloud_compact   the used (finite) points of a packed cloud, compacted with their input index in w
//                                           (cloud_used_compact), and build_index + build_gap_field over them (cloud_index_used), in the
//                                           context's CloudScratch
//   k_cloud_write                           the kept points of a cloud by keep flags and their scan: 3 floats or a packed float4 per point,
//                                           the byte mask (cloud_write_kept); cloud_filter_finish is the tail of a filter call around it
//   k_sorted_flags                          flags by input index read in an index's sorted order
//   scan_u32                                the one rocprim scan of the library: uint32 plus-scan on the context's stream
//   rings_for_bound                         the rings a grid walk needs to cover a ball
//   k_fill                                  a float array set to one value
// and the seam for caller memory: caller_order, caller_rows / caller_in, caller_out
#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "context.hpp"

namespace dcreg {
namespace {

// flag[i] = point i is used (n + 1 entries, the last 0)
static __global__ void k_cloud_used(const float4 *__restrict__ p, int64_t n, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    flag[i] = (i < n && finite_point(p[i])) ? 1u : 0u;
}
// the used points, in input order (w keeps the input index)
static __global__ void k_cloud_compact(const float4 *__restrict__ p, int64_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                       float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const float4 v = p[i];
    out[pos[i]] = make_float4(v.x, v.y, v.z, __uint_as_float((uint32_t)i));
}
static __global__ void k_fill(float *__restrict__ a, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}

static __global__ void k_cloud_write(const float4 *__restrict__ in, int64_t n, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos,
                                     float *__restrict__ out3, float4 *__restrict__ out4, uint8_t *__restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool k = keep[i] != 0u;
    if (mask) mask[i] = k ? 1 : 0;
    if (!k) return;
    const float4 v = in[i];
    const uint32_t j = pos[i];
    if (out4) out4[j] = make_float4(v.x, v.y, v.z, __uint_as_float(j));
    if (out3) { out3[3 * (int64_t)j] = v.x; out3[3 * (int64_t)j + 1] = v.y; out3[3 * (int64_t)j + 2] = v.z; }
}

static __global__ void k_sorted_flags(const float4 *__restrict__ sorted, int64_t n, const uint32_t *__restrict__ flag_r, uint32_t *__restrict__ flag_s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    flag_s[i] = i < n ? flag_r[__float_as_uint(sorted[i].w)] : 0u;
}

}  // namespace

int scan_u32(dcreg_ctx *c, const uint32_t *in, uint32_t *out, size_t n, bool inclusive) {
    size_t tmp = 0;
    if (inclusive) HIP_TRY(c, rocprim::inclusive_scan(nullptr, tmp, in, out, n, rocprim::plus<uint32_t>(), c->stream));
    else HIP_TRY(c, rocprim::exclusive_scan(nullptr, tmp, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    if (c->sort_tmp.ensure(c, tmp) != DCREG_OK) return DCREG_E_NOMEM;
    if (inclusive) HIP_TRY(c, rocprim::inclusive_scan(c->sort_tmp.data(), tmp, in, out, n, rocprim::plus<uint32_t>(), c->stream));
    else HIP_TRY(c, rocprim::exclusive_scan(c->sort_tmp.data(), tmp, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    return DCREG_OK;
}

int rings_for_bound(const GridDev &g, float bound) {
    int kk = 1;
    while (kk < 100000) { const double s = (double)kk * g.h * (1.0 - 1e-9); if (s * s * (1.0 - 1e-6) >= (double)bound) return kk; ++kk; }
    return -1;
}

SearchBound search_bound(double search_radius, const GridDev *g) {
    SearchBound s;
    if (search_radius > 0.0) {
        s.bound = (float)(search_radius * search_radius);
        if (!(s.bound <= 3.0e38f)) s.bound = 3.0e38f;
        if (g) s.max_ring = rings_for_bound(*g, s.bound);
    }
    return s;
}

// The caller most likely wrote its device memory on the legacy default stream (torch's default stream is that stream: cuda_stream == 0), and
// the context's own stream is non-blocking, so nothing orders it after that stream: make it wait for the work queued there so far.
// A context given the caller's stream (dcreg_set_stream) is ordered on that stream instead.
int caller_order(dcreg_ctx *c) {
    if (c->stream != c->own_stream) return DCREG_OK;
    if (!c->null_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->null_ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->null_ev, nullptr));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->null_ev, 0));
    return DCREG_OK;
}

int caller_in(dcreg_ctx *c, void *stage, const void *src, size_t bytes, bool on_device, bool ordered) {
    if (on_device) return ordered ? DCREG_OK : caller_order(c);
    if (bytes) HIP_TRY(c, hipMemcpyAsync(stage, src, bytes, hipMemcpyHostToDevice, c->stream));
    return DCREG_OK;
}

int caller_out(dcreg_ctx *c, void *dst, const void *src, size_t bytes, bool on_device) {
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    return DCREG_OK;
}

void fill_f32(dcreg_ctx *c, float *a, int64_t n, float v) {
    hipLaunchKernelGGL(k_fill, dim3(blocks(n, 256)), dim3(256), 0, c->stream, a, n, v);
}

int cloud_used_compact(dcreg_ctx *c, const float4 *in, int64_t n) {
    dcreg_ctx::CloudScratch &S = c->cloud;
    const size_t n1 = (size_t)n + 1;
    if (S.used.ensure(c, n1) || S.upos.ensure(c, n1) || S.cpts.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_cloud_used, dim3(blocks((int64_t)n1, 256)), dim3(256), 0, c->stream, in, n, S.used.data());
    if (int rc = scan_u32(c, S.used.data(), S.upos.data(), n1, false)) return rc;
    hipLaunchKernelGGL(k_cloud_compact, dim3(blocks(n, 256)), dim3(256), 0, c->stream, in, n, S.used.data(), S.upos.data(), S.cpts.data());
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

int cloud_index_used(dcreg_ctx *c, const float4 *in, int64_t n, double hint, int64_t min_used, int64_t *n_used_out) {
    dcreg_ctx::CloudScratch &S = c->cloud;
    if (int rc = cloud_used_compact(c, in, n)) return rc;
    uint32_t n_used = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_used, S.upos.data() + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    *n_used_out = n_used;
    if (n_used == 0 || (int64_t)n_used < min_used) return DCREG_OK;
    // (the build reports whether the table budget capped its cells: that word belongs to the target's builds)
    const bool capped = c->last_build_capped;
    int rc = build_index(c, S.cpts.data(), n_used, S.idx, hint, nullptr);
    if (rc == DCREG_OK) rc = build_gap_field(c, S.idx, hint);
    c->last_build_capped = capped;
    return rc;
}

int cloud_write_kept(dcreg_ctx *c, const float4 *in, int64_t n, const uint32_t *keep, const uint32_t *pos, float *out3, float4 *out4, uint8_t *mask) {
    if (n <= 0) return DCREG_OK;
    hipLaunchKernelGGL(k_cloud_write, dim3(blocks(n, 256)), dim3(256), 0, c->stream, in, n, keep, pos, out3, out4, mask);
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

int flags_to_sorted(dcreg_ctx *c, const float4 *sorted, int64_t n, const uint32_t *flag_r, uint32_t *flag_s) {
    hipLaunchKernelGGL(k_sorted_flags, dim3(blocks(n + 1, 256)), dim3(256), 0, c->stream, sorted, n, flag_r, flag_s);
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

int cloud_filter_finish(dcreg_ctx *c, const float4 *pts, int64_t n, const uint32_t *keep, uint32_t *pos, bool scan, int64_t n_out, int64_t capacity,
                        DevBuf<float> &out_buf, DevBuf<uint8_t> &mask_buf, float *out, uint8_t *mask, bool on_device) {
    if (n_out > capacity) { c->fail("the output holds %lld points, the capacity is %lld", (long long)n_out, (long long)capacity); return DCREG_E_INVALID; }
    if (n == 0) return DCREG_OK;
    if (out_buf.ensure(c, (size_t)(3 * std::max<int64_t>(n_out, 1))) || (mask && mask_buf.ensure(c, (size_t)n))) return DCREG_E_NOMEM;
    if (scan) if (int rc = scan_u32(c, keep, pos, (size_t)n + 1, false)) return rc;
    if (int rc = cloud_write_kept(c, pts, n, keep, pos, out_buf.data(), nullptr, mask ? mask_buf.data() : nullptr)) return rc;
    if (n_out > 0) if (int rc = caller_out(c, out, out_buf.data(), sizeof(float) * 3 * (size_t)n_out, on_device)) return rc;
    if (mask) if (int rc = caller_out(c, mask, mask_buf.data(), (size_t)n, on_device)) return rc;
    return DCREG_OK;
}

}  // namespace dcreg
