// Moving objects out of the map: visibility votes from keyframes (include/dcreg.h: dcreg_keyframes_range_images*, dcreg_visibility_filter*,
// dcreg_target_remove_dynamic).  A map point that the range images of other keyframes look THROUGH was not static.  The rule of the
// header, bitwise the numpy reference of tests/visibility_ref.py:
//   (memset)       the images of one batch of members, every pixel the bits of +inf
//   k_vis_image    the batch's stored points tiled as k_kf_gather tiles its output (a tile inside one member reads its record once, a tile
//                  across members finds every point's member by binary search); one no-return atomic minimum per used point on the bits of
//                  (float)r - in global memory: a 64 x 1024 image is 256 KB, four times what a block's LDS holds
//   k_vis_vote     one thread per point, a loop over the batch's members with pose and parameters in scalar registers; the range gate comes
//                  before any trigonometry; the two counts stay in registers and are added to the point's counters once per batch by the
//                  thread that owns the point (plain loads and stores, no atomics)
//   k_vis_keep     the decision per point, the call's counts (one atomic triple per wave); the callers scan and compact (scratch.hip)
// The counts are integers summed over the members, so neither the member order nor the batching ("visibility_max_bytes") can change a bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "context.hpp"

namespace dcreg {
namespace {

constexpr int kVisBlock = 256;
constexpr int kVisPerThread = 8;                         // stored points per thread of k_vis_image (a block covers one tile of 2048 points)
constexpr int kVisTile = kVisBlock * kVisPerThread;
constexpr int64_t kVisMaxBatchPoints = ((int64_t)1 << 31) - 1;   // stored points of one batch (VisMember::start is 32 bits wide)
constexpr uint32_t kInfBits = 0x7f800000u;
constexpr double kTwoPi = 6.283185307179586;

// the parameters as the kernels take them (by value: scalar registers)
struct VisDev {
    int rows, cols, window, min_votes;
    double elev_max, elev_span, min2, max2, margin_abs, margin_rel, min_ratio;
};

// The pixel of the sensor-frame point s (include/dcreg.h): false when the point is not used.  Every product and sum rounds once.
__device__ __forceinline__ bool vis_pixel(const VisDev &P, double sx, double sy, double sz, int &row, int &col, double &r) {
#pragma clang fp contract(off)
    const double rho2 = sx * sx + sy * sy;
    const double r2 = rho2 + sz * sz;
    if (!(r2 > 0.0 && r2 >= P.min2 && r2 < P.max2)) return false;           // (the range gate: before any trigonometry)
    r = sqrt(r2);
    const double el = atan2(sz, sqrt(rho2));
    const double a = (P.elev_max - el) * (double)P.rows / P.elev_span;
    if (!(a >= 0.0 && a < (double)P.rows)) return false;
    double az = atan2(sy, sx);
    if (az < 0.0) az += kTwoPi;
    const double b = az * (double)P.cols / kTwoPi;
    row = min((int)floor(a), P.rows - 1);                                    // (a < rows: the min only guards the cast)
    col = min((int)floor(b), P.cols - 1);
    return true;
}

// the member of the batch's stored point i: the largest m with mem[m].start <= i (the starts ascend strictly: no empty member is listed)
__device__ __forceinline__ int vis_member_of(const VisMember *__restrict__ mem, int n_members, uint32_t i) {
    int lo = 0, hi = n_members - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mem[mid].start <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void vis_splat(const VisDev &P, const float *__restrict__ p, uint32_t *__restrict__ image) {
    int row, col;
    double r;
    if (!vis_pixel(P, (double)p[0], (double)p[1], (double)p[2], row, col, r)) return;
    (void)atomicMin(image + (size_t)row * (size_t)P.cols + (size_t)col, __float_as_uint((float)r));      // (result unused: no return value travels back)
}

// The range images of one batch: n stored points in all, image m of the batch at images + m rows cols
static __global__ void __launch_bounds__(kVisBlock) k_vis_image(const float *__restrict__ store, const VisMember *__restrict__ mem, int n_members,
                                                                int64_t n, VisDev P, uint32_t *__restrict__ images) {
    const int64_t base = (int64_t)blockIdx.x * kVisTile;
    const int64_t last = std::min<int64_t>(n, base + kVisTile) - 1;
    const size_t px = (size_t)P.rows * (size_t)P.cols;
    const int m0 = vis_member_of(mem, n_members, (uint32_t)base);
    if (vis_member_of(mem, n_members, (uint32_t)last) == m0) {          // (block-uniform) the member's record once, then 12-byte records
        const float *__restrict__ src = store + 3 * ((int64_t)mem[m0].src + (base - (int64_t)mem[m0].start));
        uint32_t *__restrict__ image = images + px * (size_t)mem[m0].img;
        for (int k = 0; k < kVisPerThread; ++k) {
            const int64_t j = (int64_t)threadIdx.x + (int64_t)k * kVisBlock;
            if (base + j > last) break;
            vis_splat(P, src + 3 * j, image);
        }
        return;
    }
    for (int k = 0; k < kVisPerThread; ++k) {                            // a tile across members: every point finds its own
        const int64_t i = base + threadIdx.x + (int64_t)k * kVisBlock;
        if (i > last) break;
        const VisMember *__restrict__ M = mem + vis_member_of(mem, n_members, (uint32_t)i);
        vis_splat(P, store + 3 * ((int64_t)M->src + (i - (int64_t)M->start)), images + px * (size_t)M->img);
    }
}

// The votes of one batch's members on the n packed points at pts.  BY_W: point i counts at index w_i (a map in cell order: neighbouring
// lanes look at neighbouring pixels), otherwise at i.  A point with a non-finite coordinate fails the range gate of every member.
template <bool BY_W>
static __global__ void __launch_bounds__(kVisBlock) k_vis_vote(const float4 *__restrict__ pts, int64_t n, const VisMember *__restrict__ mem, int n_members,
                                                               VisDev P, const float *__restrict__ images, int32_t *__restrict__ through,
                                                               int32_t *__restrict__ observed) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kVisBlock + threadIdx.x;
    if (i >= n) return;
    const float4 q = pts[i];
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    const size_t px = (size_t)P.rows * (size_t)P.cols;
    int th = 0, ob = 0;
    for (int m = 0; m < n_members; ++m) {                                // (m is uniform: the record is read into scalar registers)
        const double *__restrict__ T = mem[m].pose;
        const double d0 = qx - T[9], d1 = qy - T[10], d2 = qz - T[11];
        const double sx = T[0] * d0 + T[3] * d1 + T[6] * d2;
        const double sy = T[1] * d0 + T[4] * d1 + T[7] * d2;
        const double sz = T[2] * d0 + T[5] * d1 + T[8] * d2;
        int row, col;
        double r;
        if (!vis_pixel(P, sx, sy, sz, row, col, r)) continue;
        const float *__restrict__ image = images + px * (size_t)mem[m].img;
        float best = __builtin_inff();
        const int r0 = max(row - P.window, 0), r1 = min(row + P.window, P.rows - 1);
        for (int rr = r0; rr <= r1; ++rr) {
            const float *__restrict__ line = image + (size_t)rr * (size_t)P.cols;
            for (int dc = -P.window; dc <= P.window; ++dc) {
                int cc = (col + dc) % P.cols;                            // (|dc| <= 3 may exceed cols: the remainder, then its sign)
                if (cc < 0) cc += P.cols;
                best = fminf(best, line[cc]);
            }
        }
        if (best == __builtin_inff()) continue;
        ob += 1;
        if ((double)best > r + (P.margin_abs + P.margin_rel * r)) th += 1;
    }
    const int64_t o = BY_W ? (int64_t)__float_as_uint(q.w) : i;
    through[o] += th;
    observed[o] += ob;
}

// keep[i] = point i stays (n + 1 entries, the last 0); cnt[0] += finite points, cnt[1] += observed ones, cnt[2] += removed ones
static __global__ void __launch_bounds__(kVisBlock) k_vis_keep(const float4 *__restrict__ pts, int64_t n, const int32_t *__restrict__ through,
                                                               const int32_t *__restrict__ observed, int min_votes, double min_ratio,
                                                               uint32_t *__restrict__ keep, unsigned long long *__restrict__ cnt) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kVisBlock + threadIdx.x;
    if (i > n) return;
    bool fin = false, obs = false, gone = false;
    if (i < n) {
        const float4 p = pts[i];
        fin = fabsf(p.x) <= 3.4028235e38f && fabsf(p.y) <= 3.4028235e38f && fabsf(p.z) <= 3.4028235e38f;   // (finite_point, written out: the call compiles to other code here)
        const int th = through[i], ob = observed[i];
        obs = fin && ob >= 1;
        gone = fin && th >= min_votes && (double)th >= min_ratio * (double)ob;
    }
    keep[i] = (fin && !gone) ? 1u : 0u;
    const unsigned long long A = __ballot(true), F = __ballot(fin), O = __ballot(obs), G = __ballot(gone);
    if ((int)(threadIdx.x & 63) == __ffsll(A) - 1) {
        if (F) atomicAdd(cnt, (unsigned long long)__popcll(F));
        if (O) atomicAdd(cnt + 1, (unsigned long long)__popcll(O));
        if (G) atomicAdd(cnt + 2, (unsigned long long)__popcll(G));
    }
}

int enter(dcreg_ctx *c) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return DCREG_OK;
}

int check_params(dcreg_ctx *c, const dcreg_visibility_params *p) {
    const double half_pi = 1.5707963267948966;
    if (!p) { c->fail("null visibility parameters"); return DCREG_E_INVALID; }
    if (p->rows < 1 || p->rows > 256 || p->cols < 1 || p->cols > 4096) {
        c->fail("visibility image is %d x %d: rows in [1, 256] and cols in [1, 4096] expected", p->rows, p->cols);
        return DCREG_E_INVALID;
    }
    if (!(std::isfinite(p->elev_min) && std::isfinite(p->elev_max) && p->elev_min < p->elev_max && p->elev_min >= -half_pi && p->elev_max <= half_pi)) {
        c->fail("visibility elevation span is [%g, %g]: elev_min < elev_max inside [-pi/2, pi/2] expected", p->elev_min, p->elev_max);
        return DCREG_E_INVALID;
    }
    if (!(std::isfinite(p->min_range) && std::isfinite(p->max_range) && p->min_range >= 0.0 && p->min_range < p->max_range)) {
        c->fail("visibility range is [%g, %g): 0 <= min_range < max_range, finite, expected", p->min_range, p->max_range);
        return DCREG_E_INVALID;
    }
    if (!(std::isfinite(p->margin_abs) && std::isfinite(p->margin_rel) && p->margin_abs >= 0.0 && p->margin_rel >= 0.0)) {
        c->fail("visibility margins are %g and %g: finite and >= 0 expected", p->margin_abs, p->margin_rel);
        return DCREG_E_INVALID;
    }
    if (p->window < 0 || p->window > 3) { c->fail("visibility window is %d: 0 .. 3 expected", p->window); return DCREG_E_INVALID; }
    if (p->min_votes < 1) { c->fail("visibility min_votes is %d: >= 1 expected", p->min_votes); return DCREG_E_INVALID; }
    if (!(p->min_ratio >= 0.0 && p->min_ratio <= 1.0)) { c->fail("visibility min_ratio is %g: 0 .. 1 expected", p->min_ratio); return DCREG_E_INVALID; }
    return DCREG_OK;
}

VisDev dev_params(const dcreg_visibility_params &p) {
#pragma clang fp contract(off)
    VisDev d;
    d.rows = p.rows; d.cols = p.cols; d.window = p.window; d.min_votes = p.min_votes;
    d.elev_max = p.elev_max; d.elev_span = p.elev_max - p.elev_min;
    d.min2 = p.min_range * p.min_range; d.max2 = p.max_range * p.max_range;
    d.margin_abs = p.margin_abs; d.margin_rel = p.margin_rel; d.min_ratio = p.min_ratio;
    return d;
}

// the images of batch b: memset, member records up, k_vis_image
int batch_images(dcreg_ctx *c, const VisRun &v, size_t b) {
    dcreg_ctx::VisibilityBufs &B = c->vis;
    const size_t px = (size_t)v.p.rows * (size_t)v.p.cols;
    const int64_t m0 = v.batch[b], nm = v.batch[b + 1] - m0;
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)B.images.data(), (int)kInfBits, px * (size_t)v.n_img[b], c->stream));
    if (nm == 0) return DCREG_OK;
    HIP_TRY(c, hipMemcpyAsync(B.members.data(), v.members.data() + m0, sizeof(VisMember) * (size_t)nm, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_vis_image, dim3(blocks(v.n_pts[b], kVisTile)), dim3(kVisBlock), 0, c->stream, c->kf.xyz.data(), B.members.data(), (int)nm,
                       v.n_pts[b], dev_params(v.p), reinterpret_cast<uint32_t *>(B.images.data()));
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

// the call's scratch that depends on the members alone: the largest batch's images and records
int reserve_batches(dcreg_ctx *c, const VisRun &v) {
    const size_t px = (size_t)v.p.rows * (size_t)v.p.cols;
    int64_t img = 0, rec = 0;
    for (size_t b = 0; b + 1 < v.batch.size(); ++b) { img = std::max(img, v.n_img[b]); rec = std::max(rec, v.batch[b + 1] - v.batch[b]); }
    if (c->vis.images.ensure(c, px * (size_t)std::max<int64_t>(img, 1)) || c->vis.members.ensure(c, (size_t)std::max<int64_t>(rec, 1))) return DCREG_E_NOMEM;
    return DCREG_OK;
}

int range_images(dcreg_ctx *c, int64_t n, const int64_t *ids, const dcreg_visibility_params *p, float *out, bool on_device) {
    if (int rc = enter(c)) return rc;
    VisRun v;
    if (int rc = visibility_prepare(c, n, ids, nullptr, p, v)) return rc;
    if (n > 0 && !out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (int rc = reserve_batches(c, v)) return rc;
    const size_t px = (size_t)v.p.rows * (size_t)v.p.cols;
    size_t done = 0;
    for (size_t b = 0; b + 1 < v.batch.size(); ++b) {
        if (int rc = batch_images(c, v, b)) return rc;
        if (int rc = caller_out(c, out + px * done, c->vis.images.data(), sizeof(float) * px * (size_t)v.n_img[b], on_device)) return rc;
        done += (size_t)v.n_img[b];
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

int filter_to(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, int64_t n_members, const int64_t *ids, const double *poses,
              const dcreg_visibility_params *p, float *out, int64_t capacity, int64_t *n_out, uint8_t *mask, int32_t *through, int32_t *observed,
              dcreg_visibility_info *info) {
    if (int rc = enter(c)) return rc;
    VisRun v;
    if (int rc = visibility_prepare(c, n_members, ids, poses, p, v)) return rc;
    if (n_members > 0 && !poses) { c->fail("null member poses"); return DCREG_E_INVALID; }
    if (n < 0 || stride < 3 || !n_out || capacity < 0) { c->fail("invalid visibility filter arguments"); return DCREG_E_INVALID; }
    if (n > (int64_t)INT32_MAX) { c->fail("too many points for one visibility pass (%lld)", (long long)n); return DCREG_E_INVALID; }
    if ((n > 0 && !xyz) || (capacity > 0 && !out)) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    dcreg_ctx::VisibilityBufs &B = c->vis;
    VisResult r;
    r.n_members = n_members;
    if (n > 0) {
        if (B.keep.ensure(c, (size_t)n + 1) || B.pos.ensure(c, (size_t)n + 1)) return DCREG_E_NOMEM;
        if (int rc = upload_cloud(c, xyz, n, stride, on_device, B.pts)) return rc;
        if (int rc = visibility_votes(c, B.pts.data(), n, false, v)) return rc;
        if (int rc = visibility_flags(c, B.pts.data(), n, v, B.keep.data(), r)) return rc;
    }
    *n_out = r.n_out;
    visibility_info(info, r);
    // (the flags' scan is queued just before the write)
    if (int rc = cloud_filter_finish(c, B.pts.data(), n, B.keep.data(), B.pos.data(), true, r.n_out, capacity, B.out, B.mask, out, mask, on_device)) return rc;
    if (n == 0) return DCREG_OK;
    if (through) if (int rc = caller_out(c, through, B.through.data(), sizeof(int32_t) * (size_t)n, on_device)) return rc;
    if (observed) if (int rc = caller_out(c, observed, B.observed.data(), sizeof(int32_t) * (size_t)n, on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

}  // namespace

int visibility_prepare(dcreg_ctx *c, int64_t n_members, const int64_t *ids, const double *poses, const dcreg_visibility_params *p, VisRun &v) {
    if (int rc = check_params(c, p)) return rc;
    if (!c->kf.ready) { c->fail("no keyframe store: dcreg_keyframes_reset first"); return DCREG_E_STATE; }
    if (n_members < 0 || n_members >= INT32_MAX) { c->fail("invalid member count (%lld)", (long long)n_members); return DCREG_E_INVALID; }
    if (n_members > 0 && !ids) { c->fail("null member ids"); return DCREG_E_INVALID; }
    const dcreg_ctx::KeyframeBufs &K = c->kf;
    const int64_t count = (int64_t)K.off.size() - 1;
    v = VisRun();
    v.p = *p;
    v.n_members = n_members;
    const double bytes = 4.0 * (double)p->rows * (double)p->cols;
    const int64_t per_batch = std::max<int64_t>(1, (int64_t)std::min(std::floor(c->opt_visibility_max_bytes / bytes), 1.0e9));
    try {
        v.batch.push_back(0);
        int64_t img = 0, pts = 0;
        for (int64_t m = 0; m < n_members; ++m) {
            const int64_t id = ids[m];
            if (id < 0 || id >= count) {
                c->fail("member %lld names keyframe %lld, the store holds [0, %lld)", (long long)m, (long long)id, (long long)count);
                return DCREG_E_INVALID;
            }
            if (poses)
                for (int e = 0; e < 12; ++e)
                    if (!std::isfinite(poses[12 * m + e])) { c->fail("the pose of member %lld has non-finite entries", (long long)m); return DCREG_E_INVALID; }
            const int64_t np = K.off[(size_t)id + 1] - K.off[(size_t)id];
            if (img == per_batch || pts + np > kVisMaxBatchPoints) {          // the batch is full: the next one starts here
                v.batch.push_back((int64_t)v.members.size()); v.n_img.push_back(img); v.n_pts.push_back(pts);
                img = 0; pts = 0;
            }
            if (np > 0) {
                VisMember r;
                r.start = (uint32_t)pts; r.src = (uint32_t)K.off[(size_t)id]; r.img = (uint32_t)img; r.pad_ = 0;
                if (poses) std::memcpy(r.pose, poses + 12 * m, sizeof(r.pose)); else std::memset(r.pose, 0, sizeof(r.pose));
                v.members.push_back(r);
                pts += np;
            }
            img += 1;
        }
        if (img > 0) { v.batch.push_back((int64_t)v.members.size()); v.n_img.push_back(img); v.n_pts.push_back(pts); }
    } catch (const std::bad_alloc &) {
        c->fail("out of host memory");
        return DCREG_E_NOMEM;
    }
    return DCREG_OK;
}

int visibility_votes(dcreg_ctx *c, const float4 *pts, int64_t n, bool by_w, const VisRun &v) {
    dcreg_ctx::VisibilityBufs &B = c->vis;
    if (n <= 0) return DCREG_OK;
    if (B.through.ensure(c, (size_t)n) || B.observed.ensure(c, (size_t)n) || B.cnt.ensure(c, 3)) return DCREG_E_NOMEM;
    if (int rc = reserve_batches(c, v)) return rc;
    HIP_TRY(c, hipMemsetAsync(B.through.data(), 0, sizeof(int32_t) * (size_t)n, c->stream));
    HIP_TRY(c, hipMemsetAsync(B.observed.data(), 0, sizeof(int32_t) * (size_t)n, c->stream));
    const VisDev P = dev_params(v.p);
    for (size_t b = 0; b + 1 < v.batch.size(); ++b) {          // (stream order keeps a batch's records and images until its votes are cast)
        const int64_t nm = v.batch[b + 1] - v.batch[b];
        if (nm == 0) continue;                                  // (empty keyframes only: no vote)
        if (int rc = batch_images(c, v, b)) return rc;
        if (by_w)
            hipLaunchKernelGGL(k_vis_vote<true>, dim3(blocks(n, kVisBlock)), dim3(kVisBlock), 0, c->stream, pts, n, B.members.data(), (int)nm, P,
                               B.images.data(), B.through.data(), B.observed.data());
        else
            hipLaunchKernelGGL(k_vis_vote<false>, dim3(blocks(n, kVisBlock)), dim3(kVisBlock), 0, c->stream, pts, n, B.members.data(), (int)nm, P,
                               B.images.data(), B.through.data(), B.observed.data());
        HIP_TRY(c, hipGetLastError());
    }
    return DCREG_OK;
}

int visibility_flags(dcreg_ctx *c, const float4 *pts, int64_t n, const VisRun &v, uint32_t *keep, VisResult &r) {
    dcreg_ctx::VisibilityBufs &B = c->vis;
    r = VisResult();
    r.n_in = n;
    r.n_members = v.n_members;
    if (n <= 0) return DCREG_OK;
    if (B.cnt.ensure(c, 3)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(B.cnt.data(), 0, 3 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_vis_keep, dim3(blocks(n + 1, kVisBlock)), dim3(kVisBlock), 0, c->stream, pts, n, B.through.data(), B.observed.data(), v.p.min_votes,
                       v.p.min_ratio, keep, B.cnt.data());
    HIP_TRY(c, hipGetLastError());
    unsigned long long cnt[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(cnt, B.cnt.data(), sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    r.n_finite = (int64_t)cnt[0]; r.n_observed = (int64_t)cnt[1]; r.n_flagged = (int64_t)cnt[2];
    r.n_out = r.n_finite - r.n_flagged;
    return DCREG_OK;
}

void visibility_info(dcreg_visibility_info *info, const VisResult &r) {
    if (!info) return;
    info->n_in = r.n_in; info->n_finite = r.n_finite; info->n_observed = r.n_observed; info->n_flagged = r.n_flagged; info->n_out = r.n_out;
    info->n_members = r.n_members;
}

}  // namespace dcreg

using namespace dcreg;

static_assert(sizeof(VisMember) == 112, "one member record is 112 B (include/dcreg.h states it)");

extern "C" {

int dcreg_default_visibility_params(dcreg_visibility_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->rows = 64; p->cols = 1024;
    p->elev_min = -0.39269908169872414; p->elev_max = 0.39269908169872414;      // -+ pi / 8
    p->min_range = 0.5; p->max_range = 80.0;
    p->margin_abs = 0.2; p->margin_rel = 0.01;
    p->window = 1; p->min_votes = 2; p->min_ratio = 0.0;
    return DCREG_OK;
}

int dcreg_keyframes_range_images(dcreg_ctx *c, int64_t n, const int64_t *ids, const dcreg_visibility_params *p, float *out) {
    return range_images(c, n, ids, p, out, false);
}
int dcreg_keyframes_range_images_device(dcreg_ctx *c, int64_t n, const int64_t *ids, const dcreg_visibility_params *p, float *d_out) {
    return range_images(c, n, ids, p, d_out, true);
}

int dcreg_visibility_filter(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride_floats, int64_t n_members, const int64_t *member_ids,
                            const double *member_poses, const dcreg_visibility_params *p, float *out_xyz, int64_t capacity_points, int64_t *n_out,
                            uint8_t *keep_mask, int32_t *through, int32_t *observed, dcreg_visibility_info *info) {
    return filter_to(c, xyz, n, stride_floats, false, n_members, member_ids, member_poses, p, out_xyz, capacity_points, n_out, keep_mask, through,
                     observed, info);
}
int dcreg_visibility_filter_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride_floats, int64_t n_members, const int64_t *member_ids,
                                   const double *member_poses, const dcreg_visibility_params *p, float *d_out_xyz, int64_t capacity_points,
                                   int64_t *n_out, uint8_t *d_keep_mask, int32_t *d_through, int32_t *d_observed, dcreg_visibility_info *info) {
    return filter_to(c, d_xyz, n, stride_floats, true, n_members, member_ids, member_poses, p, d_out_xyz, capacity_points, n_out, d_keep_mask,
                     d_through, d_observed, info);
}

}  // extern "C"
