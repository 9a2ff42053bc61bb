// Outlier removal on the device (include/dcreg.h: dcreg_outlier_filter*, dcreg_set_source_outliers*, dcreg_set_target_outliers*,
// dcreg_target_remove_outliers): PCL's StatisticalOutlierRemoval and RadiusOutlierRemoval with the rules of the header, bitwise the numpy
// reference of tests/outliers_ref.py.  One pass serves every entry point:
//   (cloud_index_used)   the used (finite) points, compacted with their input index in w, and the index over them: the shared first step
//                     of scratch.hip (the in-place map call skips this: the map is its own index)
//   k_out_score<K>    statistical: a lane searches the grid for the k nearest OTHER points of its own point (the ring walk of k_knn, the
//                     lane's own index never enters the heap), sums the k square roots in ascending order and writes ONE float
//   k_out_count       radius mode: the same walk with a counter in place of the heap; it stops at min_neighbors
//   k_out_tree        T(a): blocks of 512 aligned values reduced pairwise, level after level - the tree of the header whatever the grid
//   (readback)        mean, then the squared deviations through the same tree, the threshold on the host
//   k_out_keep + scan keep flags in input order and their positions; the callers compact
// A point's score depends on the cloud only: the index decides how fast the neighbours are found, never which.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include <hip/hip_runtime.h>

#include "context.hpp"

namespace dcreg {
namespace {

constexpr int kTreeBlock = 256;                          // threads of k_out_tree: a block reduces 2 x kTreeBlock aligned values
constexpr int kMaxK = 32;

// The k smallest d2 to points other than `self`, ascending, in the last k of K slots (the first K - k hold -1 and never move: one
// instantiation serves every k <= K, and the pruning distance is the k-th best, not the K-th).  Distances only: among equal d2 the rank by
// index decides which POINT is kept, never which VALUE, and the score reads values.  The interface of search.hpp's heaps.
template <int K_>
struct HeapStat {
    static constexpr int K = K_;
    static constexpr bool kDeferred = false;
    float d[K];
    uint32_t self;
    int k;
    uint32_t n_eval, n_shell;
    DCREG_DEVFN void init(float bound_f, float = 1.f, float = 0.f) {
#pragma unroll
        for (int i = 0; i < K; ++i) d[i] = i < K - k ? -1.f : bound_f;
        n_eval = 0; n_shell = 1;
    }
    DCREG_DEVFN void push(float d2, uint32_t idx, uint32_t, bool valid = true) {
        const float x = (valid && idx != self) ? d2 : __builtin_inff();
#pragma unroll
        for (int i = K - 1; i > 0; --i) d[i] = med3f(d[i - 1], d[i], x);
        d[0] = fminf(d[0], x);
    }
    DCREG_DEVFN float worst_d2() const { return d[K - 1]; }
};

// Radius mode: no heap - the other points with d2 < bound are counted, and once `need` of them are known the pruning distance drops to
// zero, which ends the walk
struct HeapCount {
    static constexpr bool kDeferred = false;
    float bound, walk;
    uint32_t self, cnt, need;
    uint32_t n_eval, n_shell;
    DCREG_DEVFN void init(float walk_f, float = 1.f, float = 0.f) { walk = walk_f; cnt = 0; n_eval = 0; n_shell = 1; }
    DCREG_DEVFN void push(float d2, uint32_t idx, uint32_t, bool valid = true) { cnt += (valid && idx != self && d2 < bound) ? 1u : 0u; }
    DCREG_DEVFN float worst_d2() const { return cnt >= need ? 0.f : walk; }
};

// Statistical mode: one lane per used point, in the index's cell order (the lanes of a wave search neighbouring cells); the point's input
// index is in w, and the score goes there.  cnt[0] += points that enter the statistics, cnt[1] += sparse points (one atomic pair per wave)
template <int K>
static __global__ __launch_bounds__(kBlock) void k_out_score(const float4 *__restrict__ q, uint32_t n, GridDev g, float bound_f, int max_ring, int k,
                                                             int bounded, float *__restrict__ score, unsigned long long *__restrict__ cnt) {
    __shared__ RunList runs[kBlock / kWave];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 s4 = q[i];
    HeapStat<K> hp;
    hp.self = __float_as_uint(s4.w);
    hp.k = k;
    knn_search<HeapStat<K>>(g, runs[threadIdx.x / kWave], s4.x, s4.y, s4.z, bound_f, max_ring, hp);
    const bool sparse = bounded && !(hp.d[K - 1] < bound_f);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j >= K - k) s += (double)sqrtf(hp.d[j]);
    const float m = (float)(s / (double)k);
    score[hp.self] = sparse ? __builtin_nanf("") : m;
    const unsigned long long A = __ballot(true), S = __ballot(sparse);
    if ((int)(threadIdx.x & 63) == __ffsll(A) - 1) {
        const unsigned long long ns = (unsigned long long)__popcll(S);
        atomicAdd(cnt, (unsigned long long)__popcll(A) - ns);
        if (ns) atomicAdd(cnt + 1, ns);
    }
}

// Radius mode: score = the count capped at min_neighbors, keep = the count reached it
static __global__ __launch_bounds__(kBlock) void k_out_count(const float4 *__restrict__ q, uint32_t n, GridDev g, float bound_f, float walk_f, int max_ring,
                                                             uint32_t need, float *__restrict__ score, uint32_t *__restrict__ keep) {
    __shared__ RunList runs[kBlock / kWave];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 s4 = q[i];
    HeapCount hp;
    hp.self = __float_as_uint(s4.w);
    hp.bound = bound_f;
    hp.need = need;
    knn_search<HeapCount>(g, runs[threadIdx.x / kWave], s4.x, s4.y, s4.z, walk_f, max_ring, hp);
    const uint32_t c = min(hp.cnt, need);
    score[hp.self] = (float)c;
    keep[hp.self] = c >= need ? 1u : 0u;
}

// One level of T(a): block b reduces the values [512 b, 512 b + 512) pairwise - a[2j] + a[2j+1], then neighbours of neighbours - and
// writes one value; positions beyond n read +0.0.  MODE 0: the values are the float scores widened to double, NaN (unused, sparse) as
// +0.0; 1: their squared deviations from `mean`; 2: the doubles of the level below.  No contraction: every add and multiply rounds once.
template <int MODE>
static __global__ __launch_bounds__(kTreeBlock) void k_out_tree(const void *__restrict__ in, int64_t n, double mean, double *__restrict__ out) {
#pragma clang fp contract(off)
    auto value = [&](int64_t i) -> double {
        if (i >= n) return 0.0;
        if (MODE == 2) return static_cast<const double *>(in)[i];
        const float f = static_cast<const float *>(in)[i];
        if (f != f) return 0.0;
        if (MODE == 0) return (double)f;
        const double d = (double)f - mean;
        return __dmul_rn(d, d);
    };
    const int64_t base = (int64_t)blockIdx.x * (2 * kTreeBlock) + 2 * (int64_t)threadIdx.x;
    double v = __dadd_rn(value(base), value(base + 1));
    for (int o = 1; o < 64; o <<= 1) v = __dadd_rn(v, __shfl_xor(v, o));
    __shared__ double sw[kTreeBlock / 64];
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        static_assert(kTreeBlock == 256, "four waves: two adds, then one");
        out[blockIdx.x] = __dadd_rn(__dadd_rn(sw[0], sw[1]), __dadd_rn(sw[2], sw[3]));
    }
}

// statistical keep flags (n + 1 entries, the last 0).  all: a cloud without statistics keeps every used point (used == null: every point)
static __global__ void k_out_keep(const float *__restrict__ score, int64_t n, double thr, int all, const uint32_t *__restrict__ used,
                                  uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    bool k = false;
    if (i < n) {
        if (all) k = !used || used[i] != 0u;
        else { const float f = score[i]; k = f == f && (double)f <= thr; }
    }
    keep[i] = k ? 1u : 0u;
}

// T over the n scores (MODE 0 / 1): queued; the sum lands in *d_sum (device)
int tree_sum(dcreg_ctx *c, int mode, const float *score, int64_t n, double mean, const double **d_sum) {
    dcreg_ctx::OutlierBufs &B = c->outl;
    int64_t m = (n + 2 * kTreeBlock - 1) / (2 * kTreeBlock);
    int side = 0;
    if (mode == 0) hipLaunchKernelGGL(k_out_tree<0>, dim3((unsigned)m), dim3(kTreeBlock), 0, c->stream, score, n, mean, B.part[side].data());
    else hipLaunchKernelGGL(k_out_tree<1>, dim3((unsigned)m), dim3(kTreeBlock), 0, c->stream, score, n, mean, B.part[side].data());
    while (m > 1) {
        const int64_t m2 = (m + 2 * kTreeBlock - 1) / (2 * kTreeBlock);
        hipLaunchKernelGGL(k_out_tree<2>, dim3((unsigned)m2), dim3(kTreeBlock), 0, c->stream, B.part[side].data(), m, 0.0, B.part[side ^ 1].data());
        side ^= 1;
        m = m2;
    }
    HIP_TRY(c, hipGetLastError());
    *d_sum = B.part[side].data();
    return DCREG_OK;
}

template <int K>
void launch_score(dcreg_ctx *c, const float4 *q, int64_t nq, const GridDev &g, float bound, int max_ring, int k, int bounded) {
    hipLaunchKernelGGL(k_out_score<K>, dim3(blocks(nq, kBlock)), dim3(kBlock), 0, c->stream, q, (uint32_t)nq, g, bound, max_ring, k, bounded,
                       c->outl.score.data(), c->outl.cnt.data());
}

}  // namespace

int outlier_check(dcreg_ctx *c, const dcreg_outlier_params *p) {
    if (!p) { c->fail("null outlier parameters"); return DCREG_E_INVALID; }
    if (p->mode == DCREG_OUTLIER_STATISTICAL) {
        if (p->k < 1 || p->k > kMaxK) { c->fail("outlier k is %d: 1 .. %d expected", p->k, kMaxK); return DCREG_E_INVALID; }
        if (!std::isfinite(p->std_mul)) { c->fail("outlier std_mul is not finite"); return DCREG_E_INVALID; }
        if (!(std::isfinite(p->search_radius) && p->search_radius >= 0.0)) { c->fail("outlier search_radius is %g: finite and >= 0 expected", p->search_radius); return DCREG_E_INVALID; }
    } else if (p->mode == DCREG_OUTLIER_RADIUS) {
        if (!(std::isfinite(p->radius) && p->radius > 0.0)) { c->fail("outlier radius is %g: finite and > 0 expected", p->radius); return DCREG_E_INVALID; }
        if (p->min_neighbors < 1) { c->fail("outlier min_neighbors is %d: >= 1 expected", p->min_neighbors); return DCREG_E_INVALID; }
    } else {
        c->fail("unknown outlier mode %d", p->mode);
        return DCREG_E_INVALID;
    }
    return DCREG_OK;
}

void outlier_info(dcreg_outlier_info *info, const OutlierResult &r) {
    if (!info) return;
    info->n_in = r.n_in; info->n_finite = r.n_finite; info->n_sparse = r.n_sparse; info->n_out = r.n_out;
    info->mean = r.mean; info->stddev = r.stddev; info->threshold = r.threshold;
}

int outlier_pass(dcreg_ctx *c, const float4 *in, int64_t n, const dcreg_outlier_params *p, const dcreg_ctx::IndexSet *map, OutlierResult &r) {
#pragma clang fp contract(off)
    if (int rc = outlier_check(c, p)) return rc;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    r = OutlierResult();
    r.n_in = n;
    r.mean = r.stddev = r.threshold = nan;
    if (n <= 0) return DCREG_OK;
    if (n > (int64_t)INT32_MAX) { c->fail("too many points for one outlier pass (%lld)", (long long)n); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::OutlierBufs &B = c->outl;
    const size_t n1 = (size_t)n + 1;
    const size_t parts = (size_t)((n + 2 * kTreeBlock - 1) / (2 * kTreeBlock));
    if (B.keep.ensure(c, n1) || B.pos.ensure(c, n1) || B.score.ensure(c, (size_t)n) || B.part[0].ensure(c, parts) || B.part[1].ensure(c, parts) ||
        B.cnt.ensure(c, 2))
        return DCREG_E_NOMEM;
    const bool stat = p->mode == DCREG_OUTLIER_STATISTICAL;
    const double hint = stat ? p->search_radius : p->radius;
    fill_f32(c, B.score.data(), n, __builtin_nanf(""));
    HIP_TRY(c, hipMemsetAsync(B.cnt.data(), 0, 2 * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(B.keep.data(), 0, n1 * sizeof(uint32_t), c->stream));
    // ---- the used points and their index
    const float4 *q;
    int64_t nq;
    GridDev g;
    const uint32_t *used = nullptr;
    if (map) {
        q = map->sorted.data(); nq = n; g = map->grid;
        r.n_finite = n;
    } else {
        // (unbounded statistics over at most k used points keep every one of them: no search, no index)
        int64_t n_used = 0;
        if (int rc = cloud_index_used(c, in, n, hint, (stat && p->search_radius == 0.0) ? (int64_t)p->k + 1 : 1, &n_used)) return rc;
        r.n_finite = n_used;
        used = c->cloud.used.data();
        if (n_used == 0) {                    // nothing to search: every score NaN, every flag 0
            HIP_TRY(c, hipMemsetAsync(B.pos.data(), 0, n1 * sizeof(uint32_t), c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return DCREG_OK;
        }
        q = c->cloud.idx.sorted.data(); nq = n_used; g = c->cloud.idx.grid;
    }
    // ---- scores, statistics, keep flags
    if (stat) {
        const int k = p->k;
        const bool bounded = p->search_radius > 0.0;
        if (!bounded && r.n_finite <= k) {    // no statistics: every used point is kept
            hipLaunchKernelGGL(k_out_keep, dim3(blocks((int64_t)n1, 256)), dim3(256), 0, c->stream, B.score.data(), n, 0.0, 1, used, B.keep.data());
        } else {
            const SearchBound s = search_bound(p->search_radius, &g);
            if (k <= 4) launch_score<4>(c, q, nq, g, s.bound, s.max_ring, k, bounded);
            else with_heap_k(k, [&](auto K) { launch_score<decltype(K)::value>(c, q, nq, g, s.bound, s.max_ring, k, bounded); });
            HIP_TRY(c, hipGetLastError());
            const double *d_sum = nullptr;
            if (int rc = tree_sum(c, 0, B.score.data(), n, 0.0, &d_sum)) return rc;
            unsigned long long cnt[2] = {0, 0};
            double sum = 0.0;
            HIP_TRY(c, hipMemcpyAsync(&sum, d_sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(cnt, B.cnt.data(), sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            const int64_t n_stat = (int64_t)cnt[0];
            r.n_sparse = (int64_t)cnt[1];
            if (n_stat > 0) {
                const double mean = sum / (double)n_stat;
                double var = 0.0;
                if (n_stat > 1) {
                    if (int rc = tree_sum(c, 1, B.score.data(), n, mean, &d_sum)) return rc;
                    double sq = 0.0;
                    HIP_TRY(c, hipMemcpyAsync(&sq, d_sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                    var = sq / (double)(n_stat - 1);
                }
                const double sd = std::sqrt(var);
                volatile double prod = p->std_mul * sd;      // (one rounded multiply, one rounded add)
                r.mean = mean; r.stddev = sd; r.threshold = mean + prod;
                hipLaunchKernelGGL(k_out_keep, dim3(blocks((int64_t)n1, 256)), dim3(256), 0, c->stream, B.score.data(), n, r.threshold, 0, (const uint32_t *)nullptr,
                                   B.keep.data());
            }
        }
    } else {
        const float bound = (float)(p->radius * p->radius);
        float walk = std::nextafterf(bound, INFINITY);
        if (!(walk <= 3.0e38f)) walk = 3.0e38f;
        const int max_ring = rings_for_bound(g, walk);
        hipLaunchKernelGGL(k_out_count, dim3(blocks(nq, kBlock)), dim3(kBlock), 0, c->stream, q, (uint32_t)nq, g, bound, walk, max_ring, (uint32_t)p->min_neighbors,
                           B.score.data(), B.keep.data());
    }
    if (int rc = scan_u32(c, B.keep.data(), B.pos.data(), n1, false)) return rc;
    uint32_t n_out = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_out, B.pos.data() + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    r.n_out = n_out;
    return DCREG_OK;
}

int outlier_write_packed(dcreg_ctx *c, const float4 *in, int64_t n, int64_t n_out) {
    dcreg_ctx::OutlierBufs &B = c->outl;
    if (B.out4.ensure(c, (size_t)std::max<int64_t>(n_out, 1))) return DCREG_E_NOMEM;
    return cloud_write_kept(c, in, n, B.keep.data(), B.pos.data(), nullptr, B.out4.data(), nullptr);
}

// dcreg_outlier_filter*: the pass, then - when the caller's capacity holds the output - the copies to the caller
static int outlier_filter_to(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, const dcreg_outlier_params *p, float *out,
                             int64_t capacity, int64_t *n_out, uint8_t *mask, float *scores, dcreg_outlier_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = outlier_check(c, p)) return rc;
    if (n < 0 || stride < 3 || !n_out || capacity < 0) { c->fail("invalid outlier filter arguments"); return DCREG_E_INVALID; }
    if (n > (int64_t)INT32_MAX) { c->fail("too many points for one outlier pass (%lld)", (long long)n); return DCREG_E_INVALID; }
    if ((n > 0 && !xyz) || (capacity > 0 && !out)) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    OutlierResult r;
    dcreg_ctx::OutlierBufs &B = c->outl;
    DevBuf<float4> &pts = c->cloud.pts;
    if (n > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (int rc = upload_cloud(c, xyz, n, stride, on_device, pts)) return rc;
    }
    if (int rc = outlier_pass(c, pts.data(), n, p, nullptr, r)) return rc;
    *n_out = r.n_out;
    outlier_info(info, r);
    if (int rc = cloud_filter_finish(c, pts.data(), n, B.keep.data(), B.pos.data(), false, r.n_out, capacity, B.out, B.mask, out, mask, on_device)) return rc;
    if (n == 0) return DCREG_OK;
    if (scores) if (int rc = caller_out(c, scores, B.score.data(), sizeof(float) * (size_t)n, on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_default_outlier_params(dcreg_outlier_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->mode = DCREG_OUTLIER_STATISTICAL; p->k = 8; p->std_mul = 2.0; p->search_radius = 0.0; p->radius = 0.5; p->min_neighbors = 3;
    return DCREG_OK;
}
int dcreg_outlier_filter(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_outlier_params *p, float *out_xyz,
                         int64_t capacity_points, int64_t *n_out, uint8_t *keep_mask, float *scores, dcreg_outlier_info *info) {
    return outlier_filter_to(c, xyz, n, stride_floats, false, p, out_xyz, capacity_points, n_out, keep_mask, scores, info);
}
int dcreg_outlier_filter_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_outlier_params *p, float *d_out_xyz,
                                int64_t capacity_points, int64_t *n_out, uint8_t *d_keep_mask, float *d_scores, dcreg_outlier_info *info) {
    return outlier_filter_to(c, d_xyz, n, stride_floats, true, p, d_out_xyz, capacity_points, n_out, d_keep_mask, d_scores, info);
}
}
