// A pose from correspondences by seeded RANSAC on the device (include/dcreg.h: dcreg_align_correspondences*): the stage behind
// dcreg_feature_match.  The rule of the header, bitwise the numpy reference of tests/align_ref.py with no stated freedom.
//   k_align_valid       one lane per correspondence m: both indices in range and the six coordinates finite
//   k_align_gather      behind an exclusive scan of the flags: the used pairs compacted in ascending m into [u] -> (p, q), six floats, and
//                       their correspondence numbers m - the scorer streams the array coalesced and never gathers
//   k_align_hypotheses  one lane per hypothesis h, a fixed grid striding over H: draws, pre-rejection and the triad test (align.hpp).
//                       Survivors are appended to the key list with a wave ballot and one atomic per wave, in no particular order - h
//                       is part of the ranking key.  ONLY h is stored: the pose is a few dozen operations from three gathered pairs,
//                       which the scorer pays once per survivor against its 30 operations for each of the M_u pairs, and 12 doubles
//                       per survivor would be 1.6 GB at H = 2^24 without pre-rejection
//   k_align_score       k_match's shape (features.hip): one survivor per lane, its R and t in registers; the used pairs go through LDS in
//                       tiles of kScoreTile pairs widened to double once, every lane reading the same row (a broadcast); blockIdx.y
//                       takes a range of pairs ("split") when survivors are few; count and cost are integers, so the splits add them
//                       with atomics in any order
//   (selection)         rocprim::merge_sort over the 16-byte keys with the total order (count descending, cost ascending, h ascending);
//                       the first T keys go to the host, which computes their records (host/align_host.cpp)
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge_sort.hpp>

#include "align.hpp"
#include "context.hpp"

// every multiply and add below rounds once: the rule is stated operation by operation
#pragma clang fp contract(off)

namespace dcreg {
namespace {

constexpr int64_t kMaxHypotheses = (int64_t)1 << 24;
constexpr int kMaxBest = 32, kMaxRefine = 8;
constexpr int kHypBlock = 256, kHypGrid = 4096;          // k_align_hypotheses: 2^20 hypotheses per stride of the grid
constexpr int kScoreBlock = 256, kScoreTile = 256;       // survivors per block, pairs per LDS tile (12 KiB of doubles)

DCREG_DEVFN bool finitef(float x) { return fabsf(x) <= 3.4028235e38f; }

// flag[m] = correspondence m is used; flag[n_pairs] = 0 (the scan's total lands behind it)
static __global__ void k_align_valid(const float *__restrict__ a, int64_t n_a, int64_t stride_a, const float *__restrict__ b, int64_t n_b,
                                     int64_t stride_b, const int32_t *__restrict__ ca, const int32_t *__restrict__ cb, int64_t n_pairs,
                                     uint32_t *__restrict__ flag) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m > n_pairs) return;
    bool ok = false;
    if (m < n_pairs) {
        const int64_t i = ca[m], j = cb[m];
        if (i >= 0 && i < n_a && j >= 0 && j < n_b) {
            const float *p = a + (size_t)i * (size_t)stride_a, *q = b + (size_t)j * (size_t)stride_b;
            ok = finitef(p[0]) && finitef(p[1]) && finitef(p[2]) && finitef(q[0]) && finitef(q[1]) && finitef(q[2]);
        }
    }
    flag[m] = ok ? 1u : 0u;
}

// the used pair m goes to place pos[m]: six floats and its correspondence number
static __global__ void k_align_gather(const float *__restrict__ a, int64_t stride_a, const float *__restrict__ b, int64_t stride_b,
                                      const int32_t *__restrict__ ca, const int32_t *__restrict__ cb, int64_t n_pairs,
                                      const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, float *__restrict__ P,
                                      int32_t *__restrict__ m_of_u) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_pairs || !flag[m]) return;
    const float *p = a + (size_t)ca[m] * (size_t)stride_a, *q = b + (size_t)cb[m] * (size_t)stride_b;
    const size_t u = pos[m];
    float *o = P + kAlignPairFloats * u;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = q[0]; o[4] = q[1]; o[5] = q[2];
    m_of_u[u] = (int32_t)m;
}

// Every lane walks h = its place in the grid, + the grid's size, ...; the trip count is the same for the whole block, so every ballot
// sees a full wave.  cnt[0] += survivors (the list's length), cnt[1] += degenerate, cnt[2] += rejected hypotheses
static __global__ __launch_bounds__(kHypBlock) void k_align_hypotheses(const float *__restrict__ P, uint32_t m_u, int64_t H, uint64_t seed, double s,
                                                                       AlignKey *__restrict__ keys, unsigned long long *__restrict__ cnt) {
    const int lane = threadIdx.x & (kWave - 1);
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long n_deg = 0, n_rej = 0;              // (the wave's, in every lane; its first lane adds them)
    for (int64_t base = (int64_t)blockIdx.x * kHypBlock; base < H; base += (int64_t)gridDim.x * kHypBlock) {
        const int64_t h = base + threadIdx.x;
        int st = -1;
        if (h < H) {
            uint32_t u[3];
            double R[9], t[3];
            st = align_hypothesis(P, m_u, seed, (uint64_t)h, s, u, R, t);
        }
        const unsigned long long S = __ballot(st == kAlignOk);
        n_deg += (unsigned long long)__popcll(__ballot(st == kAlignDegenerate));
        n_rej += (unsigned long long)__popcll(__ballot(st == kAlignRejected));
        if (S != 0ull) {
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(cnt, (unsigned long long)__popcll(S));
            at = __shfl(at, 0);
            if (st == kAlignOk) {
                AlignKey k;
                k.count = 0u; k.h = (uint32_t)h; k.cost = 0ull;
                keys[at + (unsigned long long)__popcll(S & below)] = k;
            }
        }
    }
    if (lane == 0) {
        if (n_deg) atomicAdd(cnt + 1, n_deg);
        if (n_rej) atomicAdd(cnt + 2, n_rej);
    }
}

// Block (x, y): the survivors [256 x, 256 x + 256) against the used pairs [chunk y, chunk y + chunk): count and cost of each, added to
// its key.  dd = d * d
static __global__ __launch_bounds__(kScoreBlock) void k_align_score(const float *__restrict__ P, uint32_t m_u, uint64_t seed, double dd, uint32_t n_surv,
                                                                    uint32_t chunk, AlignKey *__restrict__ keys) {
    __shared__ double tile[kScoreTile * kAlignPairFloats];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * kScoreBlock + tid;
    const bool live = i < n_surv;
    double R[9], t[3];
    {
        uint32_t u[3];
        (void)align_hypothesis(P, m_u, seed, (uint64_t)keys[live ? i : 0u].h, 0.0, u, R, t);      // (a survivor: kAlignOk)
    }
    const uint32_t u_begin = blockIdx.y * chunk, u_end = m_u - u_begin > chunk ? u_begin + chunk : m_u;      // (u_begin < m_u: the grid's y)
    uint32_t count = 0u;
    unsigned long long cost = 0ull;
    for (uint32_t t0 = u_begin; t0 < u_end; t0 += kScoreTile) {
        const uint32_t rows = min((uint32_t)kScoreTile, u_end - t0);
        __syncthreads();                                  // (the tile of the trip before is read no more)
        for (uint32_t e = tid; e < rows * kAlignPairFloats; e += kScoreBlock) tile[e] = (double)P[(size_t)t0 * kAlignPairFloats + e];
        __syncthreads();
        for (uint32_t r = 0; r < rows; ++r) {
            const double *row = tile + r * kAlignPairFloats;
            const double e2 = align_e2(R, t, row[0], row[1], row[2], row[3], row[4], row[5]);
            const bool in = e2 <= dd;
            count += in ? 1u : 0u;
            // (inliers are rare among wrong hypotheses: the division is skipped where no lane of the wave has one; a select, no branch per lane)
            if (__ballot(in) != 0ull) cost += (unsigned long long)floor(((in ? e2 : 0.0) / dd) * 1048576.0);
        }
    }
    if (live) {
        if (count) atomicAdd(&keys[i].count, count);
        if (cost) atomicAdd(&keys[i].cost, cost);
    }
}

struct AlignKeyLess {
    __host__ __device__ bool operator()(const AlignKey &a, const AlignKey &b) const {
        if (a.count != b.count) return a.count > b.count;
        if (a.cost != b.cost) return a.cost < b.cost;
        return a.h < b.h;
    }
};

int align_check(dcreg_ctx *c, const dcreg_align_params *p) {
    if (!p) { c->fail("null alignment parameters"); return DCREG_E_INVALID; }
    if (p->n_hypotheses < 1 || p->n_hypotheses > kMaxHypotheses) { c->fail("n_hypotheses is %lld: 1 .. 2^24 expected", (long long)p->n_hypotheses); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->inlier_distance) && p->inlier_distance > 0.0)) { c->fail("inlier_distance is %g: finite and > 0 expected", p->inlier_distance); return DCREG_E_INVALID; }
    if (!(p->edge_similarity >= 0.0 && p->edge_similarity < 1.0)) { c->fail("edge_similarity is %g: 0 <= s < 1 expected", p->edge_similarity); return DCREG_E_INVALID; }
    if (p->n_best < 1 || p->n_best > kMaxBest) { c->fail("n_best is %d: 1 .. %d expected", p->n_best, kMaxBest); return DCREG_E_INVALID; }
    if (p->refine_iterations < 0 || p->refine_iterations > kMaxRefine) { c->fail("refine_iterations is %d: 0 .. %d expected", p->refine_iterations, kMaxRefine); return DCREG_E_INVALID; }
    return DCREG_OK;
}

// the mask of a call without a record: all zero
int align_no_record(dcreg_ctx *c, uint8_t *mask, int64_t n_pairs, bool on_device) {
    if (!mask || n_pairs <= 0) return DCREG_OK;
    if (!on_device) { std::memset(mask, 0, (size_t)n_pairs); return DCREG_OK; }
    HIP_TRY(c, hipMemsetAsync(mask, 0, (size_t)n_pairs, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

int align_run(dcreg_ctx *c, const float *a, int64_t n_a, int64_t stride_a, const float *b, int64_t n_b, int64_t stride_b, const int32_t *ca,
              const int32_t *cb, int64_t n_pairs, bool on_device, const dcreg_align_params *p, dcreg_align_record *rec, uint8_t *mask,
              dcreg_align_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = align_check(c, p)) return rc;
    if (!rec) { c->fail("null record buffer"); return DCREG_E_INVALID; }
    if (n_a < 0 || n_b < 0 || n_pairs < 0 || stride_a < 3 || stride_b < 3) { c->fail("invalid alignment arguments"); return DCREG_E_INVALID; }
    if (n_a > (int64_t)INT32_MAX || n_b > (int64_t)INT32_MAX || n_pairs > (int64_t)INT32_MAX) { c->fail("too many points or pairs for one alignment call"); return DCREG_E_INVALID; }
    if ((n_a > 0 && !a) || (n_b > 0 && !b)) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    if (n_pairs > 0 && (!ca || !cb)) { c->fail("null correspondence buffer"); return DCREG_E_INVALID; }
    std::memset(rec, 0, sizeof(*rec) * (size_t)p->n_best);
    dcreg_align_info I;
    std::memset(&I, 0, sizeof(I));
    I.n_pairs = n_pairs;
    if (info) *info = I;
    if (n_pairs == 0) return DCREG_OK;
    dcreg_ctx::AlignBufs &A = c->algn;
    const size_t np = (size_t)n_pairs;
    // ---- the used pairs
    uint32_t m_u = 0;
    if (int rc = align_used_pairs(c, a, n_a, stride_a, b, n_b, stride_b, ca, cb, n_pairs, on_device, &m_u)) return rc;
    I.n_used = (int64_t)m_u;
    if (info) *info = I;
    if (m_u < 3u) return align_no_record(c, mask, n_pairs, on_device);
    // ---- the hypotheses
    const int64_t H = p->n_hypotheses;
    if (A.keys.ensure(c, (size_t)H) || A.sorted.ensure(c, (size_t)H)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(A.cnt.data(), 0, 3 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_align_hypotheses, dim3(std::min<unsigned>(blocks(H, kHypBlock), (unsigned)kHypGrid)), dim3(kHypBlock), 0, c->stream, A.P.data(), m_u, H,
                       (uint64_t)p->seed, p->edge_similarity, A.keys.data(), A.cnt.data());
    HIP_TRY(c, hipGetLastError());
    unsigned long long cnt[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(cnt, A.cnt.data(), sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    // (the host's share of the pairs travels while the hypotheses run)
    std::vector<float> hP(kAlignPairFloats * (size_t)m_u);
    std::vector<int32_t> hm((size_t)m_u);
    HIP_TRY(c, hipMemcpyAsync(hP.data(), A.P.data(), sizeof(float) * hP.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hm.data(), A.m_of_u.data(), sizeof(int32_t) * hm.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t n_surv = (int64_t)cnt[0];
    I.n_drawn = H; I.n_degenerate = (int64_t)cnt[1]; I.n_rejected = (int64_t)cnt[2]; I.n_scored = n_surv;
    if (info) *info = I;
    if (n_surv == 0) return align_no_record(c, mask, n_pairs, on_device);
    // ---- scores, ranks
    const int64_t blocks_x = (n_surv + kScoreBlock - 1) / kScoreBlock;
    int64_t chunk = c->opt_align_score_split;
    if (chunk <= 0) {                                       // about a thousand blocks, a split no shorter than a tile
        const int64_t want = std::max<int64_t>(1, 1024 / blocks_x), tiles = ((int64_t)m_u + kScoreTile - 1) / kScoreTile;
        chunk = (tiles + std::min(want, tiles) - 1) / std::min(want, tiles) * kScoreTile;
    }
    chunk = std::max<int64_t>(chunk, ((int64_t)m_u + 65534) / 65535);          // (blockIdx.y)
    const int64_t n_split = ((int64_t)m_u + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_align_score, dim3((unsigned)blocks_x, (unsigned)n_split), dim3(kScoreBlock), 0, c->stream, A.P.data(), m_u, (uint64_t)p->seed,
                       p->inlier_distance * p->inlier_distance, (uint32_t)n_surv, (uint32_t)chunk, A.keys.data());
    HIP_TRY(c, hipGetLastError());
    {
        size_t tmp = 0;
        HIP_TRY(c, rocprim::merge_sort(nullptr, tmp, A.keys.data(), A.sorted.data(), (size_t)n_surv, AlignKeyLess(), c->stream));
        if (c->sort_tmp.ensure(c, tmp) != DCREG_OK) return DCREG_E_NOMEM;
        HIP_TRY(c, rocprim::merge_sort(c->sort_tmp.data(), tmp, A.keys.data(), A.sorted.data(), (size_t)n_surv, AlignKeyLess(), c->stream));
    }
    const int n_rec = (int)std::min<int64_t>(p->n_best, n_surv);
    AlignKey best[kMaxBest];
    HIP_TRY(c, hipMemcpyAsync(best, A.sorted.data(), sizeof(AlignKey) * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    // ---- the records
    std::vector<uint8_t> hmask;
    if (mask && on_device) hmask.resize(np);
    align_host_records(hP.data(), hm.data(), (int64_t)m_u, n_pairs, p, best, n_rec, rec, mask ? (on_device ? hmask.data() : mask) : nullptr);
    if (mask && on_device) {
        HIP_TRY(c, hipMemcpyAsync(mask, hmask.data(), np, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    I.n_returned = n_rec;
    if (info) *info = I;
    return DCREG_OK;
}

}  // namespace

int align_used_pairs(dcreg_ctx *c, const float *a, int64_t n_a, int64_t stride_a, const float *b, int64_t n_b, int64_t stride_b, const int32_t *ca,
                     const int32_t *cb, int64_t n_pairs, bool on_device, uint32_t *m_u_out) {
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::AlignBufs &A = c->algn;
    const size_t np = (size_t)n_pairs;
    if (A.flag.ensure(c, np + 1) || A.pos.ensure(c, np + 1) || A.P.ensure(c, kAlignPairFloats * np) || A.m_of_u.ensure(c, np) || A.cnt.ensure(c, 3))
        return DCREG_E_NOMEM;
    const float *da = nullptr, *db = nullptr;
    const int32_t *dca = nullptr, *dcb = nullptr;
    if (int rc = caller_rows(c, a, n_a, stride_a, 3, on_device, A.a, &da)) return rc;
    if (int rc = caller_rows(c, b, n_b, stride_b, 3, on_device, A.b, &db, true)) return rc;
    if (int rc = caller_rows(c, ca, n_pairs, 1, 1, on_device, A.ca, &dca, true)) return rc;
    if (int rc = caller_rows(c, cb, n_pairs, 1, 1, on_device, A.cb, &dcb, true)) return rc;
    // ---- the used pairs
    hipLaunchKernelGGL(k_align_valid, dim3(blocks(n_pairs + 1, 256)), dim3(256), 0, c->stream, da, n_a, stride_a, db, n_b, stride_b, dca, dcb, n_pairs,
                       A.flag.data());
    if (int rc = scan_u32(c, A.flag.data(), A.pos.data(), np + 1, false)) return rc;
    hipLaunchKernelGGL(k_align_gather, dim3(blocks(n_pairs, 256)), dim3(256), 0, c->stream, da, stride_a, db, stride_b, dca, dcb, n_pairs, A.flag.data(),
                       A.pos.data(), A.P.data(), A.m_of_u.data());
    HIP_TRY(c, hipGetLastError());
    uint32_t m_u = 0;
    HIP_TRY(c, hipMemcpyAsync(&m_u, A.pos.data() + np, sizeof(m_u), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *m_u_out = m_u;
    return DCREG_OK;
}

}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_default_align_params(dcreg_align_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->n_hypotheses = 100000; p->seed = 0; p->inlier_distance = 0.5; p->edge_similarity = 0.9; p->n_best = 1; p->refine_iterations = 3;
    return DCREG_OK;
}
int dcreg_align_correspondences(dcreg_ctx *c, const float *a_xyz, int64_t n_a, int64_t stride_a, const float *b_xyz, int64_t n_b, int64_t stride_b,
                                const int32_t *corr_a, const int32_t *corr_b, int64_t n_pairs, const dcreg_align_params *p,
                                dcreg_align_record *records_out, uint8_t *inlier_mask_out, dcreg_align_info *info) {
    return align_run(c, a_xyz, n_a, stride_a, b_xyz, n_b, stride_b, corr_a, corr_b, n_pairs, false, p, records_out, inlier_mask_out, info);
}
int dcreg_align_correspondences_device(dcreg_ctx *c, const float *d_a_xyz, int64_t n_a, int64_t stride_a, const float *d_b_xyz, int64_t n_b,
                                       int64_t stride_b, const int32_t *d_corr_a, const int32_t *d_corr_b, int64_t n_pairs,
                                       const dcreg_align_params *p, dcreg_align_record *records_out, uint8_t *d_inlier_mask_out,
                                       dcreg_align_info *info) {
    return align_run(c, d_a_xyz, n_a, stride_a, d_b_xyz, n_b, stride_b, d_corr_a, d_corr_b, n_pairs, true, p, records_out, d_inlier_mask_out, info);
}
}
