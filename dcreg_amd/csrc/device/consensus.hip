// A consensus pose from the compatibility graph of the correspondences (include/dcreg.h: dcreg_consensus_correspondences*): the stage
// behind dcreg_feature_match for inlier shares the three-pair sampler of align.hip does not survive.  The rule of the header, bitwise the
// numpy reference of tests/consensus_ref.py: every quantity of the graph is a bit or an integer, the poses come from the host's fit.
//   (used pairs)        align.hip's step 1 as it is: k_align_valid, the scan, k_align_gather (align_used_pairs)
//   k_cons_adjacency    the graph as a bit matrix of 64-bit words, word-major (adj[word * M_u + u]): a lane per row u holds its p, q and
//                       index pair, a tile of 64 column pairs goes through LDS widened to double once, the lane builds the tile's word in
//                       a register out of selects and stores its 8 bytes next to its neighbours'.  No atomics; the bits past M_u stay zero
//   k_cons_weights      deg(u) and w(u) = sum of S(u, v) over the set bits of row u, a wave per row.  The row's words sit in LDS; the
//                       wave walks them, skips the empty ones, and in a word with set bits the lane of bit v sums popcount(row u & row v)
//                       over the words - row v's words of 64 neighbouring lanes are 512 consecutive bytes in the word-major layout.  One
//                       wave reduction per row.  This is the one kernel whose cost follows the graph: (non-empty words of the rows) x
//                       M_u / 64 steps, M_u^3 / 64^2 wave steps when every pair is compatible
//   (seeds)             rocprim::radix_sort_keys over (~w << 32 | u): w descending, u ascending
//   k_cons_members      a block per seed: its row of S again (uint16 per column, never the whole of S), S_max, then the members by
//                       repeated block-wide maxima of the key (S << 15 | 32767 - v) below the one taken before - (S descending, v
//                       ascending) -, written in ascending u
//   (poses)             the host fits every set with three members or more (host/align_host.cpp, OpenMP over the seeds): 12 doubles each
//   k_cons_score        k_align_score's shape: a lane per set, its pose from memory, the used pairs through LDS in the same tiles
//   (rank, records)     at most 1024 keys: sorted on the host, which refines and returns the first n_best (host/align_host.cpp)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "align.hpp"
#include "context.hpp"

// every multiply and add below rounds once: the rule is stated operation by operation
#pragma clang fp contract(off)

namespace dcreg {
namespace {

constexpr int64_t kMaxPairs = DCREG_CONSENSUS_MAX_PAIRS;
constexpr int kMaxBest = 32, kMaxRefine = 8;
constexpr int kBlock = 256;                              // every kernel here
constexpr int kAdjWords = 4;                             // k_cons_adjacency: words (tiles of 64 columns) per block
constexpr int kRowsPerBlock = kBlock / kWave;            // k_cons_weights: a wave per row
constexpr int kMaxWords = (int)(kMaxPairs / 64);         // 512 words in a row at the cap
constexpr int kScoreTile = 256;                          // k_cons_score: pairs per LDS tile (12 KiB of doubles), as k_align_score

// Block (x, y): rows [256 x, 256 x + 256) against the columns of words [4 y, 4 y + 4)
static __global__ __launch_bounds__(kBlock) void k_cons_adjacency(const float *__restrict__ P, const int32_t *__restrict__ m_of_u,
                                                                  const int32_t *__restrict__ ca, const int32_t *__restrict__ cb, uint32_t m_u,
                                                                  uint32_t n_words, double min_length, double compat,
                                                                  unsigned long long *__restrict__ adj) {
    __shared__ double tile[kWave * kAlignPairFloats];
    __shared__ int32_t tia[kWave], tib[kWave];
    const uint32_t tid = threadIdx.x, u = blockIdx.x * kBlock + tid;
    const bool live = u < m_u;
    const uint32_t ul = live ? u : 0u;
    double p[3], q[3];
    for (int c = 0; c < 3; ++c) { p[c] = (double)P[(size_t)kAlignPairFloats * ul + c]; q[c] = (double)P[(size_t)kAlignPairFloats * ul + 3 + c]; }
    const int32_t m = m_of_u[ul], ia = ca[m], ib = cb[m];
    const uint32_t w_begin = blockIdx.y * kAdjWords, w_end = min(w_begin + (uint32_t)kAdjWords, n_words);
    for (uint32_t word = w_begin; word < w_end; ++word) {
        const uint32_t v0 = word * kWave, cols = min((uint32_t)kWave, m_u - v0);         // (v0 < m_u: word < n_words)
        __syncthreads();                                  // (the tile of the trip before is read no more)
        for (uint32_t e = tid; e < cols * kAlignPairFloats; e += kBlock) tile[e] = (double)P[(size_t)v0 * kAlignPairFloats + e];
        if (tid < cols) { const int32_t mv = m_of_u[v0 + tid]; tia[tid] = ca[mv]; tib[tid] = cb[mv]; }
        __syncthreads();
        unsigned long long bits = 0ull;
        for (uint32_t j = 0; j < cols; ++j) {
            const double *r = tile + j * kAlignPairFloats;
            const double gx = p[0] - r[0], gy = p[1] - r[1], gz = p[2] - r[2];
            const double hx = q[0] - r[3], hy = q[1] - r[4], hz = q[2] - r[5];
            const double la = sqrt((gx * gx + gy * gy) + gz * gz), lb = sqrt((hx * hx + hy * hy) + hz * hz);
            // (u == v: the index tests fail, C(u, u) = 0)
            const bool c = (ia != tia[j]) & (ib != tib[j]) & (la >= min_length) & (lb >= min_length) & (fabs(la - lb) <= compat);
            bits |= (unsigned long long)(c ? 1u : 0u) << j;
        }
        if (live) adj[(size_t)word * m_u + u] = bits;
    }
}

// Wave w of block x: row u = 4 x + w.  deg[u], w[u] and the seeds' sort key of u
static __global__ __launch_bounds__(kBlock) void k_cons_weights(const unsigned long long *__restrict__ adj, uint32_t m_u, uint32_t n_words,
                                                                uint32_t *__restrict__ deg, uint32_t *__restrict__ w,
                                                                unsigned long long *__restrict__ key) {
    __shared__ unsigned long long rows[kRowsPerBlock][kMaxWords];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, u = blockIdx.x * kRowsPerBlock + wave;
    const bool live = u < m_u;
    const uint32_t nw = live ? n_words : 0u;             // (a wave past the last row walks nothing)
    unsigned long long *row = rows[wave];
    uint32_t d = 0u;
    for (uint32_t x = lane; x < nw; x += kWave) {
        const unsigned long long b = adj[(size_t)x * m_u + u];
        row[x] = b;
        d += (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t acc = 0u;
    for (uint32_t word = 0; word < nw; ++word) {
        const unsigned long long bits = row[word];       // (one address for the wave: a broadcast)
        if (bits == 0ull) continue;
        if ((bits >> lane) & 1ull) {
            const uint32_t v = word * kWave + lane;       // (< m_u: the bits past M_u are zero)
            uint32_t s = 0u;
            for (uint32_t x = 0; x < nw; ++x) s += (uint32_t)__popcll(row[x] & adj[(size_t)x * m_u + v]);
            acc += s;
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) { d += __shfl_xor(d, off); acc += __shfl_xor(acc, off); }
    if (live && lane == 0u) {
        deg[u] = d;
        w[u] = acc;
        key[u] = ((unsigned long long)(0xFFFFFFFFu - acc) << 32) | (unsigned long long)u;
    }
}

// the block's maximum of x in every thread; red: kBlock / kWave words of LDS
DCREG_DEVFN uint32_t block_max(uint32_t x, uint32_t *red) {
    for (int off = kWave / 2; off > 0; off >>= 1) x = max(x, (uint32_t)__shfl_xor(x, off));
    __syncthreads();                                      // (the call before is read no more)
    if ((threadIdx.x & (kWave - 1)) == 0u) red[threadIdx.x / kWave] = x;
    __syncthreads();
    uint32_t m = red[0];
    for (int k = 1; k < kBlock / kWave; ++k) m = max(m, red[k]);
    return m;
}

// Block r: the seed of rank r.  mem[64 r ..]: its members as used-pair numbers in ascending u, n_mem[r]: how many.  s_row: M_u counts per seed
static __global__ __launch_bounds__(kBlock) void k_cons_members(const unsigned long long *__restrict__ adj, uint32_t m_u, uint32_t n_words,
                                                                const unsigned long long *__restrict__ key_sorted, uint32_t consensus_size,
                                                                uint16_t *__restrict__ s_row, uint32_t *__restrict__ mem,
                                                                uint32_t *__restrict__ n_mem) {
    __shared__ uint32_t red[kBlock / kWave];
    __shared__ uint32_t sel[kConsMaxSet];
    const uint32_t tid = threadIdx.x, r = blockIdx.x, s = (uint32_t)(key_sorted[r] & 0xFFFFFFFFull);
    uint16_t *srow = s_row + (size_t)r * m_u;
    uint32_t mx = 0u;
    for (uint32_t v = tid; v < m_u; v += kBlock) {
        uint32_t S = 0u;
        if ((adj[(size_t)(v / kWave) * m_u + s] >> (v & (kWave - 1))) & 1ull)
            for (uint32_t x = 0; x < n_words; ++x) S += (uint32_t)__popcll(adj[(size_t)x * m_u + s] & adj[(size_t)x * m_u + v]);
        srow[v] = (uint16_t)S;                            // (S <= M_u - 2 < 2^15; a thread reads back only what it wrote itself)
        mx = max(mx, S);
    }
    const uint32_t s_max = block_max(mx, red);
    // a candidate's key: (S descending, v ascending) is the key descending; S >= 1 makes it positive
    uint32_t prev = 0xFFFFFFFFu, n_sel = 0u;
    for (uint32_t k = 0; k + 1u < consensus_size; ++k) {
        uint32_t best = 0u;
        for (uint32_t v = tid; v < m_u; v += kBlock) {
            const uint32_t S = srow[v], kv = (S << 15) | (0x7FFFu - v);
            const bool cand = S >= 1u && 2u * S >= s_max && kv < prev;
            best = max(best, cand ? kv : 0u);
        }
        best = block_max(best, red);
        if (best == 0u) break;                            // (the whole block alike)
        if (tid == 0u) sel[n_sel] = 0x7FFFu - (best & 0x7FFFu);
        prev = best;
        n_sel += 1u;
    }
    __syncthreads();
    const uint32_t n = n_sel + 1u;                        // (the seed itself: S(s, s) = 0, it is not among the selected)
    if (tid < n) {
        const uint32_t mine = tid < n_sel ? sel[tid] : s;
        uint32_t rank = 0u;
        for (uint32_t j = 0; j < n; ++j) rank += (j < n_sel ? sel[j] : s) < mine ? 1u : 0u;
        mem[(size_t)kConsMaxSet * r + rank] = mine;
    }
    if (tid == 0u) n_mem[r] = n;
}

// Block (x, y): the sets [256 x, 256 x + 256) against the used pairs [chunk y, chunk y + chunk): count and cost of each, added to its
// key.  pose: R row-major, then t.  dd = d * d
static __global__ __launch_bounds__(kBlock) void k_cons_score(const float *__restrict__ P, uint32_t m_u, const double *__restrict__ pose, double dd,
                                                              uint32_t n_sets, uint32_t chunk, AlignKey *__restrict__ keys) {
    __shared__ double tile[kScoreTile * kAlignPairFloats];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * kBlock + tid;
    const bool live = i < n_sets;
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = pose[12 * (size_t)(live ? i : 0u) + k];
    for (int k = 0; k < 3; ++k) t[k] = pose[12 * (size_t)(live ? i : 0u) + 9 + k];
    const uint32_t u_begin = blockIdx.y * chunk, u_end = m_u - u_begin > chunk ? u_begin + chunk : m_u;      // (u_begin < m_u: the grid's y)
    uint32_t count = 0u;
    unsigned long long cost = 0ull;
    for (uint32_t t0 = u_begin; t0 < u_end; t0 += kScoreTile) {
        const uint32_t rows = min((uint32_t)kScoreTile, u_end - t0);
        __syncthreads();                                  // (the tile of the trip before is read no more)
        for (uint32_t e = tid; e < rows * kAlignPairFloats; e += kBlock) tile[e] = (double)P[(size_t)t0 * kAlignPairFloats + e];
        __syncthreads();
        for (uint32_t r = 0; r < rows; ++r) {
            const double *row = tile + r * kAlignPairFloats;
            const double e2 = align_e2(R, t, row[0], row[1], row[2], row[3], row[4], row[5]);
            const bool in = e2 <= dd;
            count += in ? 1u : 0u;
            if (__ballot(in) != 0ull) cost += (unsigned long long)floor(((in ? e2 : 0.0) / dd) * 1048576.0);
        }
    }
    if (live) {
        if (count) atomicAdd(&keys[i].count, count);
        if (cost) atomicAdd(&keys[i].cost, cost);
    }
}

// deg and w of the used pairs at their correspondence numbers (the outputs are zero elsewhere; either may be null)
static __global__ void k_cons_scatter(const int32_t *__restrict__ m_of_u, uint32_t m_u, const uint32_t *__restrict__ deg, const uint32_t *__restrict__ w,
                                      uint32_t *__restrict__ out_deg, uint32_t *__restrict__ out_w) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= m_u) return;
    const int32_t m = m_of_u[u];
    if (out_deg) out_deg[m] = deg[u];
    if (out_w) out_w[m] = w[u];
}

int cons_check(dcreg_ctx *c, const dcreg_consensus_params *p) {
    if (!p) { c->fail("null consensus parameters"); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->compat_distance) && p->compat_distance > 0.0)) { c->fail("compat_distance is %g: finite and > 0 expected", p->compat_distance); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->min_length) && p->min_length >= 0.0)) { c->fail("min_length is %g: finite and >= 0 expected", p->min_length); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->inlier_distance) && p->inlier_distance > 0.0)) { c->fail("inlier_distance is %g: finite and > 0 expected", p->inlier_distance); return DCREG_E_INVALID; }
    if (p->n_seeds < 1 || p->n_seeds > kConsMaxSeeds) { c->fail("n_seeds is %d: 1 .. %d expected", p->n_seeds, kConsMaxSeeds); return DCREG_E_INVALID; }
    if (p->consensus_size < 3 || p->consensus_size > kConsMaxSet) { c->fail("consensus_size is %d: 3 .. %d expected", p->consensus_size, kConsMaxSet); return DCREG_E_INVALID; }
    if (p->n_best < 1 || p->n_best > kMaxBest) { c->fail("n_best is %d: 1 .. %d expected", p->n_best, kMaxBest); return DCREG_E_INVALID; }
    if (p->refine_iterations < 0 || p->refine_iterations > kMaxRefine) { c->fail("refine_iterations is %d: 0 .. %d expected", p->refine_iterations, kMaxRefine); return DCREG_E_INVALID; }
    return DCREG_OK;
}

// the caller's outputs of a call; on_device: device memory
struct ConsOut {
    uint8_t *mask;
    int32_t *members;
    uint32_t *degree, *weight;
    bool on_device;
};

// the mask and the member lists of a call without a record (all zero, all -1), and - with graph false: no graph was built - zero degrees
// and weights
int cons_no_record(dcreg_ctx *c, const ConsOut &o, int64_t n_pairs, const dcreg_consensus_params *p, bool graph) {
    const size_t np = (size_t)std::max<int64_t>(n_pairs, 0), nm = (size_t)p->n_best * (size_t)p->consensus_size;
    if (!o.on_device) {
        if (o.mask && np) std::memset(o.mask, 0, np);
        if (o.members) std::memset(o.members, 0xFF, sizeof(int32_t) * nm);
        if (!graph && o.degree && np) std::memset(o.degree, 0, sizeof(uint32_t) * np);
        if (!graph && o.weight && np) std::memset(o.weight, 0, sizeof(uint32_t) * np);
        return DCREG_OK;
    }
    if (!(o.mask || o.members || (!graph && (o.degree || o.weight)))) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (o.mask && np) HIP_TRY(c, hipMemsetAsync(o.mask, 0, np, c->stream));
    if (o.members) HIP_TRY(c, hipMemsetAsync(o.members, 0xFF, sizeof(int32_t) * nm, c->stream));
    if (!graph && o.degree && np) HIP_TRY(c, hipMemsetAsync(o.degree, 0, sizeof(uint32_t) * np, c->stream));
    if (!graph && o.weight && np) HIP_TRY(c, hipMemsetAsync(o.weight, 0, sizeof(uint32_t) * np, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

struct ConsKeyLess {
    bool operator()(const AlignKey &a, const AlignKey &b) const {
        if (a.count != b.count) return a.count > b.count;
        if (a.cost != b.cost) return a.cost < b.cost;
        return a.h < b.h;                                 // (the places of the scored sets ascend with their ranks)
    }
};

int cons_run(dcreg_ctx *c, const float *a, int64_t n_a, int64_t stride_a, const float *b, int64_t n_b, int64_t stride_b, const int32_t *ca,
             const int32_t *cb, int64_t n_pairs, const dcreg_consensus_params *p, dcreg_consensus_record *rec, const ConsOut &out,
             dcreg_consensus_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = cons_check(c, p)) return rc;
    if (!rec) { c->fail("null record buffer"); return DCREG_E_INVALID; }
    if (n_a < 0 || n_b < 0 || n_pairs < 0 || stride_a < 3 || stride_b < 3) { c->fail("invalid consensus arguments"); return DCREG_E_INVALID; }
    if (n_a > (int64_t)INT32_MAX || n_b > (int64_t)INT32_MAX) { c->fail("too many points for one consensus call"); return DCREG_E_INVALID; }
    if (n_pairs > kMaxPairs) { c->fail("n_pairs is %lld: at most %lld expected (the graph is a bit matrix)", (long long)n_pairs, (long long)kMaxPairs); return DCREG_E_INVALID; }
    if ((n_a > 0 && !a) || (n_b > 0 && !b)) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    if (n_pairs > 0 && (!ca || !cb)) { c->fail("null correspondence buffer"); return DCREG_E_INVALID; }
    std::memset(rec, 0, sizeof(*rec) * (size_t)p->n_best);
    dcreg_consensus_info I;
    std::memset(&I, 0, sizeof(I));
    I.n_pairs = n_pairs;
    if (info) *info = I;
    if (n_pairs == 0) return cons_no_record(c, out, n_pairs, p, false);
    const bool on_device = out.on_device;
    dcreg_ctx::AlignBufs &A = c->algn;
    dcreg_ctx::ConsensusBufs &G = c->cons;
    const size_t np = (size_t)n_pairs;
    // ---- the used pairs
    uint32_t m_u = 0;
    if (int rc = align_used_pairs(c, a, n_a, stride_a, b, n_b, stride_b, ca, cb, n_pairs, on_device, &m_u)) return rc;
    I.n_used = (int64_t)m_u;
    if (info) *info = I;
    if (m_u < 3u) return cons_no_record(c, out, n_pairs, p, false);
    const int32_t *dca = on_device ? ca : A.ca.data(), *dcb = on_device ? cb : A.cb.data();
    // ---- the graph, the weights, the seeds and their sets
    const uint32_t n_words = (m_u + (uint32_t)kWave - 1u) / (uint32_t)kWave, n_take = std::min<uint32_t>((uint32_t)p->n_seeds, m_u);
    if (G.adj.ensure(c, (size_t)n_words * m_u) || G.deg.ensure(c, m_u) || G.w.ensure(c, m_u) || G.key.ensure(c, m_u) || G.key_sorted.ensure(c, m_u) ||
        G.s_row.ensure(c, (size_t)n_take * m_u) || G.mem.ensure(c, (size_t)kConsMaxSet * n_take) || G.n_mem.ensure(c, n_take))
        return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_cons_adjacency, dim3(blocks(m_u, kBlock), blocks(n_words, kAdjWords)), dim3(kBlock), 0, c->stream, A.P.data(), A.m_of_u.data(), dca,
                       dcb, m_u, n_words, p->min_length, p->compat_distance, G.adj.data());
    hipLaunchKernelGGL(k_cons_weights, dim3(blocks(m_u, kRowsPerBlock)), dim3(kBlock), 0, c->stream, G.adj.data(), m_u, n_words, G.deg.data(), G.w.data(),
                       G.key.data());
    HIP_TRY(c, hipGetLastError());
    {
        size_t tmp = 0;
        HIP_TRY(c, rocprim::radix_sort_keys(nullptr, tmp, G.key.data(), G.key_sorted.data(), (size_t)m_u, 0u, 64u, c->stream));
        if (c->sort_tmp.ensure(c, tmp) != DCREG_OK) return DCREG_E_NOMEM;
        HIP_TRY(c, rocprim::radix_sort_keys(c->sort_tmp.data(), tmp, G.key.data(), G.key_sorted.data(), (size_t)m_u, 0u, 64u, c->stream));
    }
    hipLaunchKernelGGL(k_cons_members, dim3(n_take), dim3(kBlock), 0, c->stream, G.adj.data(), m_u, n_words, G.key_sorted.data(), (uint32_t)p->consensus_size,
                       G.s_row.data(), G.mem.data(), G.n_mem.data());
    HIP_TRY(c, hipGetLastError());
    if (on_device && (out.degree || out.weight)) {
        if (out.degree) HIP_TRY(c, hipMemsetAsync(out.degree, 0, sizeof(uint32_t) * np, c->stream));
        if (out.weight) HIP_TRY(c, hipMemsetAsync(out.weight, 0, sizeof(uint32_t) * np, c->stream));
        hipLaunchKernelGGL(k_cons_scatter, dim3(blocks(m_u, kBlock)), dim3(kBlock), 0, c->stream, A.m_of_u.data(), m_u, G.deg.data(), G.w.data(), out.degree,
                           out.weight);
        HIP_TRY(c, hipGetLastError());
    }
    std::vector<float> hP(kAlignPairFloats * (size_t)m_u);
    std::vector<int32_t> hm((size_t)m_u);
    std::vector<uint32_t> hdeg((size_t)m_u), hw((size_t)m_u), hmem((size_t)kConsMaxSet * n_take), hn((size_t)n_take);
    std::vector<unsigned long long> hkey((size_t)n_take);
    HIP_TRY(c, hipMemcpyAsync(hP.data(), A.P.data(), sizeof(float) * hP.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hm.data(), A.m_of_u.data(), sizeof(int32_t) * hm.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hdeg.data(), G.deg.data(), sizeof(uint32_t) * hdeg.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hw.data(), G.w.data(), sizeof(uint32_t) * hw.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hkey.data(), G.key_sorted.data(), sizeof(unsigned long long) * hkey.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hmem.data(), G.mem.data(), sizeof(uint32_t) * hmem.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hn.data(), G.n_mem.data(), sizeof(uint32_t) * hn.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    int64_t deg_sum = 0, deg_max = 0;
    for (uint32_t u = 0; u < m_u; ++u) { deg_sum += hdeg[u]; deg_max = std::max<int64_t>(deg_max, hdeg[u]); }
    if (!on_device) {
        if (out.degree) { std::memset(out.degree, 0, sizeof(uint32_t) * np); for (uint32_t u = 0; u < m_u; ++u) out.degree[hm[u]] = hdeg[u]; }
        if (out.weight) { std::memset(out.weight, 0, sizeof(uint32_t) * np); for (uint32_t u = 0; u < m_u; ++u) out.weight[hm[u]] = hw[u]; }
    }
    std::vector<uint32_t> seed_u((size_t)n_take), seed_w((size_t)n_take), set;
    for (uint32_t r = 0; r < n_take; ++r) {
        seed_u[r] = (uint32_t)(hkey[r] & 0xFFFFFFFFull);
        seed_w[r] = 0xFFFFFFFFu - (uint32_t)(hkey[r] >> 32);
        if (hn[r] >= 3u) set.push_back(r);
    }
    const uint32_t n_sets = (uint32_t)set.size();
    I.n_edges = deg_sum / 2; I.max_degree = deg_max; I.n_seeds = n_take; I.n_skipped = n_take - n_sets; I.n_scored = n_sets;
    if (info) *info = I;
    if (n_sets == 0u) return cons_no_record(c, out, n_pairs, p, true);
    // ---- the sets' poses and scores
    std::vector<double> pose(12 * (size_t)n_sets);
    consensus_host_fit(hP.data(), hmem.data(), hn.data(), set.data(), (int)n_sets, pose.data());
    std::vector<AlignKey> keys((size_t)n_sets);
    for (uint32_t i = 0; i < n_sets; ++i) { keys[i].count = 0u; keys[i].h = i; keys[i].cost = 0ull; }
    if (G.pose.ensure(c, pose.size()) || G.score.ensure(c, n_sets)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemcpyAsync(G.pose.data(), pose.data(), sizeof(double) * pose.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(G.score.data(), keys.data(), sizeof(AlignKey) * keys.size(), hipMemcpyHostToDevice, c->stream));
    const int64_t blocks_x = blocks(n_sets, kBlock), tiles = ((int64_t)m_u + kScoreTile - 1) / kScoreTile;
    const int64_t want = std::min(std::max<int64_t>(1, 1024 / blocks_x), tiles);        // about a thousand blocks, a split no shorter than a tile
    const int64_t chunk = (tiles + want - 1) / want * kScoreTile, n_split = ((int64_t)m_u + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_cons_score, dim3((unsigned)blocks_x, (unsigned)n_split), dim3(kBlock), 0, c->stream, A.P.data(), m_u, G.pose.data(),
                       p->inlier_distance * p->inlier_distance, n_sets, (uint32_t)chunk, G.score.data());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(keys.data(), G.score.data(), sizeof(AlignKey) * keys.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    std::sort(keys.begin(), keys.end(), ConsKeyLess());
    const int n_rec = (int)std::min<int64_t>(p->n_best, n_sets);
    // ---- the records
    const size_t nm = (size_t)p->n_best * (size_t)p->consensus_size;
    std::vector<uint8_t> hmask;
    std::vector<int32_t> hmembers;
    if (on_device && out.mask) hmask.resize(np);
    if (on_device && out.members) hmembers.resize(nm);
    consensus_host_records(hP.data(), hm.data(), (int64_t)m_u, n_pairs, p, keys.data(), n_rec, pose.data(), set.data(), seed_u.data(), seed_w.data(),
                           hmem.data(), hn.data(), rec, out.mask ? (on_device ? hmask.data() : out.mask) : nullptr,
                           out.members ? (on_device ? hmembers.data() : out.members) : nullptr);
    if (on_device && (out.mask || out.members)) {
        if (out.mask) HIP_TRY(c, hipMemcpyAsync(out.mask, hmask.data(), np, hipMemcpyHostToDevice, c->stream));
        if (out.members) HIP_TRY(c, hipMemcpyAsync(out.members, hmembers.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    I.n_returned = n_rec;
    if (info) *info = I;
    return DCREG_OK;
}

}  // namespace
}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_default_consensus_params(dcreg_consensus_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->compat_distance = 0.5; p->min_length = 1.0; p->inlier_distance = 0.5; p->n_seeds = 64; p->consensus_size = 16; p->n_best = 1;
    p->refine_iterations = 3;
    return DCREG_OK;
}
int dcreg_consensus_correspondences(dcreg_ctx *c, const float *a_xyz, int64_t n_a, int64_t stride_a, const float *b_xyz, int64_t n_b, int64_t stride_b,
                                    const int32_t *corr_a, const int32_t *corr_b, int64_t n_pairs, const dcreg_consensus_params *p,
                                    dcreg_consensus_record *records_out, uint8_t *inlier_mask_out, int32_t *members_out, uint32_t *degree_out,
                                    uint32_t *weight_out, dcreg_consensus_info *info) {
    return cons_run(c, a_xyz, n_a, stride_a, b_xyz, n_b, stride_b, corr_a, corr_b, n_pairs, p, records_out,
                    ConsOut{inlier_mask_out, members_out, degree_out, weight_out, false}, info);
}
int dcreg_consensus_correspondences_device(dcreg_ctx *c, const float *d_a_xyz, int64_t n_a, int64_t stride_a, const float *d_b_xyz, int64_t n_b,
                                           int64_t stride_b, const int32_t *d_corr_a, const int32_t *d_corr_b, int64_t n_pairs,
                                           const dcreg_consensus_params *p, dcreg_consensus_record *records_out, uint8_t *d_inlier_mask_out,
                                           int32_t *d_members_out, uint32_t *d_degree_out, uint32_t *d_weight_out, dcreg_consensus_info *info) {
    return cons_run(c, d_a_xyz, n_a, stride_a, d_b_xyz, n_b, stride_b, d_corr_a, d_corr_b, n_pairs, p, records_out,
                    ConsOut{d_inlier_mask_out, d_members_out, d_degree_out, d_weight_out, true}, info);
}
}
