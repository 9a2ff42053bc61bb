// Place recognition (include/dcreg.h: dcreg_place_descriptors*, dcreg_places_*): Scan Context descriptors of raw clouds, a database of them
// that lives in the context, and an exhaustive search of it over all column shifts.
//   k_place_bins     batched over clouds: a point's bin from its polar coordinates in fp64, an integer atomicMax of the order-preserving key of
//                    its height (LDS where a block's tile lies in one cloud, then one global atomic per occupied bin; per point otherwise):
//                    the maximum does not depend on order, so neither does the descriptor
//   k_place_finish   per (descriptor, column): keys to floats (an empty bin to 0) and the column's inverse norm, summed ring by ring in fp64
//   k_place_dist     per (query, entry): the column-cosine matrix Qn^T Cn as v_mfma_f64_16x16x4_f64 tiles of the normalised columns (one wave
//                    per pair, one k-step per 4 rings), each 16-row strip through LDS, where lane n sums its circulant diagonal row by row
//                    (a fixed order), then the wave's (distance, shift) minimum.  A block takes a few entries against a run of queries, so
//                    the entries are read from memory once per query batch
//   k_place_select   the k smallest (distance, index) of a chunk of 4096 candidates by k block-wide minima; chunks of chunks until one is left
//   k_place_gather   the shifts of the selected entries
// A pair's result is one instruction sequence on its two descriptors: it does not depend on the batch, the range, k or the database's size.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime.h>

#include "context.hpp"

namespace dcreg {
namespace {

constexpr int kPlBlock = 256;
constexpr int kPlPerThread = 8;                          // points per thread of k_place_bins (a block covers one tile of 2048 points)
constexpr int kPlMaxBins = 64 * 128;                     // n_rings <= 64, n_sectors <= 128
constexpr int kSelBlock = 256;
constexpr int kSelChunk = 4096;                          // candidates per block of k_place_select
constexpr int kDistEntries = 4, kDistQueries = 16;       // entries x queries of one block of k_place_dist
constexpr int64_t kDistBatchPairs = (int64_t)1 << 24;    // (query, entry) pairs whose distances are kept at once (12 B each)
constexpr int kNoIndex = 0x7FFFFFFF;                     // k_place_select: a candidate that is used up or never was one

// what the kernels need of dcreg_place_params
struct PlaceDev {
    int n_rings, n_sectors;
    double max_range, min2, max2, z_offset;
};

// order-preserving key of a float (ascending keys = ascending values) and its inverse.  No float that is not a NaN has key 0: an empty bin
__device__ __forceinline__ uint32_t fkey_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_value(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

// the bin of a finite point by the rules of include/dcreg.h (-1: outside the range gate) and the value it offers to it.  Every operation
// and its order are the header's: a folded constant (n_sectors / 2 pi, n_rings / max_range) or a gate on the root moves points that lie on
// an edge into another bin (tests/places_edge_scenes.py)
__device__ __forceinline__ int place_bin(const PlaceDev &P, float x, float y, float z, float &val) {
    const double dx = (double)x, dy = (double)y;
    const double r2 = dx * dx + dy * dy;
    if (!(r2 >= P.min2 && r2 < P.max2)) return -1;
    const double a = sqrt(r2) * (double)P.n_rings / P.max_range;
    const int ring = min((int)floor(a), P.n_rings - 1);
    double th = atan2(dy, dx);
    if (th < 0.0) th += 6.283185307179586;
    const double b = th * (double)P.n_sectors / 6.283185307179586;
    const int sector = min((int)floor(b), P.n_sectors - 1);
    val = (float)((double)z + P.z_offset);
    return ring * P.n_sectors + sector;
}

// keys[cloud][bin] = the largest key offered to the bin (0: none); cnt[0] += finite points, cnt[1] += points inside the range gate
static __global__ void __launch_bounds__(kPlBlock) k_place_bins(const float4 *__restrict__ pts, int64_t n, const int64_t *__restrict__ off, int n_clouds,
                                                                PlaceDev P, uint32_t *__restrict__ keys, unsigned long long *__restrict__ cnt) {
    __shared__ uint32_t sk[kPlMaxBins];
    __shared__ unsigned int sc[kPlBlock / 64][2];
    const int bins = P.n_rings * P.n_sectors;
    const int64_t base = (int64_t)blockIdx.x * (kPlBlock * kPlPerThread);
    const int64_t last = std::min<int64_t>(n, base + kPlBlock * kPlPerThread) - 1;
    const uint32_t s0 = n_clouds == 1 ? 0u : seg_of(off, n_clouds, base);
    const bool uniform = n_clouds == 1 || seg_of(off, n_clouds, last) == s0;      // (block-uniform)
    if (uniform) {
        for (int b = threadIdx.x; b < bins; b += kPlBlock) sk[b] = 0u;
        __syncthreads();
    }
    unsigned int fin = 0, used = 0;
    for (int k = 0; k < kPlPerThread; ++k) {
        const int64_t i = base + threadIdx.x + (int64_t)k * kPlBlock;
        if (i > last) break;
        const float4 p = pts[i];
        if (!finite_xyz(p.x, p.y, p.z)) continue;
        ++fin;
        float v;
        const int bin = place_bin(P, p.x, p.y, p.z, v);
        if (bin < 0) continue;
        ++used;
        if (uniform) atomicMax(&sk[bin], fkey_of(v));
        else atomicMax(keys + (size_t)seg_of(off, n_clouds, i) * bins + bin, fkey_of(v));
    }
    if (uniform) {
        __syncthreads();
        for (int b = threadIdx.x; b < bins; b += kPlBlock) {
            const uint32_t k = sk[b];
            if (k) atomicMax(keys + (size_t)s0 * bins + b, k);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        fin += __shfl_xor(fin, o);
        used += __shfl_xor(used, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sc[wave][0] = fin; sc[wave][1] = used; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kPlBlock / 64; ++w) { fin += sc[w][0]; used += sc[w][1]; }
        if (fin) atomicAdd(cnt, (unsigned long long)fin);
        if (used) atomicAdd(cnt + 1, (unsigned long long)used);
    }
}

// per (descriptor, column): with keys, the column's bins become floats (an empty bin 0); then inv = 1 / |column| (0 for a zero column), the
// squares summed ring by ring in fp64
static __global__ void __launch_bounds__(kPlBlock) k_place_finish(const uint32_t *__restrict__ keys, int64_t n_desc, int R, int S,
                                                                  float *__restrict__ desc, double *__restrict__ inv) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_desc * S) return;
    const int64_t e = t / S;
    const int j = (int)(t - e * S);
    const size_t at = (size_t)e * R * S + j;
    double ss = 0.0;
    for (int r = 0; r < R; ++r) {
        float v;
        if (keys) {
            const uint32_t k = keys[at + (size_t)r * S];
            v = k ? fkey_value(k) : 0.f;
            desc[at + (size_t)r * S] = v;
        } else {
            v = desc[at + (size_t)r * S];
        }
        ss += (double)v * (double)v;
    }
    inv[t] = ss > 0.0 ? 1.0 / sqrt(ss) : 0.0;
}

typedef double mfma_d4 __attribute__((ext_vector_type(4)));

// bit `col` of a 128-bit column mask
__device__ __forceinline__ int mask_bit(unsigned long long m0, unsigned long long m1, int col) {
    return (int)(((col < 64 ? m0 : m1) >> (col & 63)) & 1ull);
}

// One wave per block; the block's entries [first + e0, ..) against its queries.  NT = 16-column tiles of an entry (n_sectors <= 16 NT), JT =
// 16-column tiles of the query whose products are accumulated together (JT x NT accumulator tiles of 4 doubles per lane).  Operand layout
// of v_mfma_f64_16x16x4_f64: A[i][k] / B[k][j] in lane i + 16 k; D[row][col]: col = lane & 15, row = (lane >> 4) + 4 reg.  Here i = a query
// column, j = an entry column, k = a ring.  Lane n (and n + 64) sums the diagonal of shift n over the rows j = 0, 1, .. in that order.
template <int NT, int JT>
static __global__ void __launch_bounds__(64) k_place_dist(const float *__restrict__ qdesc, const double *__restrict__ qinv, int nq,
                                                          const float *__restrict__ db, const double *__restrict__ dbinv, int64_t first, int64_t ne,
                                                          int R, int S, double *__restrict__ dist, int32_t *__restrict__ shift) {
    constexpr int LD = NT * 16;
    __shared__ double strip[16 * LD];
    const int lane = threadIdx.x, c16 = lane & 15, k4 = lane >> 4;
    const int KS = (R + 3) >> 2, NJ = (S + 15) >> 4;
    const int n0 = lane < S ? lane : 0, n1 = lane + 64 < S ? lane + 64 : 0;
    const int64_t e0 = (int64_t)blockIdx.x * kDistEntries, e1 = std::min<int64_t>(ne, e0 + kDistEntries);
    const int q0 = blockIdx.y * kDistQueries, q1 = min(nq, q0 + kDistQueries);
    const size_t bins = (size_t)R * S;
    for (int64_t eo = e0; eo < e1; ++eo) {
        const float *__restrict__ Cd = db + (size_t)(first + eo) * bins;
        const double *__restrict__ ci = dbinv + (size_t)(first + eo) * S;
        double bc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bc[t] = 16 * t + c16 < S ? ci[16 * t + c16] : 0.0;
        const unsigned long long cm0 = __ballot(lane < S && ci[n0] != 0.0), cm1 = __ballot(lane + 64 < S && ci[n1] != 0.0);
        for (int q = q0; q < q1; ++q) {
            const float *__restrict__ Qd = qdesc + (size_t)q * bins;
            const double *__restrict__ qi = qinv + (size_t)q * S;
            const unsigned long long qm0 = __ballot(lane < S && qi[n0] != 0.0), qm1 = __ballot(lane + 64 < S && qi[n1] != 0.0);
            // every column of both has a norm: m = n_sectors at every shift (block-uniform)
            const bool all = __popcll(cm0) + __popcll(cm1) == S && __popcll(qm0) + __popcll(qm1) == S;
            double s0 = 0.0, s1 = 0.0;
            int m0 = all ? S : 0, m1 = m0;
            for (int jg = 0; jg * JT < NJ; ++jg) {
                double aq[JT];
#pragma unroll
                for (int u = 0; u < JT; ++u) {
                    const int col = 16 * (jg * JT + u) + c16;
                    aq[u] = col < S ? qi[col] : 0.0;
                }
                mfma_d4 acc[JT][NT];
#pragma unroll
                for (int u = 0; u < JT; ++u)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[u][t] = mfma_d4{0.0, 0.0, 0.0, 0.0};
                for (int ks = 0; ks < KS; ++ks) {
                    const int r = 4 * ks + k4;
                    const bool rok = r < R;
                    double b[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int col = 16 * t + c16;
                        b[t] = (rok && col < S) ? (double)Cd[(size_t)r * S + col] * bc[t] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < JT; ++u) {
                        const int col = 16 * (jg * JT + u) + c16;
                        const double a = (rok && col < S) ? (double)Qd[(size_t)r * S + col] * aq[u] : 0.0;
                        if (jg * JT + u < NJ) {
#pragma unroll
                            for (int t = 0; t < NT; ++t)
                                if (t < NJ) acc[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[u][t], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < JT; ++u) {
                    const int jt = jg * JT + u;
                    if (jt < NJ) {                           // (block-uniform)
                        __syncthreads();                     // the strip's readers of the tile before are done
#pragma unroll
                        for (int t = 0; t < NT; ++t)
#pragma unroll
                            for (int g = 0; g < 4; ++g) strip[(k4 + 4 * g) * LD + 16 * t + c16] = acc[u][t][g];
                        __syncthreads();
                        const int rows = min(16, S - 16 * jt);
                        for (int jj = 0; jj < rows; ++jj) {
                            const int j = 16 * jt + jj;
                            int col0 = j + n0, col1 = j + n1;
                            if (col0 >= S) col0 -= S;
                            if (col1 >= S) col1 -= S;
                            s0 += strip[jj * LD + col0];
                            if (NT > 4) s1 += strip[jj * LD + col1];
                            if (!all && mask_bit(qm0, qm1, j)) {
                                m0 += mask_bit(cm0, cm1, col0);
                                if (NT > 4) m1 += mask_bit(cm0, cm1, col1);
                            }
                        }
                    }
                }
            }
            const double inf = __builtin_huge_val();
            double bd = lane < S ? (m0 > 0 ? 1.0 - s0 / (double)m0 : 1.0) : inf;
            int bn = lane;
            if (NT > 4 && lane + 64 < S) {
                const double d1 = m1 > 0 ? 1.0 - s1 / (double)m1 : 1.0;
                if (d1 < bd) { bd = d1; bn = lane + 64; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double od = __shfl_xor(bd, o);
                const int on = __shfl_xor(bn, o);
                if (od < bd || (od == bd && on < bn)) { bd = od; bn = on; }
            }
            if (lane == 0) {
                dist[(size_t)q * ne + eo] = bd;
                shift[(size_t)q * ne + eo] = bn;
            }
        }
    }
}

// the k smallest (distance, index) of chunk blockIdx.x of query blockIdx.y's n_in candidates, in that order, to out[query][chunk k ..];
// in_i == null: candidate p is entry first + p.  Slots beyond the candidates hold index -1 and distance +inf
static __global__ void __launch_bounds__(kSelBlock) k_place_select(const double *__restrict__ in_d, const int32_t *__restrict__ in_i, int64_t n_in,
                                                                   int64_t first, int k, double *__restrict__ out_d, int32_t *__restrict__ out_i,
                                                                   int64_t out_stride) {
    __shared__ double sd[kSelChunk];
    __shared__ int32_t si[kSelChunk];
    __shared__ double wd[kSelBlock / 64];
    __shared__ int32_t wi[kSelBlock / 64], wp[kSelBlock / 64];
    const double inf = __builtin_huge_val();
    const int64_t base = (int64_t)blockIdx.x * kSelChunk;
    const size_t row = (size_t)blockIdx.y * (size_t)n_in;
    for (int p = threadIdx.x; p < kSelChunk; p += kSelBlock) {
        double d = inf;
        int32_t i = kNoIndex;
        if (base + p < n_in) {
            const int32_t ii = in_i ? in_i[row + base + p] : (int32_t)(first + base + p);
            if (ii >= 0) { i = ii; d = in_d[row + base + p]; }
        }
        sd[p] = d;
        si[p] = i;
    }
    __syncthreads();
    for (int s = 0; s < k; ++s) {
        double bd = inf;
        int32_t bi = kNoIndex, bp = threadIdx.x;
        for (int p = threadIdx.x; p < kSelChunk; p += kSelBlock) {
            const double d = sd[p];
            const int32_t i = si[p];
            if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; bp = p; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o);
            const int32_t oi = __shfl_xor(bi, o), op = __shfl_xor(bp, o);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; bp = op; }
        }
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { wd[wave] = bd; wi[wave] = bi; wp[wave] = bp; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kSelBlock / 64; ++w)
                if (wd[w] < bd || (wd[w] == bd && wi[w] < bi)) { bd = wd[w]; bi = wi[w]; bp = wp[w]; }
            const bool none = bi == kNoIndex;
            const size_t o = (size_t)blockIdx.y * (size_t)out_stride + (size_t)blockIdx.x * k + s;
            out_d[o] = none ? inf : bd;
            out_i[o] = none ? -1 : bi;
            sd[bp] = inf;
            si[bp] = kNoIndex;
        }
        __syncthreads();
    }
}

// the shift of every selected entry (0 for an unused slot)
static __global__ void __launch_bounds__(kPlBlock) k_place_gather(const int32_t *__restrict__ idx, int64_t n, int k, const int32_t *__restrict__ shift,
                                                                  int64_t first, int64_t ne, int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int32_t i = idx[t];
    out[t] = i >= 0 ? shift[(size_t)(t / k) * (size_t)ne + (size_t)(i - first)] : 0;
}

int check_params(dcreg_ctx *c, const dcreg_place_params *p) {
    if (!p) { c->fail("null place parameters"); return DCREG_E_INVALID; }
    if (p->n_rings < 1 || p->n_rings > 64) { c->fail("n_rings %d outside [1, 64]", p->n_rings); return DCREG_E_INVALID; }
    if (p->n_sectors < 1 || p->n_sectors > 128) { c->fail("n_sectors %d outside [1, 128]", p->n_sectors); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->max_range) && p->max_range > 0.0)) { c->fail("max_range %g: finite and > 0 expected", p->max_range); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->min_range) && p->min_range >= 0.0 && p->min_range < p->max_range)) {
        c->fail("min_range %g: finite, >= 0 and below max_range %g expected", p->min_range, p->max_range);
        return DCREG_E_INVALID;
    }
    if (!std::isfinite(p->z_offset)) { c->fail("z_offset %g is not finite", p->z_offset); return DCREG_E_INVALID; }
    return DCREG_OK;
}

int check_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride) {
    if (n_clouds < 0 || (n_clouds > 0 && !off) || stride < 3) { c->fail("invalid cloud arguments"); return DCREG_E_INVALID; }
    if (n_clouds > 0 && off[0] != 0) { c->fail("cloud offsets must start at 0"); return DCREG_E_INVALID; }
    for (int s = 0; s < n_clouds; ++s)
        if (off[s + 1] < off[s]) { c->fail("cloud offsets decrease at cloud %d", s); return DCREG_E_INVALID; }
    const int64_t n = n_clouds > 0 ? off[n_clouds] : 0;
    if (n >= ((int64_t)1 << 31) - 1) { c->fail("too many points for one call (%lld)", (long long)n); return DCREG_E_INVALID; }
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    return DCREG_OK;
}

int check_ready(dcreg_ctx *c) {
    if (!c->places.ready) { c->fail("no place database: dcreg_places_reset first"); return DCREG_E_STATE; }
    return DCREG_OK;
}

bool all_finite(const float *v, size_t n) {
    bool ok = true;
    for (size_t i = 0; i < n; ++i) ok &= std::isfinite(v[i]);
    return ok;
}

// at least `need` elements of which the first `keep` survive: the new block is allocated beside the old one, so a failure changes nothing
template <typename T>
int grow(dcreg_ctx *c, DevBuf<T> &b, size_t need, size_t keep) {
    if (b.holds(need)) return DCREG_OK;
    DevBuf<T> fresh;
    const size_t n = std::max(need, b.cap() + b.cap() / 2);
    if (fresh.alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        c->fail("hipMalloc(%zu B) failed while growing the place database", n * sizeof(T));
        return DCREG_E_NOMEM;
    }
    if (b && keep) HIP_TRY(c, hipMemcpyAsync(fresh.data(), b.data(), keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    b.swap(fresh);
    return DCREG_OK;
}

int grow_database(dcreg_ctx *c, int64_t n_more) {
    dcreg_ctx::PlaceBufs &B = c->places;
    const size_t bins = (size_t)B.p.n_rings * B.p.n_sectors, S = (size_t)B.p.n_sectors;
    if (B.count + n_more > (int64_t)INT32_MAX - 1) { c->fail("the place database would hold more than 2^31 - 2 entries"); return DCREG_E_INVALID; }
    if (int rc = grow(c, B.desc, (size_t)(B.count + n_more) * bins, (size_t)B.count * bins)) return rc;
    return grow(c, B.inv, (size_t)(B.count + n_more) * S, (size_t)B.count * S);
}

// where the clouds of a call come from: the caller's records, or the context's current source in its input order
struct CloudsIn {
    int n_clouds = 0;
    const float *xyz = nullptr;
    const int64_t *off = nullptr;
    int64_t stride = 3;
    bool on_device = false, from_source = false;
    int64_t n() const { return n_clouds > 0 ? off[n_clouds] : 0; }
};

// queues the descriptors of the clouds to d_desc [n_clouds][bins] and their inverse column norms to d_inv [n_clouds][n_sectors]; the call's
// counts go to cnt_host once the stream is waited for.  Every buffer it needs is reserved before anything is queued
int describe(dcreg_ctx *c, const CloudsIn &in, const dcreg_place_params &p, float *d_desc, double *d_inv, unsigned long long cnt_host[2]) {
    dcreg_ctx::PlaceBufs &B = c->places;
    cnt_host[0] = cnt_host[1] = 0;
    if (in.n_clouds == 0) return DCREG_OK;
    const size_t bins = (size_t)p.n_rings * p.n_sectors;
    const int64_t n = in.n();
    if (B.keys.ensure(c, (size_t)in.n_clouds * bins) || B.d_off.ensure(c, (size_t)in.n_clouds + 1) || B.cnt.ensure(c, 2)) return DCREG_E_NOMEM;
    const float4 *pts = c->d_src_raw.data();
    if (!in.from_source && n > 0) {
        if (int rc = upload_cloud(c, in.xyz, n, in.stride, in.on_device, c->vox.pts)) return rc;
        pts = c->vox.pts.data();
    }
    HIP_TRY(c, hipMemsetAsync(B.keys.data(), 0, sizeof(uint32_t) * (size_t)in.n_clouds * bins, c->stream));
    HIP_TRY(c, hipMemsetAsync(B.cnt.data(), 0, 2 * sizeof(unsigned long long), c->stream));
    if (n > 0) {
        HIP_TRY(c, hipMemcpyAsync(B.d_off.data(), in.off, sizeof(int64_t) * ((size_t)in.n_clouds + 1), hipMemcpyHostToDevice, c->stream));
        const PlaceDev P = {p.n_rings, p.n_sectors, p.max_range, p.min_range * p.min_range, p.max_range * p.max_range, p.z_offset};
        hipLaunchKernelGGL(k_place_bins, dim3(blocks(n, kPlBlock * kPlPerThread)), dim3(kPlBlock), 0, c->stream, pts, n, B.d_off.data(), in.n_clouds, P,
                           B.keys.data(), B.cnt.data());
    }
    hipLaunchKernelGGL(k_place_finish, dim3(blocks((int64_t)in.n_clouds * p.n_sectors, kPlBlock)), dim3(kPlBlock), 0, c->stream, B.keys.data(),
                       (int64_t)in.n_clouds, p.n_rings, p.n_sectors, d_desc, d_inv);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(cnt_host, B.cnt.data(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return DCREG_OK;
}

void fill_info(dcreg_place_info *info, int64_t n_in, const unsigned long long cnt[2]) {
    if (!info) return;
    info->n_in = n_in;
    info->n_finite = (int64_t)cnt[0];
    info->n_used = (int64_t)cnt[1];
}

// the inverse column norms of n descriptors that are already on the device
int norms(dcreg_ctx *c, float *d_desc, int64_t n, double *d_inv) {
    if (n == 0) return DCREG_OK;
    const dcreg_place_params &p = c->places.p;
    hipLaunchKernelGGL(k_place_finish, dim3(blocks(n * p.n_sectors, kPlBlock)), dim3(kPlBlock), 0, c->stream, (const uint32_t *)nullptr, n, p.n_rings,
                       p.n_sectors, d_desc, d_inv);
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

int check_query(dcreg_ctx *c, int nq, int64_t first, int64_t last, int k, const int32_t *idx, const int32_t *shift, const double *dist) {
    if (nq < 0) { c->fail("negative number of queries"); return DCREG_E_INVALID; }
    if (first < 0 || first > last || last > c->places.count) {
        c->fail("the range [%lld, %lld) is not inside the database's [0, %lld)", (long long)first, (long long)last, (long long)c->places.count);
        return DCREG_E_INVALID;
    }
    if (k < 1 || k > 64) { c->fail("k %d outside [1, 64]", k); return DCREG_E_INVALID; }
    if (nq > 0 && (!idx || !shift || !dist)) { c->fail("null result buffer"); return DCREG_E_INVALID; }
    return DCREG_OK;
}

// the search proper: nq query descriptors on the device (with their inverse norms) against the entries [first, last); waits for the stream
int search(dcreg_ctx *c, int nq, const float *d_q, const double *d_qinv, int64_t first, int64_t last, int k, int32_t *idx, int32_t *shift,
           double *dist) {
    dcreg_ctx::PlaceBufs &B = c->places;
    const int R = B.p.n_rings, S = B.p.n_sectors;
    const int64_t ne = last - first;
    for (int64_t i = 0; i < (int64_t)nq * k; ++i) { idx[i] = -1; shift[i] = 0; dist[i] = std::numeric_limits<double>::infinity(); }
    if (nq == 0 || ne == 0) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return DCREG_OK;
    }
    const int qb = (int)std::max<int64_t>(1, std::min<int64_t>(nq, kDistBatchPairs / ne));
    const int64_t chunks0 = (ne + kSelChunk - 1) / kSelChunk;
    if (B.dist.ensure(c, (size_t)qb * (size_t)ne) || B.shift.ensure(c, (size_t)qb * (size_t)ne) || B.sel_shift.ensure(c, (size_t)qb * k)) return DCREG_E_NOMEM;
    for (int s = 0; s < 2; ++s)
        if (B.sel_d[s].ensure(c, (size_t)qb * (size_t)chunks0 * k) || B.sel_i[s].ensure(c, (size_t)qb * (size_t)chunks0 * k)) return DCREG_E_NOMEM;
    for (int qa = 0; qa < nq; qa += qb) {
        const int nb = std::min(qb, nq - qa);
        const float *q = d_q + (size_t)qa * R * S;
        const double *qi = d_qinv + (size_t)qa * S;
        const dim3 grid(blocks(ne, kDistEntries), blocks(nb, kDistQueries));
        if (S <= 64)
            hipLaunchKernelGGL((k_place_dist<4, 4>), grid, dim3(64), 0, c->stream, q, qi, nb, B.desc.data(), B.inv.data(), first, ne, R, S, B.dist.data(),
                               B.shift.data());
        else
            hipLaunchKernelGGL((k_place_dist<8, 2>), grid, dim3(64), 0, c->stream, q, qi, nb, B.desc.data(), B.inv.data(), first, ne, R, S, B.dist.data(),
                               B.shift.data());
        // chunks of candidates until one is left: its k smallest are the result
        const double *in_d = B.dist.data();
        const int32_t *in_i = nullptr;
        int64_t n_in = ne;
        int side = 0;
        for (;;) {
            const int64_t chunks = (n_in + kSelChunk - 1) / kSelChunk;
            hipLaunchKernelGGL(k_place_select, dim3((unsigned)chunks, (unsigned)nb), dim3(kSelBlock), 0, c->stream, in_d, in_i, n_in, first, k,
                               B.sel_d[side].data(), B.sel_i[side].data(), chunks * k);
            in_d = B.sel_d[side].data();
            in_i = B.sel_i[side].data();
            n_in = chunks * k;
            side ^= 1;
            if (chunks == 1) break;
        }
        hipLaunchKernelGGL(k_place_gather, dim3(blocks((int64_t)nb * k, kPlBlock)), dim3(kPlBlock), 0, c->stream, in_i, (int64_t)nb * k, k, B.shift.data(),
                           first, ne, B.sel_shift.data());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(idx + (size_t)qa * k, in_i, sizeof(int32_t) * (size_t)nb * k, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(dist + (size_t)qa * k, in_d, sizeof(double) * (size_t)nb * k, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(shift + (size_t)qa * k, B.sel_shift.data(), sizeof(int32_t) * (size_t)nb * k, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

// what every entry point does first
int enter(dcreg_ctx *c) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return DCREG_OK;
}

int source_clouds(dcreg_ctx *c, CloudsIn &in, int64_t off[2]) {
    if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    off[0] = 0;
    off[1] = c->n_src;
    in.n_clouds = 1;
    in.off = off;
    in.from_source = true;
    return DCREG_OK;
}

int place_descriptors(dcreg_ctx *c, const CloudsIn &in, const dcreg_place_params *p, float *out, bool out_on_device, dcreg_place_info *info) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_params(c, p)) return rc;
    if (int rc = check_clouds(c, in.n_clouds, in.xyz, in.off, in.stride)) return rc;
    if (in.n_clouds > 0 && !out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    dcreg_ctx::PlaceBufs &B = c->places;
    const size_t bins = (size_t)p->n_rings * p->n_sectors, nd = (size_t)in.n_clouds;
    if (B.qinv.ensure(c, nd * p->n_sectors) || (!out_on_device && B.qdesc.ensure(c, nd * bins))) return DCREG_E_NOMEM;
    float *d_desc = out_on_device ? out : B.qdesc.data();
    unsigned long long cnt[2];
    if (int rc = describe(c, in, *p, d_desc, B.qinv.data(), cnt)) return rc;
    if (!out_on_device && nd) HIP_TRY(c, hipMemcpyAsync(out, d_desc, sizeof(float) * nd * bins, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    fill_info(info, in.n(), cnt);
    return DCREG_OK;
}

int places_add_clouds(dcreg_ctx *c, CloudsIn &in, dcreg_place_info *info) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    int64_t soff[2];
    if (in.from_source) {
        if (int rc = source_clouds(c, in, soff)) return rc;
    } else if (int rc = check_clouds(c, in.n_clouds, in.xyz, in.off, in.stride)) {
        return rc;
    }
    dcreg_ctx::PlaceBufs &B = c->places;
    if (int rc = grow_database(c, in.n_clouds)) return rc;
    const size_t bins = (size_t)B.p.n_rings * B.p.n_sectors;
    unsigned long long cnt[2];
    if (int rc = describe(c, in, B.p, B.desc.data() + (size_t)B.count * bins, B.inv.data() + (size_t)B.count * B.p.n_sectors, cnt)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    B.count += in.n_clouds;                  // (the new entries count only now: a failure above leaves the database as it was)
    fill_info(info, in.n(), cnt);
    return DCREG_OK;
}

int places_query_clouds(dcreg_ctx *c, CloudsIn &in, int64_t first, int64_t last, int k, int32_t *idx, int32_t *shift, double *dist,
                        dcreg_place_info *info) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    int64_t soff[2];
    if (in.from_source) {
        if (int rc = source_clouds(c, in, soff)) return rc;
    } else if (int rc = check_clouds(c, in.n_clouds, in.xyz, in.off, in.stride)) {
        return rc;
    }
    if (int rc = check_query(c, in.n_clouds, first, last, k, idx, shift, dist)) return rc;
    dcreg_ctx::PlaceBufs &B = c->places;
    const size_t bins = (size_t)B.p.n_rings * B.p.n_sectors, nd = (size_t)in.n_clouds;
    if (B.qdesc.ensure(c, nd * bins) || B.qinv.ensure(c, nd * B.p.n_sectors)) return DCREG_E_NOMEM;
    unsigned long long cnt[2];
    if (int rc = describe(c, in, B.p, B.qdesc.data(), B.qinv.data(), cnt)) return rc;
    if (int rc = search(c, in.n_clouds, B.qdesc.data(), B.qinv.data(), first, last, k, idx, shift, dist)) return rc;
    fill_info(info, in.n(), cnt);
    return DCREG_OK;
}

CloudsIn clouds_of(int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device) {
    CloudsIn in;
    in.n_clouds = n_clouds;
    in.xyz = xyz;
    in.off = off;
    in.stride = stride;
    in.on_device = on_device;
    return in;
}

}  // namespace
}  // namespace dcreg

using namespace dcreg;

extern "C" {

int dcreg_default_place_params(dcreg_place_params *p) {
    if (!p) return DCREG_E_INVALID;
    p->n_rings = 20;
    p->n_sectors = 60;
    p->max_range = 80.0;
    p->min_range = 0.0;
    p->z_offset = 2.0;
    return DCREG_OK;
}

int dcreg_place_descriptors(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_place_params *p,
                            float *desc_out, dcreg_place_info *info) {
    return place_descriptors(c, clouds_of(n_clouds, xyz, offsets, stride_floats, false), p, desc_out, false, info);
}
int dcreg_place_descriptors_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                   const dcreg_place_params *p, float *d_desc_out, dcreg_place_info *info) {
    return place_descriptors(c, clouds_of(n_clouds, d_xyz, offsets, stride_floats, true), p, d_desc_out, true, info);
}

int dcreg_places_reset(dcreg_ctx *c, const dcreg_place_params *p) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_params(c, p)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->places.p = *p;
    c->places.count = 0;
    c->places.ready = true;
    return DCREG_OK;
}

int64_t dcreg_places_count(const dcreg_ctx *c) { return c ? c->places.count : (int64_t)DCREG_E_INVALID; }

int dcreg_places_add(dcreg_ctx *c, int64_t n, const float *desc) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    dcreg_ctx::PlaceBufs &B = c->places;
    const size_t bins = (size_t)B.p.n_rings * B.p.n_sectors;
    if (n < 0 || (n > 0 && !desc)) { c->fail("invalid descriptor arguments"); return DCREG_E_INVALID; }
    if (!all_finite(desc, (size_t)n * bins)) { c->fail("a descriptor holds a value that is not finite"); return DCREG_E_INVALID; }
    if (n == 0) return DCREG_OK;
    if (int rc = grow_database(c, n)) return rc;
    float *tail = B.desc.data() + (size_t)B.count * bins;
    HIP_TRY(c, hipMemcpyAsync(tail, desc, sizeof(float) * (size_t)n * bins, hipMemcpyHostToDevice, c->stream));
    if (int rc = norms(c, tail, n, B.inv.data() + (size_t)B.count * B.p.n_sectors)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    B.count += n;
    return DCREG_OK;
}

int dcreg_places_add_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, dcreg_place_info *info) {
    CloudsIn in = clouds_of(n_clouds, xyz, offsets, stride_floats, false);
    return places_add_clouds(c, in, info);
}
int dcreg_places_add_clouds_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                   dcreg_place_info *info) {
    CloudsIn in = clouds_of(n_clouds, d_xyz, offsets, stride_floats, true);
    return places_add_clouds(c, in, info);
}
int dcreg_places_add_source(dcreg_ctx *c, dcreg_place_info *info) {
    CloudsIn in;
    in.from_source = true;
    return places_add_clouds(c, in, info);
}

int dcreg_places_get(dcreg_ctx *c, int64_t first, int64_t n, float *desc_out) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    dcreg_ctx::PlaceBufs &B = c->places;
    if (first < 0 || n < 0 || first > B.count || n > B.count - first) {
        c->fail("entries [%lld, %lld + %lld) are not inside the database's [0, %lld)", (long long)first, (long long)first, (long long)n, (long long)B.count);
        return DCREG_E_INVALID;
    }
    if (n == 0) return DCREG_OK;
    if (!desc_out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    const size_t bins = (size_t)B.p.n_rings * B.p.n_sectors;
    HIP_TRY(c, hipMemcpyAsync(desc_out, B.desc.data() + (size_t)first * bins, sizeof(float) * (size_t)n * bins, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

int dcreg_places_query(dcreg_ctx *c, int n_queries, const float *desc, int64_t first, int64_t last, int k, int32_t *idx, int32_t *shift, double *dist) {
    if (int rc = enter(c)) return rc;
    if (int rc = check_ready(c)) return rc;
    if (int rc = check_query(c, n_queries, first, last, k, idx, shift, dist)) return rc;
    dcreg_ctx::PlaceBufs &B = c->places;
    const size_t bins = (size_t)B.p.n_rings * B.p.n_sectors, nq = (size_t)n_queries;
    if (nq > 0 && !desc) { c->fail("null descriptor buffer"); return DCREG_E_INVALID; }
    if (!all_finite(desc, nq * bins)) { c->fail("a descriptor holds a value that is not finite"); return DCREG_E_INVALID; }
    if (B.qdesc.ensure(c, nq * bins) || B.qinv.ensure(c, nq * B.p.n_sectors)) return DCREG_E_NOMEM;
    if (nq) HIP_TRY(c, hipMemcpyAsync(B.qdesc.data(), desc, sizeof(float) * nq * bins, hipMemcpyHostToDevice, c->stream));
    if (int rc = norms(c, B.qdesc.data(), n_queries, B.qinv.data())) return rc;
    return search(c, n_queries, B.qdesc.data(), B.qinv.data(), first, last, k, idx, shift, dist);
}

int dcreg_places_query_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, int64_t first, int64_t last,
                              int k, int32_t *idx, int32_t *shift, double *dist, dcreg_place_info *info) {
    CloudsIn in = clouds_of(n_clouds, xyz, offsets, stride_floats, false);
    return places_query_clouds(c, in, first, last, k, idx, shift, dist, info);
}
int dcreg_places_query_clouds_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats, int64_t first,
                                     int64_t last, int k, int32_t *idx, int32_t *shift, double *dist, dcreg_place_info *info) {
    CloudsIn in = clouds_of(n_clouds, d_xyz, offsets, stride_floats, true);
    return places_query_clouds(c, in, first, last, k, idx, shift, dist, info);
}
int dcreg_places_query_source(dcreg_ctx *c, int64_t first, int64_t last, int k, int32_t *idx, int32_t *shift, double *dist, dcreg_place_info *info) {
    CloudsIn in;
    in.from_source = true;
    return places_query_clouds(c, in, first, last, k, idx, shift, dist, info);
}

}  // extern "C"
