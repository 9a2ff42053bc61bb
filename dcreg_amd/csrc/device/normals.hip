// Surface normals and curvature on the device (include/dcreg.h: dcreg_normals*, dcreg_target_normals*): pcl::NormalEstimation with a k
// search, with the rule of the header, bitwise the numpy reference of tests/normals_ref.py.
//   (cloud form)  the used (finite) points compacted with their input index in w and indexed: the shared first step of every pass over a
//                 cloud (scratch.hip cloud_index_used); the map form skips this - the map is its own index
//   k_nrm<K>      one lane per used point, in the index's cell order: the ring walk of k_knn with a heap of (d2, index) keys and positions in
//                 the last k of K slots; then the lane gathers its k neighbours in rank order (twice: the mean, the covariance - they are
//                 hot in L2), solves the 3x3 problem with six Jacobi sweeps in registers, orients the normal and writes 12 + 4 (+ 12) bytes
//                 at the point's input index
//   k_nrm_batch<K> the same body (nrm_point) for many clouds in ONE launch (dcreg_normals_clouds*, dcreg_frames_normals_keep): every cloud's
//                 used points behind a grid of its own, all grids built at once (context.hip clouds_index_build); a block serves one cloud;
//                 <K, true>: over the grids of a pairs' build batch, the outputs target after target (dcreg_pairs_normals_keep)
//   k_follow_*    the kept normals follow an update of the map ("normals_follow"): the cells of the points that came or went are marked,
//                 the map points whose reach touches a marked cell are compacted and go through k_nrm again, the rest is carried
// A point's result depends on the cloud only: the index decides how fast the neighbours are found, never which.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../../include/dcreg_debug.h"
#include "context.hpp"
#include "heap_nrm.hpp"
#include "jacobi.hpp"

// every multiply and add below rounds once: the rule is stated operation by operation
#pragma clang fp contract(off)

namespace dcreg {
namespace {

constexpr int kMinK = 3, kMaxK = 32;

struct NrmArgs {
    double vx, vy, vz;
    int orient;
};

// One lane per used point, in the index's cell order (the lanes of a wave search neighbouring cells); the point's input index is in w, and
// the outputs go there (a null output is not wanted).  cnt[0] += points with a normal, cnt[1] += sparse points (one atomic pair per wave)
// kept / reach (the map's kept normals, both or neither): {normal, curvature} - NaN for a sparse point - and the point's REACH, the squared
// distance within which a point that comes or goes can change its result: the k-th neighbour's d2, or the search bound when sparse
// (nrm_point: the body of one lane - k_nrm and k_nrm_batch below differ only in where the point, its grid and its counters come from)
template <int K>
DCREG_DEVFN void nrm_point(const float4 s4, const GridDev &g, RunList &rl, float bound_f, int max_ring, int k, const NrmArgs &a,
                           float *__restrict__ normal, float *__restrict__ curv, float *__restrict__ eig, float4 *__restrict__ kept,
                           float *__restrict__ reach, unsigned long long *__restrict__ cnt) {
    const uint32_t self = __float_as_uint(s4.w);
    HeapNrm<K> hp;
    hp.k = k;
    knn_search<HeapNrm<K>>(g, rl, s4.x, s4.y, s4.z, bound_f, max_ring, hp);
    const bool sparse = hp.pos[K - 1] == kNoIdx;       // (sorted: the last slot is the last to fill)
    if (!sparse) {
        const double px = (double)s4.x, py = (double)s4.y, pz = (double)s4.z;
        const double kd = (double)k;
        // (-0.0 is the identity of the IEEE addition: -0.0 + x = x bit for bit, so the sums start with their first term)
        double sx = -0.0, sy = -0.0, sz = -0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j >= K - k) {
                const float4 c = g.pts[hp.pos[j]];
                sx = sx + ((double)c.x - px); sy = sy + ((double)c.y - py); sz = sz + ((double)c.z - pz);
            }
        const double mx = sx / kd, my = sy / kd, mz = sz / kd;
        double cxx = -0.0, cxy = -0.0, cxz = -0.0, cyy = -0.0, cyz = -0.0, czz = -0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j >= K - k) {
                const float4 c = g.pts[hp.pos[j]];
                const double dx = ((double)c.x - px) - mx, dy = ((double)c.y - py) - my, dz = ((double)c.z - pz) - mz;
                cxx = cxx + dx * dx; cxy = cxy + dx * dy; cxz = cxz + dx * dz;
                cyy = cyy + dy * dy; cyz = cyz + dy * dz; czz = czz + dz * dz;
            }
        double a00 = cxx / kd, a01 = cxy / kd, a02 = cxz / kd, a11 = cyy / kd, a12 = cyz / kd, a22 = czz / kd;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int sweep = 0; sweep < 6; ++sweep) {
            jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0,1), r = 2
            jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0,2), r = 1
            jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1,2), r = 0
        }
        // the smallest eigenvalue, a tie to the lowest index
        const bool b1 = a11 < a00;
        const double l01 = b1 ? a11 : a00;
        const bool b2 = a22 < l01;
        const double lmin = b2 ? a22 : l01;
        double nx = b2 ? v02 : (b1 ? v01 : v00), ny = b2 ? v12 : (b1 ? v11 : v10), nz = b2 ? v22 : (b1 ? v21 : v20);
        const double trace = (a00 + a11) + a22;
        const double cv = trace == 0.0 ? 0.0 : fabs(lmin) / trace;
        if (a.orient == DCREG_NORMAL_ORIENT_VIEWPOINT) {
            const double dot = ((a.vx - px) * nx + (a.vy - py) * ny) + (a.vz - pz) * nz;
            if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
        }
        if (normal) { normal[3 * (size_t)self] = (float)nx; normal[3 * (size_t)self + 1] = (float)ny; normal[3 * (size_t)self + 2] = (float)nz; }
        if (curv) curv[self] = (float)cv;
        if (kept) { kept[self] = float4{(float)nx, (float)ny, (float)nz, (float)cv}; reach[self] = hp.worst_d2(); }
        if (eig) {
            double l0 = a00, l1 = a11, l2 = a22, t;
            if (l1 < l0) { t = l0; l0 = l1; l1 = t; }
            if (l2 < l1) { t = l1; l1 = l2; l2 = t; }
            if (l1 < l0) { t = l0; l0 = l1; l1 = t; }
            eig[3 * (size_t)self] = (float)l0; eig[3 * (size_t)self + 1] = (float)l1; eig[3 * (size_t)self + 2] = (float)l2;
        }
    } else if (kept) {
        const float nan_ = __builtin_nanf("");
        kept[self] = float4{nan_, nan_, nan_, nan_};
        reach[self] = bound_f;
    }
    const unsigned long long A = __ballot(true), S = __ballot(sparse);
    if ((int)(threadIdx.x & 63) == __ffsll(A) - 1) {
        const unsigned long long ns = (unsigned long long)__popcll(S);
        atomicAdd(cnt, (unsigned long long)__popcll(A) - ns);
        if (ns) atomicAdd(cnt + 1, ns);
    }
}

template <int K>
static __global__ __launch_bounds__(kBlock) void k_nrm(const float4 *__restrict__ q, uint32_t n, GridDev g, float bound_f, int max_ring, int k,
                                                       NrmArgs a, float *__restrict__ normal, float *__restrict__ curv, float *__restrict__ eig,
                                                       float4 *__restrict__ kept, float *__restrict__ reach,
                                                       unsigned long long *__restrict__ cnt) {
    __shared__ RunList runs[kBlock / kWave];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    nrm_point<K>(q[i], g, runs[threadIdx.x / kWave], bound_f, max_ring, k, a, normal, curv, eig, kept, reach, cnt);
}

// ---- many clouds in one launch (dcreg_normals_clouds*, dcreg_frames_normals_keep).  Every indexed cloud has a record - its own grid (the
// cloud's used points in its cell order are the grid's points: w = the point's index in the call's input), the rings that cover the search
// bound in its cells (-1: unbounded) and its place in the call - and as many blocks as its points need: block b is block blk[b].y of record
// blk[b].x, so a block never straddles two clouds and reads its grid through a block-uniform index.  Outputs at the point's input index;
// the counts of record r's cloud at cnt[2 cloud], cnt[2 cloud + 1].  base (read by the BASE instantiations only): added to the output index
// of every point of the record - 0 where w is the index in the call's input; the pair targets' grids carry w = the index within the own
// cloud (k_pairs_pack), and base is the target's first point in the batch (pairs_normals_keep)
struct NrmCloud {
    GridDev g;
    int max_ring;
    uint32_t cloud;
    uint32_t base;
};
template <int K, bool BASE = false>
static __global__ __launch_bounds__(kBlock) void k_nrm_batch(const NrmCloud *__restrict__ clouds, const uint2 *__restrict__ blk, float bound_f, int k,
                                                             NrmArgs a, float *__restrict__ normal, float *__restrict__ curv,
                                                             unsigned long long *__restrict__ cnt) {
    __shared__ RunList runs[kBlock / kWave];
    const uint2 b = blk[blockIdx.x];
    const NrmCloud &C = clouds[b.x];
    const GridDev g = C.g;
    const uint32_t i = b.y * kBlock + threadIdx.x;
    if (i >= g.n_pts) return;
    float4 s4 = g.pts[i];
    // (BASE: the record's base is added to the output index - nothing else reads w; without it the kernel is the one of the two callers
    // whose records carry base 0, register for register)
    if constexpr (BASE) s4.w = __uint_as_float(__float_as_uint(s4.w) + C.base);
    nrm_point<K>(s4, g, runs[threadIdx.x / kWave], bound_f, C.max_ring, k, a, normal, curv, nullptr, nullptr, nullptr, cnt + 2 * (size_t)C.cloud);
}

// the bounds of every cloud's used points (ordered floats: bounds[3 s + a] minima, bounds[3 n_clouds + 3 s + a] maxima, as k_pairs_pack
// leaves a target's) - six atomics per wave where the wave's used points belong to one cloud, per lane across a boundary
static __global__ __launch_bounds__(256) void k_ncl_bounds(const float4 *__restrict__ pts, int64_t n, const uint32_t *__restrict__ used,
                                                          const int64_t *__restrict__ off, int n_clouds, uint32_t *__restrict__ bounds) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n && used[i] != 0u;
    const uint32_t s = live ? seg_of(off, n_clouds, i) : 0u;
    float v[3] = {0.f, 0.f, 0.f};
    if (live) { const float4 p = pts[i]; v[0] = p.x; v[1] = p.y; v[2] = p.z; }
    const unsigned long long lanes = __ballot(live);
    if (lanes == 0ull) return;
    const uint32_t s0 = (uint32_t)__shfl((int)s, __ffsll(lanes) - 1);
    if (__ballot(live && s == s0) == lanes) {
        float mn[3], mx[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = live ? v[a] : 3.4e38f; mx[a] = live ? v[a] : -3.4e38f;
            for (int o = 32; o > 0; o >>= 1) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], o)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o)); }
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { atomicMin(&bounds[3 * s0 + a], f2ord(mn[a])); atomicMax(&bounds[3 * n_clouds + 3 * s0 + a], f2ord(mx[a])); }
        }
    } else if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(&bounds[3 * s + a], f2ord(v[a])); atomicMax(&bounds[3 * n_clouds + 3 * s + a], f2ord(v[a])); }
    }
}
// starts[s] = the used points in front of cloud s (n_clouds + 1 entries: upos has n + 1)
static __global__ void k_ncl_starts(const uint32_t *__restrict__ upos, const int64_t *__restrict__ off, int n_clouds, uint32_t *__restrict__ starts) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= n_clouds) starts[s] = upos[off[s]];
}
// the kept normals of loaded frames: position p of the frames' curve-ordered points (frame f from dst[f], every frame padded to a query
// block; w = the point's index within its frame) takes the normal (3 floats, `stride` apart) and curvature (null: NaN) of upload point
// off[f] + w -> float4 p; the padding gets NaN
static __global__ void k_nrm_pack_frames(const float4 *__restrict__ src, int64_t n_padded, const uint32_t *__restrict__ dst, const int64_t *__restrict__ off,
                                         int n_frames, const float *__restrict__ normal, int64_t stride, const float *__restrict__ curv,
                                         float4 *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_padded) return;
    int lo = 0, hi = n_frames - 1;                       // the last frame that starts at or before p (empty frames share a start)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)dst[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int64_t local = p - (int64_t)dst[lo];
    const float nan_ = __builtin_nanf("");
    float4 v = float4{nan_, nan_, nan_, nan_};
    if (local < off[lo + 1] - off[lo]) {
        const size_t oi = (size_t)(off[lo] + (int64_t)__float_as_uint(src[p].w));
        const float *q = normal + oi * (size_t)stride;
        v = float4{q[0], q[1], q[2], curv ? curv[oi] : nan_};
    }
    out[p] = v;
}

// the kept form: normal (3 floats, `stride` apart) and curvature (null: NaN) of point i -> float4 i
static __global__ void k_nrm_pack(const float *__restrict__ normal, int64_t stride, const float *__restrict__ curv, int64_t n, float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = normal + (size_t)i * (size_t)stride;
    out[i] = float4{p[0], p[1], p[2], curv ? curv[i] : __builtin_nanf("")};
}

// the kept SOURCE normals: lane i takes the normal (3 floats, `stride` apart) and curvature (null: NaN) of the point that sits at
// position i of the context's curve order (its original index rides in src[i].w) -> float4 i; and back: float4 i -> original order
static __global__ void k_nrm_pack_src(const float4 *__restrict__ src, int64_t n, const float *__restrict__ normal, int64_t stride,
                                      const float *__restrict__ curv, float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t oi = __float_as_uint(src[i].w);
    const float *p = normal + oi * (size_t)stride;
    out[i] = float4{p[0], p[1], p[2], curv ? curv[oi] : __builtin_nanf("")};
}
// ... and the kept normals of loaded frames back in upload order (the inverse of k_nrm_pack_frames; the padding is skipped)
static __global__ void k_nrm_unpack_frames(const float4 *__restrict__ src, int64_t n_padded, const uint32_t *__restrict__ dst, const int64_t *__restrict__ off,
                                           int n_frames, const float4 *__restrict__ kept, float4 *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_padded) return;
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)dst[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int64_t local = p - (int64_t)dst[lo];
    if (local < off[lo + 1] - off[lo]) out[(size_t)(off[lo] + (int64_t)__float_as_uint(src[p].w))] = kept[p];
}
static __global__ void k_nrm_unpack_src(const float4 *__restrict__ src, int64_t n, const float4 *__restrict__ kept, float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[__float_as_uint(src[i].w)] = kept[i];
}

template <int K>
void launch_nrm(dcreg_ctx *c, const float4 *q, int64_t nq, const GridDev &g, float bound, int max_ring, int k, const NrmArgs &a, float *normal,
                float *curv, float *eig, float4 *kept = nullptr, float *reach = nullptr) {
    hipLaunchKernelGGL(k_nrm<K>, dim3(blocks(nq, kBlock)), dim3(kBlock), 0, c->stream, q, (uint32_t)nq, g, bound, max_ring, k, a, normal, curv, eig,
                       kept, reach, c->nrm.cnt.data());
}
// the search of a parameter set in a grid, and the launch of the instantiation its k takes
struct NrmSearch { float bound; int max_ring; NrmArgs a; };
NrmSearch nrm_search(const dcreg_normal_params *p, const GridDev *g) {       // (g null: the bound and the arguments, no grid yet, max_ring -1)
    const SearchBound b = search_bound(p->search_radius, g);
    NrmSearch s{b.bound, b.max_ring, {}};
    s.a.vx = p->viewpoint[0]; s.a.vy = p->viewpoint[1]; s.a.vz = p->viewpoint[2]; s.a.orient = p->orient;
    return s;
}
void launch_nrm_k(dcreg_ctx *c, const float4 *q, int64_t nq, const GridDev &g, const dcreg_normal_params *p, float *normal, float *curv, float *eig,
                  float4 *kept, float *reach) {
    const NrmSearch s = nrm_search(p, &g);
    with_heap_k(p->k, [&](auto K) { launch_nrm<decltype(K)::value>(c, q, nq, g, s.bound, s.max_ring, p->k, s.a, normal, curv, eig, kept, reach); });
}

}  // namespace

int normals_check(dcreg_ctx *c, const dcreg_normal_params *p) {
    if (!p) { c->fail("null normal parameters"); return DCREG_E_INVALID; }
    if (p->k < kMinK || p->k > kMaxK) { c->fail("normal k is %d: %d .. %d expected", p->k, kMinK, kMaxK); return DCREG_E_INVALID; }
    if (p->orient != DCREG_NORMAL_ORIENT_VIEWPOINT && p->orient != DCREG_NORMAL_ORIENT_NONE) { c->fail("unknown normal orientation %d", p->orient); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->search_radius) && p->search_radius >= 0.0)) { c->fail("normal search_radius is %g: finite and >= 0 expected", p->search_radius); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->viewpoint[0]) && std::isfinite(p->viewpoint[1]) && std::isfinite(p->viewpoint[2]))) { c->fail("the normal viewpoint is not finite"); return DCREG_E_INVALID; }
    return DCREG_OK;
}

namespace {

struct NormalOut {
    float *normal, *curv, *eig;       // the caller's buffers (null: not wanted)
    bool on_device;
    bool keep = false;                // normal and curvature go to the context's kept normals instead (nothing is copied out)
    bool scratch = false;             // normal and curvature are computed into the call's scratch (c->nrm) and stay there for the caller
};

// The outputs of n points start as NaN; the nq used points at q (cell order, w = the output index) behind the grid g get theirs; then the
// copies to the caller and the counts.  nq = 0: no index was built (fewer than k of the n_used used points) - every used point is sparse
int normals_run(dcreg_ctx *c, const float4 *q, int64_t nq, const GridDev &g, int64_t n, int64_t n_used, const dcreg_normal_params *p, const NormalOut &o,
                dcreg_normal_info *info) {
    dcreg_ctx::NormalBufs &B = c->nrm;
    // (keep: the kernel writes the kept normals and their reaches itself, at every point of the map - nq == n there)
    const bool want_n = o.normal != nullptr || o.scratch, want_c = o.curv != nullptr || o.scratch;
    if (o.keep && nq != n) { c->fail("kept normals need the map's own index"); return DCREG_E_STATE; }
    if ((want_n && B.normal.ensure(c, 3 * (size_t)n)) || (want_c && B.curv.ensure(c, (size_t)n)) || (o.eig && B.eig.ensure(c, 3 * (size_t)n)) ||
        B.cnt.ensure(c, 2) || (o.keep && (c->nicp.normals.ensure(c, (size_t)n) || c->nicp.reach.ensure(c, (size_t)n))))
        return DCREG_E_NOMEM;
    float *d_normal = want_n ? B.normal.data() : nullptr, *d_curv = want_c ? B.curv.data() : nullptr, *d_eig = o.eig ? B.eig.data() : nullptr;
    const float nanf_ = __builtin_nanf("");
    if (d_normal) fill_f32(c, d_normal, 3 * n, nanf_);
    if (d_curv) fill_f32(c, d_curv, n, nanf_);
    if (d_eig) fill_f32(c, d_eig, 3 * n, nanf_);
    HIP_TRY(c, hipMemsetAsync(B.cnt.data(), 0, 2 * sizeof(unsigned long long), c->stream));
    unsigned long long cnt[2] = {0, (unsigned long long)n_used};
    if (nq > 0) {
        launch_nrm_k(c, q, nq, g, p, d_normal, d_curv, d_eig, o.keep ? c->nicp.normals.data() : nullptr, o.keep ? c->nicp.reach.data() : nullptr);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(cnt, B.cnt.data(), sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    }
    if (o.normal) if (int rc = caller_out(c, o.normal, d_normal, sizeof(float) * 3 * (size_t)n, o.on_device)) return rc;
    if (o.curv) if (int rc = caller_out(c, o.curv, d_curv, sizeof(float) * (size_t)n, o.on_device)) return rc;
    if (o.eig) if (int rc = caller_out(c, o.eig, d_eig, sizeof(float) * 3 * (size_t)n, o.on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (info) { info->n_in = n; info->n_finite = n_used; info->n_sparse = (int64_t)cnt[1]; info->n_out = (int64_t)cnt[0]; }
    return DCREG_OK;
}

// dcreg_normals*: the cloud packed, its used points indexed, the kernel, the copies
int normals_cloud(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, const dcreg_normal_params *p, float *normal, float *curv,
                  float *eig, dcreg_normal_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = normals_check(c, p)) return rc;
    if (n < 0 || stride < 3) { c->fail("invalid normal estimation arguments"); return DCREG_E_INVALID; }
    if (n > (int64_t)INT32_MAX) { c->fail("too many points for one normal estimation (%lld)", (long long)n); return DCREG_E_INVALID; }
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    if (!normal && !curv && !eig) { c->fail("no output buffer: normals, curvature or eigenvalues expected"); return DCREG_E_INVALID; }
    if (info) std::memset(info, 0, sizeof(*info));
    if (n == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::CloudScratch &B = c->cloud;
    if (int rc = upload_cloud(c, xyz, n, stride, on_device, B.pts)) return rc;
    int64_t n_used = 0;
    if (int rc = cloud_index_used(c, B.pts.data(), n, p->search_radius, p->k, &n_used)) return rc;
    const bool indexed = n_used >= p->k;
    const NormalOut o{normal, curv, eig, on_device};
    return normals_run(c, indexed ? B.idx.sorted.data() : nullptr, indexed ? n_used : 0, indexed ? B.idx.grid : GridDev{}, n, n_used, p, o, info);
}

// ------------------------------------------------------------------------------------------ many clouds in one call
// The n packed points at `in` (input order, w = the index; on the device) are n_clouds clouds, cloud s = [off[s], off[s + 1]) (host memory,
// checked by the caller).  ONE used / scan / compaction pass and ONE bounds pass over all of them, ONE readback of every cloud's bounds
// and used count; the clouds with at least k used points are indexed together (clouds_index_build: one sort per pass), the others get
// no grid and come out all sparse; then ONE upload of the launch's records, ONE k_nrm_batch and ONE readback of the counts.  Leaves the
// normals (3 n floats) and curvatures (n floats) in c->nrm.normal / curv - NaN where a point has none - with the work queued on the
// stream and waited for; infos (may be null): one record per cloud, as dcreg_normals fills it.
int normals_clouds_run(dcreg_ctx *c, const float4 *in, int64_t n, int n_clouds, const int64_t *off, const dcreg_normal_params *p,
                       dcreg_normal_info *infos) {
    dcreg_ctx::NormalBufs &B = c->nrm;
    const size_t nc = (size_t)n_clouds;
    if (B.normal.ensure(c, 3 * (size_t)n) || B.curv.ensure(c, (size_t)n) || B.cnt.ensure(c, 2 * nc) || B.d_off.ensure(c, nc + 1) ||
        B.d_words.ensure(c, 7 * nc + 1))
        return DCREG_E_NOMEM;
    const float nanf_ = __builtin_nanf("");
    fill_f32(c, B.normal.data(), 3 * n, nanf_);
    fill_f32(c, B.curv.data(), n, nanf_);
    HIP_TRY(c, hipMemsetAsync(B.cnt.data(), 0, 2 * nc * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemcpyAsync(B.d_off.data(), off, sizeof(int64_t) * (nc + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(B.d_words.data(), 0xFF, sizeof(uint32_t) * 3 * nc, c->stream));
    HIP_TRY(c, hipMemsetAsync(B.d_words.data() + 3 * nc, 0, sizeof(uint32_t) * 3 * nc, c->stream));
    if (int rc = cloud_used_compact(c, in, n)) return rc;
    hipLaunchKernelGGL(k_ncl_bounds, dim3(blocks(n, 256)), dim3(256), 0, c->stream, in, n, c->cloud.used.data(), B.d_off.data(), n_clouds, B.d_words.data());
    hipLaunchKernelGGL(k_ncl_starts, dim3(blocks((int64_t)nc + 1, 256)), dim3(256), 0, c->stream, c->cloud.upos.data(), B.d_off.data(), n_clouds,
                       B.d_words.data() + 6 * nc);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> words(7 * nc + 1);
    HIP_TRY(c, hipMemcpyAsync(words.data(), B.d_words.data(), sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const uint32_t *starts = words.data() + 6 * nc;
    std::vector<int64_t> used(nc), count(nc), first(nc);
    bool any = false;
    for (size_t s = 0; s < nc; ++s) {
        used[s] = (int64_t)starts[s + 1] - (int64_t)starts[s];
        count[s] = used[s] >= p->k ? used[s] : 0;             // (fewer than k used points: no index, all sparse - as the single call)
        first[s] = (int64_t)starts[s];
        any = any || count[s] > 0;
    }
    std::vector<unsigned long long> cnt(2 * nc, 0ull);
    if (any) {
        std::vector<GridDev> grids;
        std::vector<uint8_t> built;
        words.resize(6 * nc);
        // (the table budget of a pair target, and at most 2^22 entries a cloud: the clouds of a call share the device)
        const double max_cells = (double)std::min<int64_t>(c->opt_pair_max_table_entries, (int64_t)1 << 22);
        if (int rc = clouds_index_build(c, B.clouds, c->cloud.cpts.data(), n_clouds, count, first, words, p->search_radius, max_cells, grids, built)) return rc;
        const NrmSearch sr = nrm_search(p, nullptr);             // (the rings are counted per grid below)
        std::vector<NrmCloud> recs;
        std::vector<uint2> blk;
        for (size_t s = 0; s < nc; ++s) {
            if (!built[s]) continue;
            NrmCloud r;
            r.g = grids[s];
            r.max_ring = p->search_radius > 0.0 ? rings_for_bound(grids[s], sr.bound) : -1;
            r.cloud = (uint32_t)s;
            r.base = 0u;
            const uint32_t nb = blocks(count[s], kBlock);
            for (uint32_t b = 0; b < nb; ++b) blk.push_back(make_uint2((uint32_t)recs.size(), b));
            recs.push_back(r);
        }
        const size_t rec_bytes = recs.size() * sizeof(NrmCloud), bytes = rec_bytes + blk.size() * sizeof(uint2);
        std::vector<unsigned char> h(bytes);
        std::memcpy(h.data(), recs.data(), rec_bytes);
        std::memcpy(h.data() + rec_bytes, blk.data(), blk.size() * sizeof(uint2));
        if (B.d_launch.ensure(c, bytes)) return DCREG_E_NOMEM;
        HIP_TRY(c, hipMemcpyAsync(B.d_launch.data(), h.data(), bytes, hipMemcpyHostToDevice, c->stream));
        const NrmCloud *d_recs = (const NrmCloud *)B.d_launch.data();
        const uint2 *d_blk = (const uint2 *)(B.d_launch.data() + rec_bytes);
        const dim3 grid((unsigned)blk.size()), block(kBlock);
        const int k = p->k;
        with_heap_k(k, [&](auto K) { hipLaunchKernelGGL(k_nrm_batch<decltype(K)::value>, grid, block, 0, c->stream, d_recs, d_blk, sr.bound, k, sr.a, B.normal.data(), B.curv.data(), B.cnt.data()); });
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(cnt.data(), B.cnt.data(), sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // (h, recs and blk are the sources of the upload)
        HIP_TRY(c, hipGetLastError());
    }
    if (infos)
        for (size_t s = 0; s < nc; ++s) {
            infos[s].n_in = off[s + 1] - off[s]; infos[s].n_finite = used[s];
            infos[s].n_sparse = count[s] > 0 ? (int64_t)cnt[2 * s + 1] : used[s];
            infos[s].n_out = count[s] > 0 ? (int64_t)cnt[2 * s] : 0;
        }
    return DCREG_OK;
}

// the offset rules of dcreg_voxel_downsample, and the size of one call
int clouds_check(dcreg_ctx *c, int n_clouds, const int64_t *off) {
    if (n_clouds < 0) { c->fail("negative cloud count"); return DCREG_E_INVALID; }
    if (n_clouds > 0 && !off) { c->fail("null cloud offsets"); return DCREG_E_INVALID; }
    if (n_clouds > 0 && off[0] != 0) { c->fail("cloud offsets must start at 0"); return DCREG_E_INVALID; }
    for (int s = 0; s < n_clouds; ++s)
        if (off[s + 1] < off[s]) { c->fail("cloud offsets decrease at cloud %d", s); return DCREG_E_INVALID; }
    if (n_clouds > 0 && off[n_clouds] > (int64_t)INT32_MAX) { c->fail("too many points for one normal estimation (%lld)", (long long)off[n_clouds]); return DCREG_E_INVALID; }
    return DCREG_OK;
}

// dcreg_normals_clouds*: the clouds packed in one upload, the pass above, the copies to the caller
int normals_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device, const dcreg_normal_params *p,
                   float *normal, float *curv, dcreg_normal_info *infos) {
    if (!c) return DCREG_E_INVALID;
    // (the arguments first, then the context's state: a call without clouds or without points queues nothing and asks for no state)
    if (int rc = normals_check(c, p)) return rc;
    if (stride < 3) { c->fail("invalid normal estimation arguments"); return DCREG_E_INVALID; }
    if (int rc = clouds_check(c, n_clouds, off)) return rc;
    if (!normal && !curv) { c->fail("no output buffer: normals or curvature expected"); return DCREG_E_INVALID; }
    if (n_clouds == 0) return DCREG_OK;
    const int64_t n = off[n_clouds];
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    if (n > 0) if (int rc = refuse_in_flight(c)) return rc;
    if (infos) std::memset(infos, 0, sizeof(*infos) * (size_t)n_clouds);
    if (n == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = upload_cloud(c, xyz, n, stride, on_device, c->cloud.pts)) return rc;
    if (int rc = normals_clouds_run(c, c->cloud.pts.data(), n, n_clouds, off, p, infos)) return rc;
    if (normal) if (int rc = caller_out(c, normal, c->nrm.normal.data(), sizeof(float) * 3 * (size_t)n, on_device)) return rc;
    if (curv) if (int rc = caller_out(c, curv, c->nrm.curv.data(), sizeof(float) * (size_t)n, on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

// the loaded frames' host offsets (FrameSet keeps the slices) and the padded length of their curve-ordered points
int64_t frames_offsets(const dcreg_ctx::FrameSet &fs, std::vector<int64_t> &off) {
    off.assign(fs.slice.size() + 1, 0);
    int64_t padded = 0;
    for (size_t f = 0; f < fs.slice.size(); ++f) {
        off[f + 1] = off[f] + (int64_t)fs.slice[f].y;
        padded = (int64_t)fs.slice[f].x + ((int64_t)fs.slice[f].y + kLinBlock - 1) / kLinBlock * kLinBlock;
    }
    return padded;
}

// dcreg_frames_normals_keep: the pass above over the loaded frames in upload order (FrameSet::raw is what upload_cloud packs for
// dcreg_normals_clouds: the same points, the same build, the same kernel), then one gather into every frame's curve order
// (fs: the context's frames, or the sources of the pairs' calls - dcreg_pairs_sources_normals_keep)
const char *no_frames_msg(const dcreg_ctx *c, const dcreg_ctx::FrameSet &fs) {
    return &fs == &c->pair_src ? "no pair sources: dcreg_pairs_sources_load first" : "no frames: dcreg_frames_load first";
}
int frames_normals_keep(dcreg_ctx *c, dcreg_ctx::FrameSet &fs, const dcreg_normal_params *p, dcreg_normal_info *infos) {
    if (int rc = normals_check(c, p)) return rc;
    if (int rc = refuse_in_flight(c)) return rc;
    if (fs.slice.empty()) { c->fail("%s", no_frames_msg(c, fs)); return DCREG_E_STATE; }
    std::vector<int64_t> off;
    const int64_t padded = frames_offsets(fs, off), n = off.back();
    const int n_frames = (int)fs.slice.size();
    if (infos) std::memset(infos, 0, sizeof(*infos) * (size_t)n_frames);
    HIP_TRY(c, hipSetDevice(c->device));
    fs.normals_kept = false;                                    // (a failed call leaves none)
    if (n > 0) {
        if (fs.normals.ensure(c, (size_t)padded)) return DCREG_E_NOMEM;
        if (int rc = normals_clouds_run(c, fs.raw.data(), n, n_frames, off.data(), p, infos)) return rc;
        hipLaunchKernelGGL(k_nrm_pack_frames, dim3(blocks(padded, 256)), dim3(256), 0, c->stream, fs.src.data(), padded, fs.d_dst.data(), fs.d_off.data(),
                           n_frames, c->nrm.normal.data(), (int64_t)3, c->nrm.curv.data(), fs.normals.data());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    fs.normals_kept = true;
    return DCREG_OK;
}

// ------------------------------------------------------------------------------------------ kept normals given and read back
// The four holders of kept normals (the map, the source, a frame set, the pair targets) share what their set and get forms do behind the
// holder's own refusals, whose order each entry point keeps.  kept_args / kept_count / kept_capacity: the refusals with a common text
// (`holds`: "the map holds", ...).  kept_take: the holder's array sized, the caller's n rows staged in c->d_stage or ordered
// (caller_rows), `pack` queues the holder's kernel over them, the wait.  kept_give: n records from `from` to the caller, the wait.
int kept_args(dcreg_ctx *c, const float *normals, int64_t stride) {
    if (!normals || stride < 3) { c->fail("invalid kept-normal arguments"); return DCREG_E_INVALID; }
    return DCREG_OK;
}
int kept_count(dcreg_ctx *c, const char *holds, int64_t n, int64_t n_given) {
    if (n_given != n) { c->fail("%s %lld points, %lld normals were given", holds, (long long)n, (long long)n_given); return DCREG_E_INVALID; }
    return DCREG_OK;
}
int kept_capacity(dcreg_ctx *c, const char *holds, int64_t n, int64_t capacity) {
    if (capacity < n) { c->fail("%s %lld points, the capacity is %lld", holds, (long long)n, (long long)capacity); return DCREG_E_INVALID; }
    return DCREG_OK;
}
template <class Pack>
int kept_take(dcreg_ctx *c, const float *normals, int64_t n, int64_t stride, bool on_device, DevBuf<float4> &kept, int64_t kept_len, Pack pack) {
    const float *src = nullptr;
    if (kept.ensure(c, (size_t)kept_len)) return DCREG_E_NOMEM;
    if (int rc = caller_rows(c, normals, n, stride, 3, on_device, c->d_stage, &src)) return rc;
    pack(src);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}
int kept_give(dcreg_ctx *c, float *out, const float4 *from, int64_t n, bool on_device) {
    if (int rc = caller_out(c, out, from, sizeof(float4) * (size_t)n, on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

// dcreg_frames_normals_set: the caller's normals in the upload order of the load become the frames' kept normals, as given
int frames_normals_set(dcreg_ctx *c, dcreg_ctx::FrameSet &fs, const float *normals, int64_t n_given, int64_t stride) {
    if (int rc = kept_args(c, normals, stride)) return rc;
    if (int rc = refuse_in_flight(c)) return rc;
    if (fs.slice.empty()) { c->fail("%s", no_frames_msg(c, fs)); return DCREG_E_STATE; }
    std::vector<int64_t> off;
    const int64_t padded = frames_offsets(fs, off), n = off.back();
    if (int rc = kept_count(c, "the frames hold", n, n_given)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    fs.normals_kept = false;
    if (n > 0)
        if (int rc = kept_take(c, normals, n, stride, false, fs.normals, padded, [&](const float *src) {
                hipLaunchKernelGGL(k_nrm_pack_frames, dim3(blocks(padded, 256)), dim3(256), 0, c->stream, fs.src.data(), padded, fs.d_dst.data(),
                                   fs.d_off.data(), (int)fs.slice.size(), src, stride, (const float *)nullptr, fs.normals.data());
            }))
            return rc;
    fs.normals_kept = true;
    return DCREG_OK;
}

// the kept normals of a frame set in the upload order of its load, 4 floats per point (the pairs' sources: dcreg_pairs_sources_normals_get)
int frames_normals_get(dcreg_ctx *c, dcreg_ctx::FrameSet &fs, float *out, int64_t capacity) {
    if (int rc = refuse_in_flight(c)) return rc;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (fs.slice.empty() || !fs.normals_kept) { c->fail("no kept normals of these clouds"); return DCREG_E_STATE; }
    std::vector<int64_t> off;
    const int64_t padded = frames_offsets(fs, off), n = off.back();
    if (int rc = kept_capacity(c, "the clouds hold", n, capacity)) return rc;
    if (n == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->gicp.tmp.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_nrm_unpack_frames, dim3(blocks(padded, 256)), dim3(256), 0, c->stream, fs.src.data(), padded, fs.d_dst.data(), fs.d_off.data(),
                       (int)fs.slice.size(), fs.normals.data(), c->gicp.tmp.data());
    HIP_TRY(c, hipGetLastError());
    return kept_give(c, out, c->gicp.tmp.data(), n, false);
}

// ------------------------------------------------------------------------------------------ the targets of a pairs' build batch
// The record the batched 1-NN launches read per target (context.hpp OneNnGrid): its grid, the rings of the 1-NN bound at the radius the
// batch was built for, the start of its kept normals.  Uploaded behind every keep / set; waits for the stream.
int pairs_nn_grids(dcreg_ctx *c) {
    dcreg_ctx::PairSet &ps = c->pairs;
    const size_t nt = (size_t)ps.n;
    std::vector<OneNnGrid> recs(nt);
    std::memset(recs.data(), 0, sizeof(OneNnGrid) * nt);
    for (size_t t = 0; t < nt; ++t) {
        if (!ps.built[t]) continue;
        recs[t].g = ps.grids[t];
        recs[t].max_ring = one_nn_bound(ps.grids[t], ps.search_radius).max_ring;
        recs[t].normals_first = (uint32_t)ps.off[t];
    }
    if (ps.d_nn_grids.ensure(c, nt)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemcpyAsync(ps.d_nn_grids.data(), recs.data(), sizeof(OneNnGrid) * nt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}
int pairs_batch_check(dcreg_ctx *c) {
    if (int rc = refuse_in_flight(c)) return rc;
    if (c->pairs.n <= 0 || c->pairs.off.size() != (size_t)c->pairs.n + 1) { c->fail("no pair batch built: dcreg_pairs_build first"); return DCREG_E_STATE; }
    return DCREG_OK;
}

// dcreg_pairs_normals_keep: the kept normals of every target of the build batch, in ONE launch of k_nrm_batch over the grids the batch
// already has - no second index, no second sort.  A grid's points carry w = the index within their own target, so every record adds the
// target's first point (NrmCloud::base): the outputs land target after target, each in its own index order.  A target with fewer than k
// points gets no record and keeps the NaN the outputs start with, as a cloud of normals_clouds_run; the rings per grid, -1 unbounded.
// The searches are exact in any cells: target t's values are bitwise dcreg_normals of that target alone.
int pairs_normals_keep(dcreg_ctx *c, const dcreg_normal_params *p, dcreg_normal_info *infos) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = normals_check(c, p)) return rc;
    if (int rc = pairs_batch_check(c)) return rc;
    dcreg_ctx::PairSet &ps = c->pairs;
    dcreg_ctx::NormalBufs &B = c->nrm;
    const size_t nt = (size_t)ps.n;
    const int64_t n = ps.off.back();
    if (infos) std::memset(infos, 0, sizeof(*infos) * nt);
    HIP_TRY(c, hipSetDevice(c->device));
    ps.normals_kept = false;                                    // (a failed call leaves none)
    std::vector<unsigned long long> cnt(2 * nt, 0ull);
    std::vector<uint8_t> has(nt, 0);
    if (n > 0) {
        if (B.normal.ensure(c, 3 * (size_t)n) || B.curv.ensure(c, (size_t)n) || B.cnt.ensure(c, 2 * nt) || ps.normals.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
        const float nanf_ = __builtin_nanf("");
        fill_f32(c, B.normal.data(), 3 * n, nanf_);
        fill_f32(c, B.curv.data(), n, nanf_);
        HIP_TRY(c, hipMemsetAsync(B.cnt.data(), 0, 2 * nt * sizeof(unsigned long long), c->stream));
        const NrmSearch sr = nrm_search(p, nullptr);
        std::vector<NrmCloud> recs;
        std::vector<uint2> blk;
        for (size_t t = 0; t < nt; ++t) {
            const int64_t m = ps.off[t + 1] - ps.off[t];
            if (!ps.built[t] || m < p->k) continue;
            NrmCloud r;
            r.g = ps.grids[t];
            r.max_ring = p->search_radius > 0.0 ? rings_for_bound(ps.grids[t], sr.bound) : -1;
            r.cloud = (uint32_t)t;
            r.base = (uint32_t)ps.off[t];
            const uint32_t nb = blocks(m, kBlock);
            for (uint32_t b = 0; b < nb; ++b) blk.push_back(make_uint2((uint32_t)recs.size(), b));
            recs.push_back(r);
            has[t] = 1;
        }
        const size_t rec_bytes = recs.size() * sizeof(NrmCloud), bytes = rec_bytes + blk.size() * sizeof(uint2);
        std::vector<unsigned char> h(bytes);
        if (!recs.empty()) {
            std::memcpy(h.data(), recs.data(), rec_bytes);
            std::memcpy(h.data() + rec_bytes, blk.data(), blk.size() * sizeof(uint2));
            if (B.d_launch.ensure(c, bytes)) return DCREG_E_NOMEM;
            HIP_TRY(c, hipMemcpyAsync(B.d_launch.data(), h.data(), bytes, hipMemcpyHostToDevice, c->stream));
            const NrmCloud *d_recs = (const NrmCloud *)B.d_launch.data();
            const uint2 *d_blk = (const uint2 *)(B.d_launch.data() + rec_bytes);
            const dim3 grid((unsigned)blk.size()), block(kBlock);
            const int k = p->k;
            with_heap_k(k, [&](auto K) { hipLaunchKernelGGL((k_nrm_batch<decltype(K)::value, true>), grid, block, 0, c->stream, d_recs, d_blk, sr.bound, k, sr.a, B.normal.data(), B.curv.data(), B.cnt.data()); });
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(cnt.data(), B.cnt.data(), sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost, c->stream));
        }
        hipLaunchKernelGGL(k_nrm_pack, dim3(blocks(n, 256)), dim3(256), 0, c->stream, B.normal.data(), (int64_t)3, B.curv.data(), n, ps.normals.data());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));              // (h is the source of the upload)
        HIP_TRY(c, hipGetLastError());
    }
    if (infos)
        for (size_t t = 0; t < nt; ++t) {
            const int64_t m = ps.off[t + 1] - ps.off[t];
            infos[t].n_in = m; infos[t].n_finite = m;
            infos[t].n_sparse = has[t] ? (int64_t)cnt[2 * t + 1] : m;
            infos[t].n_out = has[t] ? (int64_t)cnt[2 * t] : 0;
        }
    if (int rc = pairs_nn_grids(c)) return rc;
    ps.normals_kept = true;
    return DCREG_OK;
}

// dcreg_pairs_normals_set: the caller's normals for all points of the batch in its upload order become the kept normals, as given
int pairs_normals_set(dcreg_ctx *c, const float *normals, int64_t n_given, int64_t stride) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = kept_args(c, normals, stride)) return rc;
    if (int rc = pairs_batch_check(c)) return rc;
    dcreg_ctx::PairSet &ps = c->pairs;
    const int64_t n = ps.off.back();
    if (int rc = kept_count(c, "the pair targets hold", n, n_given)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ps.normals_kept = false;
    if (n > 0)
        if (int rc = kept_take(c, normals, n, stride, false, ps.normals, n, [&](const float *src) {
                hipLaunchKernelGGL(k_nrm_pack, dim3(blocks(n, 256)), dim3(256), 0, c->stream, src, stride, (const float *)nullptr, n, ps.normals.data());
            }))
            return rc;
    if (int rc = pairs_nn_grids(c)) return rc;
    ps.normals_kept = true;
    return DCREG_OK;
}

// dcreg_pairs_normals_get: the batch's kept normals as they stand, 4 floats per point
int pairs_normals_get(dcreg_ctx *c, float *out, int64_t capacity) {
    if (!c) return DCREG_E_INVALID;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (int rc = pairs_batch_check(c)) return rc;
    dcreg_ctx::PairSet &ps = c->pairs;
    if (!ps.normals_kept) { c->fail("no kept pair normals: dcreg_pairs_normals_keep or dcreg_pairs_normals_set first"); return DCREG_E_STATE; }
    const int64_t n = ps.off.back();
    if (int rc = kept_capacity(c, "the pair targets hold", n, capacity)) return rc;
    if (n == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    return kept_give(c, out, ps.normals.data(), n, false);
}

// dcreg_target_normals*: the whole map's points through the map's own index
// keep: into the context's kept normals (dcreg_target_normals_keep: no outputs, no capacity)
int normals_map(dcreg_ctx *c, bool on_device, const dcreg_normal_params *p, float *normal, float *curv, float *eig, int64_t capacity,
                dcreg_normal_info *info, bool keep = false) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = normals_check(c, p)) return rc;
    if (!keep && !normal && !curv && !eig) { c->fail("no output buffer: normals, curvature or eigenvalues expected"); return DCREG_E_INVALID; }
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    const dcreg_ctx::IndexSet &wm = c->roi_active ? c->roi_store : c->map;      // the whole map's index, whichever is active
    const int64_t n = wm.n;
    if (!keep && capacity < n) { c->fail("the map holds %lld points, the capacity is %lld", (long long)n, (long long)capacity); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    const NormalOut o{normal, curv, eig, on_device, keep};
    if (!keep) return normals_run(c, wm.sorted.data(), n, wm.grid, n, n, p, o, info);
    c->nicp.kept = false; c->nicp.warm_valid = false;          // (a failed call leaves none)
    if (int rc = normals_run(c, wm.sorted.data(), n, wm.grid, n, n, p, o, info)) return rc;
    c->nicp.kept = true;
    c->nicp.from_keep = true; c->nicp.keep_params = *p;        // (the rule a followed update refits with: "normals_follow")
    return DCREG_OK;
}

// dcreg_target_normals_set*: the caller's normals in index order become the kept normals, as given
int normals_set(dcreg_ctx *c, const float *normals, int64_t n, int64_t stride, bool on_device) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = kept_args(c, normals, stride)) return rc;
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    if (int rc = kept_count(c, "the map holds", c->roi_active ? c->roi_store.n : c->map.n, n)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->nicp.kept = false; c->nicp.warm_valid = false;
    c->nicp.from_keep = false;                                 // (given normals have no rule to refit with: updates drop them)
    if (int rc = kept_take(c, normals, n, stride, on_device, c->nicp.normals, n, [&](const float *src) {
            hipLaunchKernelGGL(k_nrm_pack, dim3(blocks(n, 256)), dim3(256), 0, c->stream, src, stride, (const float *)nullptr, n, c->nicp.normals.data());
        }))
        return rc;
    c->nicp.kept = true;
    return DCREG_OK;
}


// dcreg_source_normals_keep: the cloud form over the context's source in its original order (d_src_raw is what upload_cloud packs for
// dcreg_normals: the same points, the same index build, the same kernel), then one pack into curve order
int normals_source_keep(dcreg_ctx *c, const dcreg_normal_params *p, dcreg_normal_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = normals_check(c, p)) return rc;
    if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    if (info) std::memset(info, 0, sizeof(*info));
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t n = c->n_src;
    c->gicp.src_kept = false;                                   // (a failed call leaves none)
    if (c->gicp.src_normals.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
    int64_t n_used = 0;
    if (int rc = cloud_index_used(c, c->d_src_raw.data(), n, p->search_radius, p->k, &n_used)) return rc;
    const bool indexed = n_used >= p->k;
    NormalOut o{nullptr, nullptr, nullptr, true};
    o.scratch = true;
    if (int rc = normals_run(c, indexed ? c->cloud.idx.sorted.data() : nullptr, indexed ? n_used : 0, indexed ? c->cloud.idx.grid : GridDev{}, n, n_used, p, o, info))
        return rc;
    hipLaunchKernelGGL(k_nrm_pack_src, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->d_src.data(), n, c->nrm.normal.data(), (int64_t)3,
                       c->nrm.curv.data(), c->gicp.src_normals.data());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->gicp.src_kept = true;
    return DCREG_OK;
}

// dcreg_source_normals_set*: the caller's normals in the source's original order become the kept source normals, as given
int normals_source_set(dcreg_ctx *c, const float *normals, int64_t n, int64_t stride, bool on_device) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = kept_args(c, normals, stride)) return rc;
    if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    if (int rc = kept_count(c, "the source holds", c->n_src, n)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->gicp.src_kept = false;
    if (int rc = kept_take(c, normals, n, stride, on_device, c->gicp.src_normals, n, [&](const float *src) {
            hipLaunchKernelGGL(k_nrm_pack_src, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->d_src.data(), n, src, stride, (const float *)nullptr,
                               c->gicp.src_normals.data());
        }))
        return rc;
    c->gicp.src_kept = true;
    return DCREG_OK;
}

// dcreg_source_normals_get*: the kept source normals as they stand, 4 floats per point in the source's original order
int normals_source_get(dcreg_ctx *c, float *out, int64_t capacity, bool on_device) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (!c->gicp.src_kept) { c->fail("no kept source normals: dcreg_source_normals_keep or dcreg_source_normals_set first"); return DCREG_E_STATE; }
    const int64_t n = c->n_src;
    if (int rc = kept_capacity(c, "the source holds", n, capacity)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->gicp.tmp.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_nrm_unpack_src, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->d_src.data(), n, c->gicp.src_normals.data(), c->gicp.tmp.data());
    HIP_TRY(c, hipGetLastError());
    return kept_give(c, out, c->gicp.tmp.data(), n, on_device);
}

// ------------------------------------------------------------------------------------------ kept normals that follow the map ("normals_follow")
// Candidates are ranked by (d2, index).  An insert appends, so an old point's neighbour set changes only if a new point has a float d2
// BELOW its k-th d2 (an equal one loses on the index); a removal renumbers the survivors in their old order, so a survivor's set changes
// only if a removed point had d2 AT OR BELOW its k-th d2.  With the k-th d2 kept per point (its reach; the search bound for a sparse point)
// the points whose result can have changed are those with a point that came or went within their reach, and everything else is carried
// bit for bit.  The test below is conservative - it may refit a clean point, never miss a changed one - and works on cells:
//   k_follow_mark   one bit per cell of the UPDATED map's grid (x sub-cells ignored) for every point that came or went, its cell taken as
//                   floor((x - o) / h) per axis in doubles and clamped to the grid: a removed point outside the new box lands in the
//                   nearest cell, and clamping into a convex box that holds the query never increases a distance
//   k_follow_dirty  one lane per point of the updated map in cell order: the cells whose distance to the point is within its reach are
//                   walked and their bits tested.  A cell's distance is the exact one between the point and the cell's slab per axis, in
//                   cells and doubles, against sqrt(reach) / h enlarged by 1e-5 relative and 1e-6 cells: dist2_nofma's float chain can
//                   come out below the exact value by a few ulp (4e-7 relative at most), the doubles of the cell coordinates by 1e-10
//                   cells - so the bound never exceeds a float d2 the search would compute for a point of that cell.  A reach of more
//                   than kFollowRings cells (isolated points of an unbounded search, sparse points of a wide radius) is not walked:
//                   the point is dirty.  Appended points (index >= n_old) are dirty.
constexpr int kFollowRings = 3;
constexpr double kFollowRel = 1.0e-5, kFollowAbs = 1.0e-6;

DCREG_DEVFN int follow_cell(double f, int n) { return (int)fmin(fmax(floor(f), 0.0), (double)(n - 1)); }

// keep != null: the points whose flag is set stay - only the others are marked
static __global__ void k_follow_mark(const float4 *__restrict__ pts, int64_t n, const uint32_t *__restrict__ keep, GridDev g, uint32_t *__restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (keep && keep[i] != 0u)) return;
    const float4 v = pts[i];
    const int cx = follow_cell(((double)v.x - g.ox) * g.inv_h, g.nx), cy = follow_cell(((double)v.y - g.oy) * g.inv_h, g.ny),
              cz = follow_cell(((double)v.z - g.oz) * g.inv_h, g.nz);
    const int64_t cell = ((int64_t)cz * g.ny + cy) * g.nx + cx;
    atomicOr(bits + (cell >> 5), 1u << (uint32_t)(cell & 31));
}

// squared distance, in cells, from coordinate f to the slab [c, c + 1)
DCREG_DEVFN double follow_gap2(double f, int c) {
    const double lo = (double)c - f, hi = f - (double)(c + 1);
    const double gp = fmax(fmax(lo, hi), 0.0);
    return gp * gp;
}

// flag[i] = 1: the point at sorted position i must be refitted (n + 1 entries, the last 0)
static __global__ __launch_bounds__(kBlock) void k_follow_dirty(const float4 *__restrict__ sorted, uint32_t n, uint32_t n_old, const float *__restrict__ reach,
                                                               GridDev g, const uint32_t *__restrict__ bits, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) { flag[i] = 0u; return; }
    const float4 s4 = sorted[i];
    const uint32_t self = __float_as_uint(s4.w);
    bool dirty = self >= n_old;
    if (!dirty) {
        const double rc = sqrt((double)reach[self]) * g.inv_h * (1.0 + kFollowRel) + kFollowAbs;      // the reach in cells
        if (!(rc <= (double)kFollowRings)) dirty = true;                                              // (a NaN reach too)
        else {
            const double fx = ((double)s4.x - g.ox) * g.inv_h, fy = ((double)s4.y - g.oy) * g.inv_h, fz = ((double)s4.z - g.oz) * g.inv_h;
            const double r2 = rc * rc;
            const int x0 = follow_cell(fx - rc, g.nx), x1 = follow_cell(fx + rc, g.nx), y0 = follow_cell(fy - rc, g.ny), y1 = follow_cell(fy + rc, g.ny),
                      z0 = follow_cell(fz - rc, g.nz), z1 = follow_cell(fz + rc, g.nz);
            for (int z = z0; z <= z1 && !dirty; ++z) {
                const double gz = follow_gap2(fz, z);
                for (int y = y0; y <= y1 && !dirty; ++y) {
                    const double gyz = gz + follow_gap2(fy, y);
                    if (gyz > r2) continue;
                    const int64_t row = ((int64_t)z * g.ny + y) * g.nx;
                    for (int x = x0; x <= x1; ++x) {
                        const int64_t cell = row + x;
                        const bool hit = (bits[cell >> 5] >> (uint32_t)(cell & 31)) & 1u;
                        if (hit && gyz + follow_gap2(fx, x) <= r2) { dirty = true; break; }
                    }
                }
            }
        }
    }
    flag[i] = dirty ? 1u : 0u;
}

// the dirty points, compacted in cell order: k_nrm's input
static __global__ void k_follow_gather(const float4 *__restrict__ sorted, int64_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                       float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    out[pos[i]] = sorted[i];
}

// the survivors' kept normals and reaches, renumbered as k_crop_raw renumbers the points
static __global__ void k_follow_crop(const float4 *__restrict__ normals, const float *__restrict__ reach, int64_t n, const uint32_t *__restrict__ flag,
                                     const uint32_t *__restrict__ pos, float4 *__restrict__ normals_out, float *__restrict__ reach_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint32_t r = pos[i];
    normals_out[r] = normals[i];
    reach_out[r] = reach[i];
}

// An incremental refit searches from a compacted list: its waves' lanes are neighbours only where dirty points are, and each pays the
// dirty test of the whole map first.  Past a share of dirty points ("normals_follow_full_share") the update recomputes everything
// (followed = 2).  DESIGN.md, "Kept normals that follow the map", has the numbers behind the default; no result depends on it.

// dirty test, compaction and refit behind the marks; the arrays already hold the carried entries of the n points of c->map
int follow_refit(dcreg_ctx *c, int64_t n, int64_t n_old) {
    dcreg_ctx::NormalIcpBufs &N = c->nicp;
    const dcreg_ctx::IndexSet &m = c->map;
    const size_t n1 = (size_t)n + 1;
    if (N.f_flag.ensure(c, 2 * n1) || c->nrm.cnt.ensure(c, 2)) return DCREG_E_NOMEM;
    uint32_t *flag = N.f_flag.data(), *pos = flag + n1;
    hipLaunchKernelGGL(k_follow_dirty, dim3(blocks((int64_t)n1, kBlock)), dim3(kBlock), 0, c->stream, m.sorted.data(), (uint32_t)n, (uint32_t)n_old,
                       N.reach.data(), m.grid, N.f_bits.data(), flag);
    if (int rc = scan_u32(c, flag, pos, n1, false)) return rc;
    uint32_t n_dirty = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_dirty, pos + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if ((double)n_dirty > c->opt_normals_follow_full_share * (double)n) {
        NormalOut o{nullptr, nullptr, nullptr, true, true};
        if (int rc = normals_run(c, m.sorted.data(), n, m.grid, n, n, &N.keep_params, o, nullptr)) return rc;
        N.follow.n_refit = n; N.follow.n_carried = 0; N.follow.followed = 2;
        return DCREG_OK;
    }
    if (n_dirty > 0u) {
        if (N.f_list.ensure(c, (size_t)n_dirty)) return DCREG_E_NOMEM;
        hipLaunchKernelGGL(k_follow_gather, dim3(blocks(n, 256)), dim3(256), 0, c->stream, m.sorted.data(), n, flag, pos, N.f_list.data());
        HIP_TRY(c, hipMemsetAsync(c->nrm.cnt.data(), 0, 2 * sizeof(unsigned long long), c->stream));
        launch_nrm_k(c, N.f_list.data(), (int64_t)n_dirty, m.grid, &N.keep_params, nullptr, nullptr, nullptr, N.normals.data(), N.reach.data());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    }
    N.follow.n_refit = (int64_t)n_dirty; N.follow.n_carried = n - (int64_t)n_dirty; N.follow.followed = 1;
    return DCREG_OK;
}

int follow_update(dcreg_ctx *c, const FollowChange &ch) {
    dcreg_ctx::NormalIcpBufs &N = c->nicp;
    const dcreg_ctx::IndexSet &m = c->map;
    const GridDev &g = m.grid;
    const int64_t n = m.n;
    if (n <= 0 || c->roi_active) { c->fail("the kept normals cannot follow: the whole map's index is not the active one"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t n_old = n;                                    // indices below it are points the map had before
    if (ch.carried) {
        N.normals.swap(N.normals_alt);
        N.reach.swap(N.reach_alt);
    } else {
        n_old = n - ch.n_added;
        if (n_old < 0 || N.normals.grow_keep(c, (size_t)n, (size_t)n_old) || N.reach.grow_keep(c, (size_t)n, (size_t)n_old)) return DCREG_E_NOMEM;
    }
    const size_t n_words = (size_t)(((int64_t)g.nx * g.ny * g.nz + 31) >> 5);
    if (N.f_bits.ensure(c, n_words)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(N.f_bits.data(), 0, n_words * sizeof(uint32_t), c->stream));
    if (ch.n_added > 0)
        hipLaunchKernelGGL(k_follow_mark, dim3(blocks(ch.n_added, 256)), dim3(256), 0, c->stream, ch.added, ch.n_added, (const uint32_t *)nullptr, g,
                           N.f_bits.data());
    if (ch.n_old > 0)
        hipLaunchKernelGGL(k_follow_mark, dim3(blocks(ch.n_old, 256)), dim3(256), 0, c->stream, ch.old_raw, ch.n_old, ch.flag_r, g, N.f_bits.data());
    HIP_TRY(c, hipGetLastError());
    return follow_refit(c, n, n_old);
}

// dcreg_target_normals_get*: the kept normals as they stand, 4 floats per point
int normals_get(dcreg_ctx *c, float *out, int64_t capacity, bool on_device) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (!c->nicp.kept) { c->fail("no kept normals: dcreg_target_normals_keep or dcreg_target_normals_set first"); return DCREG_E_STATE; }
    const int64_t n = c->roi_active ? c->roi_store.n : c->map.n;
    if (int rc = kept_capacity(c, "the map holds", n, capacity)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return kept_give(c, out, c->nicp.normals.data(), n, on_device);
}

}  // namespace

// features.hip (dcreg_fpfh with normals == NULL): dcreg_normals of a cloud that is already indexed - normals and curvature into the call's
// scratch (c->nrm.normal, 3 floats per point; c->nrm.curv), NaN where a point has none; waits for the stream
int normals_to_scratch(dcreg_ctx *c, const float4 *q, int64_t nq, const GridDev &g, int64_t n, int64_t n_used, const dcreg_normal_params *p,
                       dcreg_normal_info *info) {
    NormalOut o{nullptr, nullptr, nullptr, true};
    o.scratch = true;
    return normals_run(c, q, nq, g, n, n_used, p, o, info);
}

bool normals_follow_wanted(const dcreg_ctx *c) { return c->opt_normals_follow && c->nicp.kept && c->nicp.from_keep; }

bool normals_follow_carry(dcreg_ctx *c, int64_t n_old, const uint32_t *flag_r, const uint32_t *pos_r, int64_t kept) {
    dcreg_ctx::NormalIcpBufs &N = c->nicp;
    if (N.normals_alt.ensure(c, (size_t)kept) || N.reach_alt.ensure(c, (size_t)kept)) return false;
    hipLaunchKernelGGL(k_follow_crop, dim3(blocks(n_old, 256)), dim3(256), 0, c->stream, N.normals.data(), N.reach.data(), n_old, flag_r, pos_r,
                       N.normals_alt.data(), N.reach_alt.data());
    return true;
}

// (the update stands whatever happens here: a failure leaves the normals dropped, as map_changed left them, and says so in the info)
void normals_follow_update(dcreg_ctx *c, const FollowChange &ch) {
    c->nicp.follow.n_target = c->map.n;
    if (follow_update(c, ch) == DCREG_OK) { c->nicp.kept = true; return; }
    (void)hipGetLastError();
    c->nicp.kept = false;
    c->nicp.follow.n_refit = 0; c->nicp.follow.n_carried = 0; c->nicp.follow.followed = 0;
}

}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_default_normal_params(dcreg_normal_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->k = 5; p->orient = DCREG_NORMAL_ORIENT_VIEWPOINT; p->search_radius = 0.0;
    return DCREG_OK;
}
int dcreg_normals(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_normal_params *p, float *normals_out,
                  float *curvature_out, float *eigenvalues_out, dcreg_normal_info *info) {
    return normals_cloud(c, xyz, n, stride_floats, false, p, normals_out, curvature_out, eigenvalues_out, info);
}
int dcreg_normals_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_normal_params *p, float *d_normals_out,
                         float *d_curvature_out, float *d_eigenvalues_out, dcreg_normal_info *info) {
    return normals_cloud(c, d_xyz, n, stride_floats, true, p, d_normals_out, d_curvature_out, d_eigenvalues_out, info);
}
int dcreg_normals_clouds(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_normal_params *p,
                         float *normals_out, float *curvature_out, dcreg_normal_info *infos) {
    return normals_clouds(c, n_clouds, xyz, offsets, stride_floats, false, p, normals_out, curvature_out, infos);
}
int dcreg_normals_clouds_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                const dcreg_normal_params *p, float *d_normals_out, float *d_curvature_out, dcreg_normal_info *infos) {
    return normals_clouds(c, n_clouds, d_xyz, offsets, stride_floats, true, p, d_normals_out, d_curvature_out, infos);
}
int dcreg_frames_normals_keep(dcreg_ctx *c, const dcreg_normal_params *p, dcreg_normal_info *infos) {
    return c ? frames_normals_keep(c, c->frames, p, infos) : DCREG_E_INVALID;
}
int dcreg_frames_normals_set(dcreg_ctx *c, const float *normals, int64_t n_points, int64_t stride_floats) {
    return c ? frames_normals_set(c, c->frames, normals, n_points, stride_floats) : DCREG_E_INVALID;
}
int dcreg_pairs_sources_normals_keep(dcreg_ctx *c, const dcreg_normal_params *p, dcreg_normal_info *infos) {
    return c ? frames_normals_keep(c, c->pair_src, p, infos) : DCREG_E_INVALID;
}
int dcreg_pairs_sources_normals_set(dcreg_ctx *c, const float *normals, int64_t n_points, int64_t stride_floats) {
    return c ? frames_normals_set(c, c->pair_src, normals, n_points, stride_floats) : DCREG_E_INVALID;
}
int dcreg_pairs_sources_normals_get(dcreg_ctx *c, float *out, int64_t capacity_points) {
    return c ? frames_normals_get(c, c->pair_src, out, capacity_points) : DCREG_E_INVALID;
}
int dcreg_pairs_normals_keep(dcreg_ctx *c, const dcreg_normal_params *p, dcreg_normal_info *infos) { return pairs_normals_keep(c, p, infos); }
int dcreg_pairs_normals_set(dcreg_ctx *c, const float *normals, int64_t n_points, int64_t stride_floats) {
    return pairs_normals_set(c, normals, n_points, stride_floats);
}
int dcreg_pairs_normals_get(dcreg_ctx *c, float *out, int64_t capacity_points) { return pairs_normals_get(c, out, capacity_points); }
int dcreg_pairs_normals_kept(const dcreg_ctx *c) { return c && c->pairs.normals_kept ? 1 : 0; }
int dcreg_frames_normals_kept(const dcreg_ctx *c) { return c && c->frames.normals_kept ? 1 : 0; }
int dcreg_normal_params_check(dcreg_ctx *c, const dcreg_normal_params *p) { return c ? normals_check(c, p) : DCREG_E_INVALID; }
int dcreg_target_normals(dcreg_ctx *c, const dcreg_normal_params *p, float *normals_out, float *curvature_out, float *eigenvalues_out,
                         int64_t capacity_points, dcreg_normal_info *info) {
    return normals_map(c, false, p, normals_out, curvature_out, eigenvalues_out, capacity_points, info);
}
int dcreg_target_normals_device(dcreg_ctx *c, const dcreg_normal_params *p, float *d_normals_out, float *d_curvature_out,
                                float *d_eigenvalues_out, int64_t capacity_points, dcreg_normal_info *info) {
    return normals_map(c, true, p, d_normals_out, d_curvature_out, d_eigenvalues_out, capacity_points, info);
}
int dcreg_target_normals_keep(dcreg_ctx *c, const dcreg_normal_params *p, dcreg_normal_info *info) {
    return normals_map(c, true, p, nullptr, nullptr, nullptr, 0, info, true);
}
int dcreg_target_normals_set(dcreg_ctx *c, const float *normals, int64_t n, int64_t stride_floats) { return normals_set(c, normals, n, stride_floats, false); }
int dcreg_target_normals_set_device(dcreg_ctx *c, const float *d_normals, int64_t n, int64_t stride_floats) {
    return normals_set(c, d_normals, n, stride_floats, true);
}
int dcreg_target_normals_kept(const dcreg_ctx *c) { return c && c->nicp.kept ? 1 : 0; }
int dcreg_target_normals_drop(dcreg_ctx *c) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    c->nicp.kept = false; c->nicp.warm_valid = false;
    c->nicp.normals.reset(); c->nicp.reach.reset();
    c->nicp.normals_alt.reset(); c->nicp.reach_alt.reset(); c->nicp.f_list.reset(); c->nicp.f_bits.reset(); c->nicp.f_flag.reset();
    return DCREG_OK;
}
int dcreg_target_normals_get(dcreg_ctx *c, float *out, int64_t capacity_points) { return normals_get(c, out, capacity_points, false); }
int dcreg_target_normals_get_device(dcreg_ctx *c, float *d_out, int64_t capacity_points) { return normals_get(c, d_out, capacity_points, true); }
int dcreg_source_normals_keep(dcreg_ctx *c, const dcreg_normal_params *p, dcreg_normal_info *info) { return normals_source_keep(c, p, info); }
int dcreg_source_normals_set(dcreg_ctx *c, const float *normals, int64_t n, int64_t stride_floats) { return normals_source_set(c, normals, n, stride_floats, false); }
int dcreg_source_normals_set_device(dcreg_ctx *c, const float *d_normals, int64_t n, int64_t stride_floats) {
    return normals_source_set(c, d_normals, n, stride_floats, true);
}
int dcreg_source_normals_get(dcreg_ctx *c, float *out, int64_t capacity_points) { return normals_source_get(c, out, capacity_points, false); }
int dcreg_source_normals_get_device(dcreg_ctx *c, float *d_out, int64_t capacity_points) { return normals_source_get(c, d_out, capacity_points, true); }
int dcreg_source_normals_kept(const dcreg_ctx *c) { return c && c->gicp.src_kept ? 1 : 0; }
int dcreg_source_normals_drop(dcreg_ctx *c) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    c->gicp.src_kept = false;
    c->gicp.src_normals.reset(); c->gicp.tmp.reset();
    return DCREG_OK;
}
int dcreg_target_normals_follow_info(const dcreg_ctx *c, dcreg_normals_follow_info *info) {
    if (!c || !info) return DCREG_E_INVALID;
    *info = c->nicp.follow;
    return DCREG_OK;
}
}
