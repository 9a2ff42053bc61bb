// Voxel-grid downsampling on the device (include/dcreg.h: dcreg_voxel_downsample*, dcreg_set_source_voxel*, dcreg_set_target_voxel*).
// Raw LiDAR sweeps (NaN where a beam had no return) and dense maps go in; one point per occupied voxel comes out, with PCL VoxelGrid's order
// and semantics (the exact rules are in the header).  One segmented path serves every entry point - a cloud is a segment, a single cloud one
// segment:
//   k_vox_coords   finite flag, voxel coordinates, per-cloud minimum / maximum voxel and finite count (integer atomics: deterministic)
//   (readback)     spans and refusals on the host, the key widths
//   k_vox_keys     key = (cloud, voxel relative to the cloud's minimum), z y x; non-finite points get cloud id n_clouds (sorted behind all)
//   radix sort     stable: the points of a voxel stay in input order (one pass when cloud + voxel bits fit 64, else voxel key then cloud)
//   k_vox_heads    first sorted position of every voxel; inclusive scan = voxel numbers; k_vox_starts: where each voxel starts
//   k_vox_reduce   ONE lane per voxel: count, min_points, the sequential double sum (or the first point) - exact and reproducible
//   scan + k_vox_write   compaction, per-cloud counts, bounds of the output
//   (readback)     counts, bounds: the only one at the end of the call
// The packed points come from upload_cloud: k_pack, the deskew packs (DeskewRun) or the keyframe gather (GatherRun, keyframes.hip).
// A voxel's result depends on its own points only: where its cloud sits in the call and how the launches are cut never enter it.
// The kept voxel map of the fourth engine (voxel_map_keep: k_vmap_reduce, k_vmap_write) runs behind the same keying and sort, and so do
// the voxel maps of a build batch of scan-pair targets, one per target, all at once (pairs_voxels_build: k_pvmap_count, k_pvmap_write).
// Under "voxels_follow" an update of the map refits the kept voxel map's touched voxels and carries the rest (follow_run: k_vfollow_*).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "context.hpp"
#include "jacobi.hpp"
#include "voxel_icp.hpp"

namespace dcreg {
namespace {

constexpr int kVoxBlock = 256;
constexpr int kVoxPerThread = 8;                        // points per thread of k_vox_coords (a block covers one tile of 2048 points)
constexpr int kSpanBits = 21;                           // a cloud spans fewer than 2^21 voxels per axis
constexpr int64_t kSpanMax = ((int64_t)1 << kSpanBits) - 1;     // the most voxels per axis that are accepted: 2^21 or more are refused
constexpr double kVoxLimit = 4611686018427387904.0;     // 2^62: voxel coordinates beyond it are refused
// counters of one call, per cloud s: cnt[kCnt s + 0..2] minimum voxel x y z, + 3..5 maximum, + 6 finite points, + 7 voxels, + 8 kept voxels;
// behind the clouds kTail int64 slots read as uint32: [0..2] minimum, [3..5] maximum of the output (ordered-uint, k_bounds), [6] overflow
constexpr int kCnt = 9;
constexpr int kTail = 4;

// floor((double)p / leaf) per axis, as the header defines it (an IEEE double division: the build has no fast-math)
__device__ __forceinline__ void voxel_of(const float4 p, const double lx, const double ly, const double lz, double v[3]) {
    v[0] = floor((double)p.x / lx);
    v[1] = floor((double)p.y / ly);
    v[2] = floor((double)p.z / lz);
}

static __global__ void k_vox_init(int64_t *__restrict__ cnt, int n_clouds) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nc = (int64_t)kCnt * n_clouds;
    if (i < nc) {
        const int f = (int)(i % kCnt);
        cnt[i] = f < 3 ? INT64_MAX : f < 6 ? INT64_MIN : 0;
    } else if (i < nc + 2 * kTail) {
        const int j = (int)(i - nc);
        reinterpret_cast<uint32_t *>(cnt + nc)[j] = j < 3 ? 0xFFFFFFFFu : 0u;
    }
}

// Pass 1: the cloud of every point, and per cloud the minimum / maximum voxel and the finite points.  A block covers a tile of kVoxBlock x
// kVoxPerThread points; a tile inside one cloud reduces in registers and LDS and adds 7 atomics, a tile across clouds adds per point.
static __global__ void __launch_bounds__(kVoxBlock) k_vox_coords(const float4 *__restrict__ pts, int64_t n, const int64_t *__restrict__ off,
                                                                 int n_clouds, double lx, double ly, double lz, uint32_t *__restrict__ seg,
                                                                 int64_t *__restrict__ cnt) {
    const int64_t base = (int64_t)blockIdx.x * (kVoxBlock * kVoxPerThread);
    const int64_t last = std::min<int64_t>(n, base + kVoxBlock * kVoxPerThread) - 1;
    const uint32_t s0 = seg_of(off, n_clouds, base);
    const bool uniform = seg_of(off, n_clouds, last) == s0;
    uint32_t *ovf = reinterpret_cast<uint32_t *>(cnt + (int64_t)kCnt * n_clouds) + 6;
    long long mn[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, mx[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    long long fin = 0;
    for (int k = 0; k < kVoxPerThread; ++k) {
        const int64_t i = base + threadIdx.x + (int64_t)k * kVoxBlock;
        if (i > last) break;
        const uint32_t s = uniform ? s0 : seg_of(off, n_clouds, i);
        seg[i] = s;
        const float4 p = pts[i];
        if (!finite_point(p)) continue;
        double v[3];
        voxel_of(p, lx, ly, lz, v);
        long long vi[3];
        bool big = false;
        for (int a = 0; a < 3; ++a) {
            big |= !(fabs(v[a]) < kVoxLimit);
            vi[a] = big ? 0 : (long long)v[a];
        }
        if (big) { atomicOr(ovf, 1u); continue; }
        if (uniform) {
            for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], vi[a]); mx[a] = std::max(mx[a], vi[a]); }
            ++fin;
        } else {
            long long *c = reinterpret_cast<long long *>(cnt + (int64_t)kCnt * s);
            for (int a = 0; a < 3; ++a) { atomicMin(c + a, vi[a]); atomicMax(c + 3 + a, vi[a]); }
            atomicAdd(reinterpret_cast<unsigned long long *>(c + 6), 1ull);
        }
    }
    if (!uniform) return;          // (block-uniform)
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], (long long)__shfl_xor(mn[a], o)); mx[a] = std::max(mx[a], (long long)__shfl_xor(mx[a], o)); }
        fin += __shfl_xor(fin, o);
    }
    __shared__ long long smn[kVoxBlock / 64][3], smx[kVoxBlock / 64][3], sfin[kVoxBlock / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) { smn[wave][a] = mn[a]; smx[wave][a] = mx[a]; }
        sfin[wave] = fin;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kVoxBlock / 64; ++w) {
            for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], smn[w][a]); mx[a] = std::max(mx[a], smx[w][a]); }
            fin += sfin[w];
        }
        if (fin > 0) {
            long long *c = reinterpret_cast<long long *>(cnt + (int64_t)kCnt * s0);
            for (int a = 0; a < 3; ++a) { atomicMin(c + a, mn[a]); atomicMax(c + 3 + a, mx[a]); }
            atomicAdd(reinterpret_cast<unsigned long long *>(c + 6), (unsigned long long)fin);
        }
    }
}

// Pass 2: the sort key of every point - (cloud, voxel z y x relative to the cloud's minimum) when `with_seg`, else the voxel part alone -
// and rel = the voxel part.  A non-finite point is given cloud n_clouds (seg[i] too): it sorts behind every voxel.
static __global__ void k_vox_keys(const float4 *__restrict__ pts, int64_t n, uint32_t *__restrict__ seg, int n_clouds, double lx, double ly,
                                  double lz, const int64_t *__restrict__ cnt, int bx, int by, int bz, bool with_seg, uint64_t *__restrict__ keys,
                                  uint32_t *__restrict__ vals, uint64_t *__restrict__ rel) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    uint32_t s = seg[i];
    uint64_t r = 0;
    if (finite_point(p)) {
        double v[3];
        voxel_of(p, lx, ly, lz, v);
        const int64_t *c = cnt + (int64_t)kCnt * s;
        const uint64_t rx = (uint64_t)((long long)v[0] - c[0]), ry = (uint64_t)((long long)v[1] - c[1]), rz = (uint64_t)((long long)v[2] - c[2]);
        r = (rz << (bx + by)) | (ry << bx) | rx;
    } else {
        s = (uint32_t)n_clouds;
        seg[i] = s;
    }
    rel[i] = r;
    keys[i] = with_seg ? (((uint64_t)s << (bx + by + bz)) | r) : r;
    vals[i] = (uint32_t)i;
}

// the cloud of every sorted position: the key of the second (stable) sort of the two-pass order
static __global__ void k_vox_seg_keys(const uint32_t *__restrict__ ord, int64_t n, const uint32_t *__restrict__ seg, uint32_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = seg[ord[i]];
}

// head[i] = sorted position i is the first point of a voxel
static __global__ void k_vox_heads(const uint32_t *__restrict__ ord, int64_t n, const uint32_t *__restrict__ seg, const uint64_t *__restrict__ rel,
                                   uint32_t n_clouds, uint32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = ord[i], s = seg[o];
    bool h = s < n_clouds;
    if (h && i > 0) {
        const uint32_t q = ord[i - 1];
        h = seg[q] != s || rel[q] != rel[o];
    }
    head[i] = h ? 1u : 0u;
}

// start[v] = first sorted position of voxel v (v = incl - 1 at a head); start[V] = one past the last finite point
static __global__ void k_vox_starts(const uint32_t *__restrict__ ord, int64_t n, const uint32_t *__restrict__ seg, uint32_t n_clouds,
                                    const uint32_t *__restrict__ head, const uint32_t *__restrict__ incl, uint32_t *__restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (head[i]) start[incl[i] - 1] = (uint32_t)i;
    if (seg[ord[i]] < n_clouds && (i == n - 1 || seg[ord[i + 1]] >= n_clouds)) start[incl[i]] = (uint32_t)(i + 1);
}

// One lane per voxel: its points are ord[start[v] .. start[v + 1]), in input order.  The centroid is the sequential double sum divided by
// the count; "first" copies the lowest-index point.  Per cloud: voxels and kept voxels (one atomic pair per run of a cloud in a wave).
static __global__ void __launch_bounds__(kVoxBlock) k_vox_reduce(const float4 *__restrict__ pts, const uint32_t *__restrict__ ord, int64_t n,
                                                                 const uint32_t *__restrict__ seg, const uint32_t *__restrict__ start,
                                                                 const uint32_t *__restrict__ incl, int mode, int min_points,
                                                                 float4 *__restrict__ vout, uint32_t *__restrict__ keep, int64_t *__restrict__ cnt) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_vox = incl[n - 1];
    const bool act = v < n_vox;
    uint32_t s = 0;
    bool k = false;
    if (act) {
        const uint32_t b = start[v], e = start[v + 1];
        const uint32_t o = ord[b];
        s = seg[o];
        k = (int64_t)(e - b) >= (int64_t)min_points;
        float4 q;
        if (mode == DCREG_VOXEL_FIRST) {
            q = pts[o];
        } else {
            const float4 p0 = pts[o];
            double sx = p0.x, sy = p0.y, sz = p0.z;
            for (uint32_t j = b + 1; j < e; ++j) {
                const float4 p = pts[ord[j]];
                sx += (double)p.x; sy += (double)p.y; sz += (double)p.z;
            }
            const double m = (double)(e - b);
            q = make_float4((float)(sx / m), (float)(sy / m), (float)(sz / m), 0.f);
        }
        vout[v] = make_float4(q.x, q.y, q.z, 0.f);
        keep[v] = k ? 1u : 0u;
    } else if (v < n) {
        keep[v] = 0u;              // (the scan of keep runs over n entries)
    }
    // the active lanes are a prefix of the wave and their clouds ascend: a lane whose cloud differs from its left neighbour's starts a run
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t left = __shfl_up(s, 1);
    const bool leader = act && (lane == 0 || left != s);
    const uint64_t L = __ballot(leader), A = __ballot(act), K = __ballot(act && k);
    if (leader) {
        const uint64_t above = lane == 63 ? 0ull : (L & ~((2ull << lane) - 1ull));
        const int end = above ? __ffsll((unsigned long long)above) - 1 : 64 - __clzll((long long)A);     // next run / past the last active lane
        const uint64_t run = (end >= 64 ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
        unsigned long long *c = reinterpret_cast<unsigned long long *>(cnt + (int64_t)kCnt * s);
        atomicAdd(c + 7, (unsigned long long)(end - lane));
        atomicAdd(c + 8, (unsigned long long)__popcll(K & run));
    }
}

// compaction of the kept voxels (pos = exclusive scan of keep): 3 floats per point, or packed as k_pack packs a cloud (w = the point's index)
// with the bounds of the output (ordered-uint atomics, one set per block)
static __global__ void __launch_bounds__(kVoxBlock) k_vox_write(const float4 *__restrict__ vout, const uint32_t *__restrict__ keep,
                                                                const uint32_t *__restrict__ pos, const uint32_t *__restrict__ incl, int64_t n,
                                                                float *__restrict__ out3, float4 *__restrict__ out4, uint32_t *__restrict__ bounds) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_vox = incl[n - 1];
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (v < n_vox && keep[v]) {
        const float4 q = vout[v];
        const uint32_t j = pos[v];
        if (out4) {
            out4[j] = make_float4(q.x, q.y, q.z, __uint_as_float(j));
            const float c[3] = {q.x, q.y, q.z};
            for (int a = 0; a < 3; ++a) { lo[a] = f2ord(c[a]); hi[a] = f2ord(c[a]); }
        } else {
            out3[3 * (int64_t)j] = q.x; out3[3 * (int64_t)j + 1] = q.y; out3[3 * (int64_t)j + 2] = q.z;
        }
    }
    if (!out4) return;             // (grid-uniform)
    for (int o = 32; o > 0; o >>= 1)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (uint32_t)__shfl_xor(lo[a], o)); hi[a] = std::max(hi[a], (uint32_t)__shfl_xor(hi[a], o)); }
    __shared__ uint32_t slo[kVoxBlock / 64][3], shi[kVoxBlock / 64][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) { slo[wave][a] = lo[a]; shi[wave][a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        uint32_t l = slo[0][a], h = shi[0][a];
        for (int w = 1; w < kVoxBlock / 64; ++w) { l = std::min(l, slo[w][a]); h = std::max(h, shi[w][a]); }
        if (l <= h) { atomicMin(&bounds[a], l); atomicMax(&bounds[3 + a], h); }
    }
}

// ---- the kept voxel map (dcreg_target_voxels_keep): k_vox_reduce's shape with the second pass, the eigen-solve and the clamp.  ONE lane
// per voxel: its points are ord[start[v] .. start[v + 1]) in index order, so the sums are left to right; a call pays for its fullest voxel.
// rec: 3 float4 per voxel (context.hpp VoxelMapBufs), written for the kept ones; keep[v] = 1 for those.  cls[0] += voxels below
// min_points, cls[1] += degenerate ones (one atomic pair per wave).  The rule is the header's, operation by operation.
static __global__ void __launch_bounds__(kVoxBlock) k_vmap_reduce(const float4 *__restrict__ pts, const uint32_t *__restrict__ ord, int64_t n_vox,
                                                                  const uint32_t *__restrict__ start, int min_points, double eps,
                                                                  float4 *__restrict__ rec, uint32_t *__restrict__ keep,
                                                                  unsigned long long *__restrict__ cls) {
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool small = false, degenerate = false;
    if (v < n_vox) {
        const uint32_t b = start[v], e = start[v + 1];
        small = (int64_t)(e - b) < (int64_t)min_points;
        bool k = false;
        if (!small) {
            const float4 p0 = pts[ord[b]];
            double sx = p0.x, sy = p0.y, sz = p0.z;
            for (uint32_t j = b + 1; j < e; ++j) {
                const float4 p = pts[ord[j]];
                sx += (double)p.x; sy += (double)p.y; sz += (double)p.z;
            }
            const double m = (double)(e - b);
            const double mx = sx / m, my = sy / m, mz = sz / m;
            // (-0.0 is the identity of the IEEE addition: the sums start with their first term)
            double cxx = -0.0, cxy = -0.0, cxz = -0.0, cyy = -0.0, cyz = -0.0, czz = -0.0;
            for (uint32_t j = b; j < e; ++j) {
                const float4 p = pts[ord[j]];
                const double dx = (double)p.x - mx, dy = (double)p.y - my, dz = (double)p.z - mz;
                cxx = cxx + dx * dx; cxy = cxy + dx * dy; cxz = cxz + dx * dz;
                cyy = cyy + dy * dy; cyz = cyz + dy * dz; czz = czz + dz * dz;
            }
            double a00 = cxx / m, a01 = cxy / m, a02 = cxz / m, a11 = cyy / m, a12 = cyz / m, a22 = czz / m;
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
            for (int sweep = 0; sweep < 6; ++sweep) {
                jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0,1), r = 2
                jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0,2), r = 1
                jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1,2), r = 0
            }
            double lmax = a00;
            if (a11 > lmax) lmax = a11;
            if (a22 > lmax) lmax = a22;
            const double big = 1.7976931348623157e308;
            k = lmax > 0.0 && fabs(a00) <= big && fabs(a11) <= big && fabs(a22) <= big;
            degenerate = !k;
            if (k) {
                double l0 = a00 / lmax, l1 = a11 / lmax, l2 = a22 / lmax;
                if (l0 < eps) l0 = eps;
                if (l1 < eps) l1 = eps;
                if (l2 < eps) l2 = eps;
                // C'_ab = ((V_a0 l_0) V_b0 + (V_a1 l_1) V_b1) + (V_a2 l_2) V_b2, a >= b
                const double c00 = ((v00 * l0) * v00 + (v01 * l1) * v01) + (v02 * l2) * v02;
                const double c10 = ((v10 * l0) * v00 + (v11 * l1) * v01) + (v12 * l2) * v02;
                const double c20 = ((v20 * l0) * v00 + (v21 * l1) * v01) + (v22 * l2) * v02;
                const double c11 = ((v10 * l0) * v10 + (v11 * l1) * v11) + (v12 * l2) * v12;
                const double c21 = ((v20 * l0) * v10 + (v21 * l1) * v11) + (v22 * l2) * v12;
                const double c22 = ((v20 * l0) * v20 + (v21 * l1) * v21) + (v22 * l2) * v22;
                rec[3 * v] = make_float4((float)mx, (float)my, (float)mz, (float)c00);
                rec[3 * v + 1] = make_float4((float)c10, (float)c20, (float)c11, (float)c21);
                rec[3 * v + 2] = make_float4((float)c22, __uint_as_float(e - b), 0.f, 0.f);
            }
        }
        keep[v] = k ? 1u : 0u;
    }
    const uint64_t S = __ballot(small), D = __ballot(degenerate);
    if ((threadIdx.x & 63) == 0) {
        if (S) atomicAdd(cls, (unsigned long long)__popcll(S));
        if (D) atomicAdd(cls + 1, (unsigned long long)__popcll(D));
    }
}

// compaction of the kept voxels (pos = exclusive scan of keep) into the member's arrays, and the fill of the lookup table: the voxel's key
// (its rel key - widths bx, by - repacked to 21 bits per axis) claims the first free slot of its probe sequence with one 64-bit
// atomicCAS; keys are unique, so only slots are contended, and the value is written by the lane that won the slot (the kernels that read
// the table are later launches).  Which slot a key ends in depends on the order of arrival; what a lookup answers does not.
static __global__ void __launch_bounds__(kVoxBlock) k_vmap_write(const float4 *__restrict__ rec, const uint32_t *__restrict__ keep,
                                                                 const uint32_t *__restrict__ pos, int64_t n_vox, const uint32_t *__restrict__ ord,
                                                                 const uint32_t *__restrict__ start, const uint64_t *__restrict__ rel, int bx, int by,
                                                                 float4 *__restrict__ recs, uint64_t *__restrict__ vkeys,
                                                                 uint64_t *__restrict__ t_keys, uint32_t *__restrict__ t_vals, uint32_t mask) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vox || !keep[v]) return;
    const uint32_t j = pos[v];
    recs[3 * (size_t)j] = rec[3 * v]; recs[3 * (size_t)j + 1] = rec[3 * v + 1]; recs[3 * (size_t)j + 2] = rec[3 * v + 2];
    const uint64_t r = rel[ord[start[v]]];
    const uint64_t key = vmap_key(r & ((1ull << bx) - 1ull), (r >> bx) & ((1ull << by) - 1ull), r >> (bx + by));
    vkeys[j] = key;
    uint32_t s = vmap_slot(key, mask);
    for (;;) {                                           // (ends: at most half of the slots are ever claimed)
        const unsigned long long was = atomicCAS(reinterpret_cast<unsigned long long *>(t_keys + s), (unsigned long long)kVmapEmpty, (unsigned long long)key);
        if (was == (unsigned long long)kVmapEmpty) { t_vals[s] = j; break; }
        s = (s + 1u) & mask;
    }
}

// ---- the pairs' voxel maps (pairs_voxels_build): many targets' kept maps from ONE k_vmap_reduce over the voxels of all of them.
// Per-target counters of a build: pc[4 s + 0] voxels, + 1 below min_points, + 2 degenerate, + 3 kept.  One lane per voxel; the voxels
// are in (target, z, y, x) order, so the targets of a wave's active lanes ascend: one atomic set per run of a target in a wave (integer
// atomics: the counts do not depend on the order).  A voxel that is neither small nor kept is degenerate (k_vmap_reduce's rule).
static __global__ void __launch_bounds__(kVoxBlock) k_pvmap_count(const uint32_t *__restrict__ ord, int64_t n_vox, const uint32_t *__restrict__ seg,
                                                                  const uint32_t *__restrict__ start, const uint32_t *__restrict__ keep, int min_points,
                                                                  unsigned long long *__restrict__ pc) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = v < n_vox;
    uint32_t s = 0;
    bool small = false, k = false;
    if (act) {
        const uint32_t b = start[v], e = start[v + 1];
        s = seg[ord[b]];
        small = (int64_t)(e - b) < (int64_t)min_points;
        k = keep[v] != 0u;
    }
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t left = __shfl_up(s, 1);
    const bool leader = act && (lane == 0 || left != s);
    const uint64_t L = __ballot(leader), A = __ballot(act), S = __ballot(act && small), K = __ballot(act && k);
    if (leader) {
        const uint64_t above = lane == 63 ? 0ull : (L & ~((2ull << lane) - 1ull));
        const int end = above ? __ffsll((unsigned long long)above) - 1 : 64 - __clzll((long long)A);     // next run / past the last active lane
        const uint64_t run = (end >= 64 ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull);
        const int n_run = end - lane, n_small = __popcll(S & run), n_kept = __popcll(K & run);
        unsigned long long *p = pc + 4 * (size_t)s;
        atomicAdd(p, (unsigned long long)n_run);
        if (n_small) atomicAdd(p + 1, (unsigned long long)n_small);
        if (n_run - n_small - n_kept) atomicAdd(p + 2, (unsigned long long)(n_run - n_small - n_kept));
        if (n_kept) atomicAdd(p + 3, (unsigned long long)n_kept);
    }
}

// k_vmap_write for many targets: the compaction of the kept voxels (pos = exclusive scan of keep over the voxels of ALL targets: the
// (target, z, y, x) order makes every target's records contiguous and in dcreg_target_voxels_get order, target s from record
// maps[s].first) and the fill of every target's OWN table - maps[s].mask + 1 slots from slot maps[s].base, the key relative to that
// target's minimum voxel, the value the record's number within the target.  The probing is k_vmap_write's: one 64-bit atomicCAS claims
// the first free slot; a target's table is at most half full, so the loop ends inside it.
static __global__ void __launch_bounds__(kVoxBlock) k_pvmap_write(const float4 *__restrict__ rec, const uint32_t *__restrict__ keep,
                                                                  const uint32_t *__restrict__ pos, int64_t n_vox, const uint32_t *__restrict__ ord,
                                                                  const uint32_t *__restrict__ seg, const uint32_t *__restrict__ start,
                                                                  const uint64_t *__restrict__ rel, int bx, int by,
                                                                  const PairVoxMap *__restrict__ maps, float4 *__restrict__ recs,
                                                                  uint64_t *__restrict__ vkeys, uint64_t *__restrict__ t_keys,
                                                                  uint32_t *__restrict__ t_vals) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vox || !keep[v]) return;
    const uint32_t j = pos[v], o = ord[start[v]];
    recs[3 * (size_t)j] = rec[3 * v]; recs[3 * (size_t)j + 1] = rec[3 * v + 1]; recs[3 * (size_t)j + 2] = rec[3 * v + 2];
    const uint64_t r = rel[o];
    const uint64_t key = vmap_key(r & ((1ull << bx) - 1ull), (r >> bx) & ((1ull << by) - 1ull), r >> (bx + by));
    vkeys[j] = key;
    const PairVoxMap m = maps[seg[o]];
    uint64_t *tk = t_keys + m.base;
    uint32_t s = vmap_slot(key, m.mask);
    for (;;) {                                           // (ends: at most half of the target's slots are ever claimed)
        const unsigned long long was = atomicCAS(reinterpret_cast<unsigned long long *>(tk + s), (unsigned long long)kVmapEmpty, (unsigned long long)key);
        if (was == (unsigned long long)kVmapEmpty) { t_vals[m.base + s] = j - m.first; break; }
        s = (s + 1u) & m.mask;
    }
}

template <typename K>
int sort_pairs(dcreg_ctx *c, K *keys_in, K *keys_out, uint32_t *vals_in, uint32_t *vals_out, size_t n, int bits) {
    size_t tmp = 0;
    HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, n, 0, bits, c->stream));
    if (c->sort_tmp.ensure(c, tmp) != DCREG_OK) return DCREG_E_NOMEM;
    HIP_TRY(c, rocprim::radix_sort_pairs(c->sort_tmp.data(), tmp, keys_in, keys_out, vals_in, vals_out, n, 0, bits, c->stream));
    return DCREG_OK;
}

int bits_for(int64_t v) { int b = 0; while (b < 63 && ((int64_t)1 << b) <= v) ++b; return b; }

// Keys, stable sort, voxel heads and starts of the n packed points at pts (k_vox_coords has run: seg and the clouds' minimum voxels in
// B.cnt; bx / by / bz: the key widths of the largest spans).  ord: the points' indices in (cloud, voxel z y x, input) order; B.incl the
// voxel numbers + 1 of the sorted positions, B.start where each voxel starts.  The buffers are the caller's to size (n entries each)
int vox_order(dcreg_ctx *c, const float4 *pts, int64_t n, int n_clouds, double lx, double ly, double lz, int bx, int by, int bz, const uint32_t *&ord) {
    dcreg_ctx::VoxelBufs &B = c->vox;
    int rc;
    const int sbits = bits_for(n_clouds);        // cloud ids 0 .. n_clouds (n_clouds = the non-finite points)
    const bool one_pass = sbits + bx + by + bz <= 64;
    hipLaunchKernelGGL(k_vox_keys, dim3(blocks(n, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, pts, n, B.seg.data(), n_clouds, lx, ly, lz, B.cnt.data(),
                       bx, by, bz, one_pass, c->d_mkeys.data(), c->d_vals.data(), B.rel.data());
    if (one_pass) {
        rc = sort_pairs<uint64_t>(c, c->d_mkeys.data(), c->d_mkeys2.data(), c->d_vals.data(), c->d_vals2.data(), (size_t)n, sbits + bx + by + bz);
        if (rc) return rc;
        ord = c->d_vals2.data();
    } else {            // voxel key first, then the cloud: both sorts stable, so each cloud's voxels and each voxel's points keep their order
        rc = sort_pairs<uint64_t>(c, c->d_mkeys.data(), c->d_mkeys2.data(), c->d_vals.data(), c->d_vals2.data(), (size_t)n, bx + by + bz);
        if (rc) return rc;
        hipLaunchKernelGGL(k_vox_seg_keys, dim3(blocks(n, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, c->d_vals2.data(), n, B.seg.data(), B.head.data());
        rc = sort_pairs<uint32_t>(c, B.head.data(), B.incl.data(), c->d_vals2.data(), c->d_vals.data(), (size_t)n, sbits);
        if (rc) return rc;
        ord = c->d_vals.data();
    }
    hipLaunchKernelGGL(k_vox_heads, dim3(blocks(n, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, ord, n, B.seg.data(), B.rel.data(), (uint32_t)n_clouds, B.head.data());
    rc = scan_u32(c, B.head.data(), B.incl.data(), (size_t)n, true);
    if (rc) return rc;
    hipLaunchKernelGGL(k_vox_starts, dim3(blocks(n, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, ord, n, B.seg.data(), (uint32_t)n_clouds, B.head.data(), B.incl.data(),
                       B.start.data());
    return DCREG_OK;
}

}  // namespace

int voxel_pass(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device, const dcreg_voxel_params *p,
               bool packed, VoxelResult &r, DeskewRun *dsk, const GatherRun *gat) {
    // ---- everything the host can check, before anything is queued
    if (!p) { c->fail("null voxel parameters"); return DCREG_E_INVALID; }
    for (int a = 0; a < 3; ++a)
        if (!(std::isfinite(p->leaf[a]) && p->leaf[a] > 0.0)) { c->fail("voxel leaf %d is %g: finite and > 0 expected", a, p->leaf[a]); return DCREG_E_INVALID; }
    if (p->mode != DCREG_VOXEL_CENTROID && p->mode != DCREG_VOXEL_FIRST) { c->fail("unknown voxel mode %d", p->mode); return DCREG_E_INVALID; }
    if (n_clouds < 0 || (n_clouds > 0 && !off) || stride < 3) { c->fail("invalid cloud arguments"); return DCREG_E_INVALID; }
    if (n_clouds > 0 && off[0] != 0) { c->fail("cloud offsets must start at 0"); return DCREG_E_INVALID; }
    for (int s = 0; s < n_clouds; ++s)
        if (off[s + 1] < off[s]) { c->fail("cloud offsets decrease at cloud %d", s); return DCREG_E_INVALID; }
    const int64_t n = n_clouds > 0 ? off[n_clouds] : 0;
    if (n >= ((int64_t)1 << 31) - 1) { c->fail("too many points for one voxel pass (%lld)", (long long)n); return DCREG_E_INVALID; }
    if (n > 0 && !xyz && !gat) { c->fail("null point buffer"); return DCREG_E_INVALID; }      // (gat: the points come from the keyframe store)
    if (packed && n_clouds != 1) { c->fail("a packed voxel output holds one cloud"); return DCREG_E_INVALID; }
    const int min_points = std::max(p->min_points, 1);
    r = VoxelResult();
    r.voxels.assign((size_t)n_clouds, 0);
    r.kept.assign((size_t)n_clouds, 0);
    r.n_in = n;
    if (n == 0) return DCREG_OK;

    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::VoxelBufs &B = c->vox;
    const size_t nc = (size_t)kCnt * n_clouds + kTail;
    if (B.seg.ensure(c, (size_t)n) || B.rel.ensure(c, (size_t)n) || B.head.ensure(c, (size_t)n) ||
        B.incl.ensure(c, (size_t)n) || B.start.ensure(c, (size_t)n + 1) || B.keep.ensure(c, (size_t)n) ||
        B.pos.ensure(c, (size_t)n) || B.vout.ensure(c, (size_t)n) || B.d_off.ensure(c, (size_t)n_clouds + 1) ||
        B.cnt.ensure(c, nc) || c->d_mkeys.ensure(c, (size_t)n) || c->d_mkeys2.ensure(c, (size_t)n) ||
        c->d_vals.ensure(c, (size_t)n) || c->d_vals2.ensure(c, (size_t)n))
        return DCREG_E_NOMEM;
    if (packed ? c->d_aligned.ensure(c, (size_t)n) : B.out.ensure(c, (size_t)(3 * n))) return DCREG_E_NOMEM;
    int rc = upload_cloud(c, xyz, n, stride, on_device, B.pts, dsk, gat);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(B.d_off.data(), off, sizeof(int64_t) * ((size_t)n_clouds + 1), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_vox_init, dim3(blocks((int64_t)nc * 2, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, B.cnt.data(), n_clouds);
    const double lx = p->leaf[0], ly = p->leaf[1], lz = p->leaf[2];
    hipLaunchKernelGGL(k_vox_coords, dim3(blocks(n, kVoxBlock * kVoxPerThread)), dim3(kVoxBlock), 0, c->stream, B.pts.data(), n, B.d_off.data(), n_clouds,
                       lx, ly, lz, B.seg.data(), B.cnt.data());
    std::vector<int64_t> h((size_t)nc);
    HIP_TRY(c, hipMemcpyAsync(h.data(), B.cnt.data(), sizeof(int64_t) * nc, hipMemcpyDeviceToHost, c->stream));
    if (dsk && (rc = deskew_readback(c, *dsk))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());

    // ---- spans: refusals, key widths
    uint32_t tail[2 * kTail];
    std::memcpy(tail, h.data() + (size_t)kCnt * n_clouds, sizeof(tail));
    if (tail[6]) { c->fail("a voxel coordinate reaches 2^62 (leaf too small for the coordinates)"); return DCREG_E_INVALID; }
    int64_t span[3] = {0, 0, 0};
    for (int s = 0; s < n_clouds; ++s) {
        const int64_t *q = h.data() + (size_t)kCnt * s;
        if (q[6] == 0) continue;
        r.n_finite += q[6];
        for (int a = 0; a < 3; ++a) {
            const int64_t d = q[3 + a] - q[a];
            if (d + 1 > kSpanMax) {                           // (d = maximum - minimum: d + 1 voxels)
                c->fail("cloud %d spans %lld voxels on axis %d (at most 2^21 - 1 = %lld)", s, (long long)d + 1, a, (long long)kSpanMax);
                return DCREG_E_INVALID;
            }
            span[a] = std::max(span[a], d);
        }
    }
    if (r.n_finite == 0) return DCREG_OK;
    const int bx = bits_for(span[0]), by = bits_for(span[1]), bz = bits_for(span[2]);

    // ---- keys, stable sort, voxel heads and starts
    const uint32_t *ord;
    rc = vox_order(c, B.pts.data(), n, n_clouds, lx, ly, lz, bx, by, bz, ord);
    if (rc) return rc;
    // ---- one lane per voxel (at most n of them: the grids are sized for n, the lanes beyond the voxel count idle), compaction
    hipLaunchKernelGGL(k_vox_reduce, dim3(blocks(n, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, B.pts.data(), ord, n, B.seg.data(), B.start.data(), B.incl.data(), p->mode,
                       min_points, B.vout.data(), B.keep.data(), B.cnt.data());
    rc = scan_u32(c, B.keep.data(), B.pos.data(), (size_t)n, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_vox_write, dim3(blocks(n, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, B.vout.data(), B.keep.data(), B.pos.data(), B.incl.data(), n,
                       packed ? nullptr : B.out.data(), packed ? c->d_aligned.data() : nullptr,
                       reinterpret_cast<uint32_t *>(B.cnt.data() + (size_t)kCnt * n_clouds));
    HIP_TRY(c, hipMemcpyAsync(h.data(), B.cnt.data(), sizeof(int64_t) * nc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    for (int s = 0; s < n_clouds; ++s) {
        r.voxels[(size_t)s] = h[(size_t)kCnt * s + 7];
        r.kept[(size_t)s] = h[(size_t)kCnt * s + 8];
        r.n_voxels += r.voxels[(size_t)s];
        r.n_out += r.kept[(size_t)s];
    }
    std::memcpy(tail, h.data() + (size_t)kCnt * n_clouds, sizeof(tail));
    for (int a = 0; a < 3; ++a) { r.mn[a] = ord2f(tail[a]); r.mx[a] = ord2f(tail[3 + a]); }
    return DCREG_OK;
}

// dcreg_voxel_downsample* (and dcreg_deskew* with a voxel block): the pass into the context's output buffer, then - when the caller's capacity
// holds it - one copy to the caller
int voxel_downsample_to(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device, const dcreg_voxel_params *p,
                        float *out, int64_t capacity, int64_t *out_off, dcreg_voxel_info *info, DeskewRun *dsk) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (!out_off || capacity < 0) { c->fail("invalid output arguments"); return DCREG_E_INVALID; }
    VoxelResult r;
    int rc = voxel_pass(c, n_clouds, xyz, off, stride, on_device, p, false, r, dsk);
    if (rc) return rc;
    out_off[0] = 0;
    for (int s = 0; s < n_clouds; ++s) out_off[s + 1] = out_off[s] + r.kept[(size_t)s];
    if (info) { info->n_in = r.n_in; info->n_finite = r.n_finite; info->n_voxels = r.n_voxels; info->n_out = r.n_out; }
    if (r.n_out > capacity) { c->fail("the output holds %lld points, the capacity is %lld", (long long)r.n_out, (long long)capacity); return DCREG_E_INVALID; }
    if (r.n_out == 0) return DCREG_OK;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if ((rc = caller_out(c, out, c->vox.out.data(), sizeof(float) * 3 * (size_t)r.n_out, on_device))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

// dcreg_target_voxels_keep: the whole map's points (index order, all finite) as one cloud through the pass's keying and sort, then the
// records, their compaction and the table.  Everything is built beside the member; it is replaced once the last launch has run.
int voxel_map_keep(dcreg_ctx *c, const dcreg_voxel_map_params *p, dcreg_voxel_map_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (!p) { c->fail("null voxel map parameters"); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->leaf) && p->leaf > 0.0)) { c->fail("voxel map leaf is %g: finite and > 0 expected", p->leaf); return DCREG_E_INVALID; }
    if (!(p->epsilon >= 1.0e-6 && p->epsilon <= 1.0)) { c->fail("voxel map epsilon is %g: 1e-6 .. 1 expected", p->epsilon); return DCREG_E_INVALID; }
    if (p->min_points < 2) { c->fail("voxel map min_points is %d: at least 2 expected", p->min_points); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    const dcreg_ctx::IndexSet &wm = c->roi_active ? c->roi_store : c->map;
    const int64_t n = wm.n;
    if (n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::VoxelBufs &B = c->vox;
    dcreg_ctx::VoxelMapBufs &M = c->vmap;
    const size_t nc = (size_t)kCnt + kTail;
    if (B.seg.ensure(c, (size_t)n) || B.rel.ensure(c, (size_t)n) || B.head.ensure(c, (size_t)n) || B.incl.ensure(c, (size_t)n) ||
        B.start.ensure(c, (size_t)n + 1) || B.keep.ensure(c, (size_t)n) || B.pos.ensure(c, (size_t)n) || B.d_off.ensure(c, 2) ||
        B.cnt.ensure(c, nc) || c->d_mkeys.ensure(c, (size_t)n) || c->d_mkeys2.ensure(c, (size_t)n) || c->d_vals.ensure(c, (size_t)n) ||
        c->d_vals2.ensure(c, (size_t)n) || M.cls.ensure(c, 2))
        return DCREG_E_NOMEM;
    const float4 *pts = wm.raw.data();
    const int64_t off[2] = {0, n};
    HIP_TRY(c, hipMemcpyAsync(B.d_off.data(), off, sizeof(off), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(M.cls.data(), 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_vox_init, dim3(blocks((int64_t)nc * 2, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, B.cnt.data(), 1);
    const double l = p->leaf;
    hipLaunchKernelGGL(k_vox_coords, dim3(blocks(n, kVoxBlock * kVoxPerThread)), dim3(kVoxBlock), 0, c->stream, pts, n, B.d_off.data(), 1, l, l, l, B.seg.data(),
                       B.cnt.data());
    int64_t h[kCnt + kTail];
    HIP_TRY(c, hipMemcpyAsync(h, B.cnt.data(), sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    // ---- the voxel pass's limits
    uint32_t tail[2 * kTail];
    std::memcpy(tail, h + kCnt, sizeof(tail));
    if (tail[6]) { c->fail("a voxel coordinate reaches 2^62 (leaf too small for the coordinates)"); return DCREG_E_INVALID; }
    int bits[3];
    for (int a = 0; a < 3; ++a) {
        const int64_t d = h[3 + a] - h[a];
        if (d + 1 > kSpanMax) {                               // (d = maximum - minimum: d + 1 voxels)
            c->fail("the map spans %lld voxels on axis %d (at most 2^21 - 1 = %lld)", (long long)d + 1, a, (long long)kSpanMax);
            return DCREG_E_INVALID;
        }
        bits[a] = bits_for(d);
    }
    const uint32_t *ord;
    int rc = vox_order(c, pts, n, 1, l, l, l, bits[0], bits[1], bits[2], ord);
    if (rc) return rc;
    uint32_t n_vox32 = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_vox32, B.incl.data() + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const int64_t n_vox = n_vox32;
    // ---- one lane per voxel, then the kept ones' count
    if (M.tmp.ensure(c, 3 * (size_t)n_vox)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_vmap_reduce, dim3(blocks(n_vox, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, pts, ord, n_vox, B.start.data(), p->min_points, p->epsilon,
                       M.tmp.data(), B.keep.data(), M.cls.data());
    rc = scan_u32(c, B.keep.data(), B.pos.data(), (size_t)n_vox, false);
    if (rc) return rc;
    unsigned long long cls[2] = {0, 0};
    uint32_t last[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(cls, M.cls.data(), sizeof(cls), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&last[0], B.keep.data() + (n_vox - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&last[1], B.pos.data() + (n_vox - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const int64_t n_kept = (int64_t)last[0] + (int64_t)last[1];
    if (info) { info->n_points = n; info->n_voxels = n_vox; info->n_small = (int64_t)cls[0]; info->n_degenerate = (int64_t)cls[1]; info->n_kept = n_kept; }
    M.kept = false; M.n_kept = 0;                      // (the member's arrays are rewritten from here on: a failure leaves none)
    if (n_kept == 0) return DCREG_OK;                  // (nothing to keep: no member)
    // ---- the member: records, keys, and a table of the power of two at or above 2 n_kept slots
    size_t slots = 2;
    while (slots < 2 * (size_t)n_kept) slots <<= 1;
    if (M.recs.ensure(c, 3 * (size_t)n_kept) || M.vkeys.ensure(c, (size_t)n_kept) || M.t_keys.ensure(c, slots) || M.t_vals.ensure(c, slots)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(M.t_keys.data(), 0xFF, slots * sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_vmap_write, dim3(blocks(n_vox, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, M.tmp.data(), B.keep.data(), B.pos.data(), n_vox, ord, B.start.data(),
                       B.rel.data(), bits[0], bits[1], M.recs.data(), M.vkeys.data(), M.t_keys.data(), M.t_vals.data(), (uint32_t)(slots - 1));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    for (int a = 0; a < 3; ++a) { M.mn[a] = h[a]; M.mx[a] = h[3 + a]; }
    M.leaf = l; M.mask = (uint32_t)(slots - 1); M.n_kept = n_kept; M.kept = true;
    M.params = *p;                                     // (the rule a followed update refits with: "voxels_follow")
    return DCREG_OK;
}

// dcreg_target_voxels_get: the member's records and keys to the host, unpacked there
static int voxel_map_get(dcreg_ctx *c, int64_t *coords, int32_t *count, float *mean, float *cov, int64_t capacity) {
    if (!c) return DCREG_E_INVALID;
    if (!coords || !count || !mean || !cov) { c->fail("null argument"); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    const dcreg_ctx::VoxelMapBufs &M = c->vmap;
    if (!M.kept) { c->fail("no kept voxels: dcreg_target_voxels_keep first"); return DCREG_E_STATE; }
    if (capacity < M.n_kept) { c->fail("the output holds %lld voxels, the map keeps %lld", (long long)capacity, (long long)M.n_kept); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nk = (size_t)M.n_kept;
    std::vector<float> rec(12 * nk);
    std::vector<uint64_t> keys(nk);
    HIP_TRY(c, hipMemcpyAsync(rec.data(), M.recs.data(), sizeof(float) * 12 * nk, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(keys.data(), M.vkeys.data(), sizeof(uint64_t) * nk, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t am = (1ull << kVmapAxisBits) - 1ull;
    for (size_t j = 0; j < nk; ++j) {
        const float *r = rec.data() + 12 * j;
        coords[3 * j] = M.mn[0] + (int64_t)(keys[j] & am);
        coords[3 * j + 1] = M.mn[1] + (int64_t)((keys[j] >> kVmapAxisBits) & am);
        coords[3 * j + 2] = M.mn[2] + (int64_t)(keys[j] >> (2 * kVmapAxisBits));
        std::memcpy(mean + 3 * j, r, 3 * sizeof(float));
        std::memcpy(cov + 6 * j, r + 3, 6 * sizeof(float));
        std::memcpy(count + j, r + 9, sizeof(int32_t));
    }
    return DCREG_OK;
}

// ------------------------------------------------------------------------------------------ the kept voxel map follows the map ("voxels_follow")
// A voxel's record is a function of its points in index order (k_vmap_reduce), and an update appends points or removes some and renumbers
// the survivors in their old order: the records of the voxels that hold no added and no removed point are what a fresh keep computes,
// bit for bit.  The others - the "touched" voxels - are reduced again from ALL of their points in the updated map:
//   k_vfollow_box    one lane per changed point: the voxel box of the changed points (= the touched voxels' box), per wave before the atomics
//   k_vfollow_mark   one lane per changed point: its voxel, relative to the union of that box and the member's, claims a slot of the touched set
//   k_vfollow_flags  the ONLY pass over the updated map (16 B read per point): the points in touched voxels, and the map's new voxel box
//   scan, k_vfollow_gather   those points, compacted in index order: a cloud that vox_order + k_vmap_reduce take as they take a map
//   k_vfollow_carry  one lane per old record: touched = it goes, else it is carried
//   k_vfollow_runs   the two sorted runs of the merge - carried records and the subset's kept voxels - with keys relative to the NEW minimum
//   k_vfollow_write  one lane per record of either run: its place = its rank in its run + the keys below it in the other run (keys are
//                    unique across the runs: a touched voxel is never carried); the record, its key and its slot of a fresh table
// Keys order as voxels do (z y x) whatever minimum they are relative to, so both runs ascend and the merged records are in _get order.
namespace {

constexpr int kVfOvf = 6, kVfDistinct = 7, kVfNew = 8, kVfWords = 16;   // f_cnt: [0..5] the changed points' voxel box, [8..13] the updated map's
struct VfBox { long long lo[3], hi[3]; };

// k_vox_coords' voxel of a finite point as integers; false: a coordinate reaches 2^62 (the pass's refusal)
__device__ __forceinline__ bool voxel_int(const float4 p, const double l, long long vi[3]) {
    double v[3];
    voxel_of(p, l, l, l, v);
    const bool ok = fabs(v[0]) < kVoxLimit && fabs(v[1]) < kVoxLimit && fabs(v[2]) < kVoxLimit;
    for (int a = 0; a < 3; ++a) vi[a] = ok ? (long long)v[a] : 0;
    return ok;
}
__device__ __forceinline__ bool vf_inside(const long long vi[3], const VfBox &b) {
    return vi[0] >= b.lo[0] && vi[0] <= b.hi[0] && vi[1] >= b.lo[1] && vi[1] <= b.hi[1] && vi[2] >= b.lo[2] && vi[2] <= b.hi[2];
}
__device__ __forceinline__ uint64_t vf_key(const long long vi[3], const long long mn[3]) {
    return vmap_key((uint64_t)(vi[0] - mn[0]), (uint64_t)(vi[1] - mn[1]), (uint64_t)(vi[2] - mn[2]));
}
// is the key in the touched set (the probing of vmap_find_voxel: the set is at most half full)
__device__ __forceinline__ bool vf_touched(const uint64_t *__restrict__ set, uint32_t mask, uint64_t key) {
    uint32_t s = vmap_slot(key, mask);
    for (;;) {
        const uint64_t k = set[s];
        if (k == key) return true;
        if (k == kVmapEmpty) return false;
        s = (s + 1u) & mask;
    }
}
__device__ __forceinline__ void vf_wave_box(long long mn[3], long long mx[3]) {
    for (int o = 32; o > 0; o >>= 1)
        for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], (long long)__shfl_xor(mn[a], o)); mx[a] = std::max(mx[a], (long long)__shfl_xor(mx[a], o)); }
}

// keep != null: the points whose flag is set stay - only the others changed
static __global__ void __launch_bounds__(kVoxBlock) k_vfollow_box(const float4 *__restrict__ pts, int64_t n, const uint32_t *__restrict__ keep, double leaf,
                                                                  long long *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < n && !(keep && keep[i] != 0u);
    long long mn[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, mx[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    bool big = false;
    if (on) {
        long long vi[3];
        big = !voxel_int(pts[i], leaf, vi);
        if (!big)
            for (int a = 0; a < 3; ++a) { mn[a] = vi[a]; mx[a] = vi[a]; }
    }
    const uint64_t any = __ballot(on && !big), B = __ballot(big);
    if (!any && !B) return;                // (wave-uniform)
    vf_wave_box(mn, mx);
    if ((threadIdx.x & 63) == 0) {
        if (B) atomicOr(reinterpret_cast<unsigned long long *>(cnt + kVfOvf), 1ull);
        // (a removal brings millions of points and every wave's six atomics meet at the same words: a plain look first - the words only
        // ever move outwards, so a stale value can cost an atomic and never skips one that is needed)
        if (any)
            for (int a = 0; a < 3; ++a) {
                if (mn[a] < *reinterpret_cast<volatile long long *>(cnt + a)) atomicMin(cnt + a, mn[a]);
                if (mx[a] > *reinterpret_cast<volatile long long *>(cnt + 3 + a)) atomicMax(cnt + 3 + a, mx[a]);
            }
    }
}

// The touched set: a changed point's voxel, relative to the union of the member's box `old` and the changed points' box (the old box for
// a removal, the new one for an insert: one contains the other), claims the first free slot of its probe sequence with k_vmap_write's
// 64-bit atomicCAS; a lane that meets its own key stops.  The claims are the distinct touched voxels: counted per wave.  A union of
// 2^21 voxels on an axis or a coordinate of 2^62 marks nothing (grid-uniform; the host refuses from the same words)
static __global__ void __launch_bounds__(kVoxBlock) k_vfollow_mark(const float4 *__restrict__ pts, int64_t n, const uint32_t *__restrict__ keep, double leaf,
                                                                   VfBox old, long long *cnt, uint64_t *__restrict__ set, uint32_t mask) {
    long long u[3];
    bool bad = cnt[kVfOvf] != 0;
    for (int a = 0; a < 3; ++a) {
        u[a] = std::min(old.lo[a], cnt[a]);
        bad |= std::max(old.hi[a], cnt[3 + a]) - u[a] + 1 > kSpanMax;
    }
    if (bad) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool won = false;
    if (i < n && !(keep && keep[i] != 0u)) {
        long long vi[3];
        (void)voxel_int(pts[i], leaf, vi);
        const uint64_t key = vf_key(vi, u);
        uint32_t s = vmap_slot(key, mask);
        for (;;) {                                       // (ends: at most half of the slots are ever claimed)
            // a plain look first: a removal sends thousands of lanes to one voxel's slot, and all but the first find its key there
            // without an atomic (a slot never changes once claimed; a stale "empty" only costs the CAS)
            unsigned long long was = *reinterpret_cast<volatile unsigned long long *>(set + s);
            if (was == (unsigned long long)kVmapEmpty)
                was = atomicCAS(reinterpret_cast<unsigned long long *>(set + s), (unsigned long long)kVmapEmpty, (unsigned long long)key);
            if (was == (unsigned long long)kVmapEmpty) { won = true; break; }
            if (was == (unsigned long long)key) break;
            s = (s + 1u) & mask;
        }
    }
    const uint64_t W = __ballot(won);
    if (W && (threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(cnt + kVfDistinct), (unsigned long long)__popcll(W));
}

// The pass over the updated map, k_vox_coords' tile shape: flag[i] = point i lies in a touched voxel (n + 1 entries, the last 0) - its
// voxel, the early-out against the touched voxels' box `tb`, then the probe - and the voxel box of all points (the member's new box)
static __global__ void __launch_bounds__(kVoxBlock) k_vfollow_flags(const float4 *__restrict__ pts, int64_t n, double leaf, VfBox uni, VfBox tb,
                                                                    const uint64_t *__restrict__ set, uint32_t mask, uint32_t *__restrict__ flag,
                                                                    long long *__restrict__ cnt) {
    const int64_t base = (int64_t)blockIdx.x * (kVoxBlock * kVoxPerThread);
    long long mn[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, mx[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
    for (int k = 0; k < kVoxPerThread; ++k) {
        const int64_t i = base + threadIdx.x + (int64_t)k * kVoxBlock;
        if (i > n) break;
        if (i == n) { flag[i] = 0u; break; }
        const float4 p = pts[i];
        long long vi[3];
        bool hit = false;
        if (voxel_int(p, leaf, vi)) {
            for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], vi[a]); mx[a] = std::max(mx[a], vi[a]); }
            hit = vf_inside(vi, tb) && vf_touched(set, mask, vf_key(vi, uni.lo));
        }
        flag[i] = hit ? 1u : 0u;
    }
    vf_wave_box(mn, mx);
    __shared__ long long smn[kVoxBlock / 64][3], smx[kVoxBlock / 64][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) { smn[wave][a] = mn[a]; smx[wave][a] = mx[a]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        long long l = smn[0][a], h = smx[0][a];
        for (int w = 1; w < kVoxBlock / 64; ++w) { l = std::min(l, smn[w][a]); h = std::max(h, smx[w][a]); }
        if (l <= h) { atomicMin(cnt + kVfNew + a, l); atomicMax(cnt + kVfNew + 3 + a, h); }
    }
}

// the points of the touched voxels, compacted in index order (pos = exclusive scan of flag)
static __global__ void k_vfollow_gather(const float4 *__restrict__ pts, int64_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                        float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    out[pos[i]] = pts[i];
}

__device__ __forceinline__ void vf_unpack(uint64_t key, const long long mn[3], long long vi[3]) {
    const uint64_t am = (1ull << kVmapAxisBits) - 1ull;
    vi[0] = mn[0] + (long long)(key & am);
    vi[1] = mn[1] + (long long)((key >> kVmapAxisBits) & am);
    vi[2] = mn[2] + (long long)(key >> (2 * kVmapAxisBits));
}

// cflag[j] = 1: old record j is carried - its voxel (the member's minimum + its key) holds no changed point (nk + 1 entries, the last 0)
static __global__ void k_vfollow_carry(const uint64_t *__restrict__ vkeys, int64_t nk, VfBox old, VfBox uni, VfBox tb, const uint64_t *__restrict__ set,
                                       uint32_t mask, uint32_t *__restrict__ cflag) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nk) return;
    if (j == nk) { cflag[j] = 0u; return; }
    long long vi[3];
    vf_unpack(vkeys[j], old.lo, vi);
    const bool touched = vf_inside(vi, tb) && vf_touched(set, mask, vf_key(vi, uni.lo));
    cflag[j] = touched ? 0u : 1u;
}

// The runs of the merge.  Lanes [0, nk): a carried record's key, rewritten relative to the new minimum `nw`, and its number, at its rank
// cpos.  Lanes [nk, nk + n_vox): a kept voxel of the subset - its rel key (widths bx, by, relative to tb's minimum, as vox_order was
// given it) rewritten the same way - and its number in the uncompacted records, at its rank pos
static __global__ void k_vfollow_runs(const uint64_t *__restrict__ vkeys, int64_t nk, const uint32_t *__restrict__ cflag, const uint32_t *__restrict__ cpos,
                                      VfBox old, VfBox nw, int64_t n_vox, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos,
                                      const uint32_t *__restrict__ ord, const uint32_t *__restrict__ start, const uint64_t *__restrict__ rel, int bx, int by,
                                      VfBox tb, uint64_t *__restrict__ akeys, uint32_t *__restrict__ asrc, uint64_t *__restrict__ bkeys,
                                      uint32_t *__restrict__ bsrc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    long long vi[3];
    if (i < nk) {
        if (!cflag[i]) return;
        vf_unpack(vkeys[i], old.lo, vi);
        const uint32_t r = cpos[i];
        akeys[r] = vf_key(vi, nw.lo); asrc[r] = (uint32_t)i;
    } else {
        const int64_t v = i - nk;
        if (v >= n_vox || !keep[v]) return;
        const uint64_t q = rel[ord[start[v]]];
        vi[0] = tb.lo[0] + (long long)(q & ((1ull << bx) - 1ull));
        vi[1] = tb.lo[1] + (long long)((q >> bx) & ((1ull << by) - 1ull));
        vi[2] = tb.lo[2] + (long long)(q >> (bx + by));
        const uint32_t r = pos[v];
        bkeys[r] = vf_key(vi, nw.lo); bsrc[r] = (uint32_t)v;
    }
}

// Merge and write: lane i < n_a is carried record i of run a (from the member's records), the others the kept voxels of run b (from the
// subset's uncompacted records).  Place = rank in the own run + the other run's keys below the own key (binary search); then the record,
// its key, and its slot of the fresh table by k_vmap_write's probing
static __global__ void __launch_bounds__(kVoxBlock) k_vfollow_write(int64_t n_a, int64_t n_b, const uint64_t *__restrict__ akeys, const uint32_t *__restrict__ asrc,
                                                                    const uint64_t *__restrict__ bkeys, const uint32_t *__restrict__ bsrc,
                                                                    const float4 *__restrict__ recs_old, const float4 *__restrict__ tmp,
                                                                    float4 *__restrict__ recs, uint64_t *__restrict__ vkeys, uint64_t *__restrict__ t_keys,
                                                                    uint32_t *__restrict__ t_vals, uint32_t mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_a + n_b) return;
    const bool own_a = i < n_a;
    const int64_t r = own_a ? i : i - n_a;
    const uint64_t key = own_a ? akeys[r] : bkeys[r];
    const uint64_t *other = own_a ? bkeys : akeys;
    int64_t lo = 0, hi = own_a ? n_b : n_a;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (other[mid] < key) lo = mid + 1; else hi = mid;
    }
    const uint32_t j = (uint32_t)(r + lo);
    const float4 *src = own_a ? recs_old + 3 * (size_t)asrc[r] : tmp + 3 * (size_t)bsrc[r];
    recs[3 * (size_t)j] = src[0]; recs[3 * (size_t)j + 1] = src[1]; recs[3 * (size_t)j + 2] = src[2];
    vkeys[j] = key;
    uint32_t s = vmap_slot(key, mask);
    for (;;) {                                           // (ends: at most half of the slots are ever claimed)
        const unsigned long long was = atomicCAS(reinterpret_cast<unsigned long long *>(t_keys + s), (unsigned long long)kVmapEmpty, (unsigned long long)key);
        if (was == (unsigned long long)kVmapEmpty) { t_vals[s] = j; break; }
        s = (s + 1u) & mask;
    }
}

// scratch that grows with the map from keyframe to keyframe: an eighth of headroom, so that not every update allocates again
template <typename T>
int vf_ensure(dcreg_ctx *c, DevBuf<T> &b, size_t need) { return b.holds(need) ? DCREG_OK : b.ensure(c, need + need / 8 + 4096); }

// A followed update.  FIVE stream synchronises on the incremental path (the touched box and count; the hits and the new box; the subset's
// voxels; the two runs' lengths; the end).  Every array of the next member is written beside the current one and swapped in last
int follow_run(dcreg_ctx *c, const FollowChange &ch) {
    dcreg_ctx::VoxelBufs &B = c->vox;
    dcreg_ctx::VoxelMapBufs &M = c->vmap;
    const int64_t n = c->map.n, nk = M.n_kept;
    if (n <= 0 || nk <= 0 || c->roi_active) { c->fail("the kept voxel map cannot follow: the whole map's index is not the active one"); return DCREG_E_STATE; }
    const bool removal = ch.n_old > 0;
    const float4 *cpts = removal ? ch.old_raw : ch.added;
    const uint32_t *ckeep = removal ? ch.flag_r : nullptr;
    const int64_t n_c = removal ? ch.n_old : ch.n_added, n_changed = removal ? ch.n_old - n : ch.n_added;
    if (!cpts || n_changed <= 0 || (removal && !ckeep)) { c->fail("the kept voxel map cannot follow: no change given"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    const dcreg_voxel_map_params prm = M.params;
    const double l = prm.leaf;
    dcreg_voxels_follow_info &F = M.follow;
    // ---- the touched voxels
    size_t fslots = 2;
    while (fslots < 2 * (size_t)n_changed) fslots <<= 1;
    if (M.f_set.ensure(c, fslots) || M.f_cnt.ensure(c, kVfWords)) return DCREG_E_NOMEM;
    long long h[kVfWords] = {};
    for (int a = 0; a < 3; ++a) { h[a] = INT64_MAX; h[3 + a] = INT64_MIN; h[kVfNew + a] = INT64_MAX; h[kVfNew + 3 + a] = INT64_MIN; }
    HIP_TRY(c, hipMemcpyAsync(M.f_cnt.data(), h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(M.f_set.data(), 0xFF, fslots * sizeof(uint64_t), c->stream));
    VfBox old, tb, uni, nw;
    for (int a = 0; a < 3; ++a) { old.lo[a] = M.mn[a]; old.hi[a] = M.mx[a]; }
    const uint32_t fmask = (uint32_t)(fslots - 1);
    hipLaunchKernelGGL(k_vfollow_box, dim3(blocks(n_c, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, cpts, n_c, ckeep, l, M.f_cnt.data());
    hipLaunchKernelGGL(k_vfollow_mark, dim3(blocks(n_c, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, cpts, n_c, ckeep, l, old, M.f_cnt.data(), M.f_set.data(), fmask);
    HIP_TRY(c, hipMemcpyAsync(h, M.f_cnt.data(), sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    // ---- the keep's limits, on the union box (an insert's union is the updated map's box; a removal's is the member's, which passed)
    if (h[kVfOvf]) { c->fail("a voxel coordinate reaches 2^62 (leaf too small for the coordinates): the kept voxel map is dropped"); return DCREG_E_INVALID; }
    for (int a = 0; a < 3; ++a) {
        tb.lo[a] = h[a]; tb.hi[a] = h[3 + a];
        uni.lo[a] = std::min(old.lo[a], tb.lo[a]); uni.hi[a] = std::max(old.hi[a], tb.hi[a]);
        if (uni.hi[a] - uni.lo[a] + 1 > kSpanMax) {
            c->fail("the map spans %lld voxels on axis %d (at most 2^21 - 1 = %lld): the kept voxel map is dropped", (long long)(uni.hi[a] - uni.lo[a] + 1), a,
                    (long long)kSpanMax);
            return DCREG_E_INVALID;
        }
    }
    F.n_touched = h[kVfDistinct];
    // ---- the one pass over the updated map: the points in touched voxels (flag and its scan in the voxel pass's head / incl), the new box
    const float4 *pts = c->map.raw.data();
    const size_t n1 = (size_t)n + 1;
    if (vf_ensure(c, B.head, n1) || vf_ensure(c, B.incl, n1)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_vfollow_flags, dim3(blocks((int64_t)n1, kVoxBlock * kVoxPerThread)), dim3(kVoxBlock), 0, c->stream, pts, n, l, uni, tb, M.f_set.data(), fmask,
                       B.head.data(), M.f_cnt.data());
    int rc = scan_u32(c, B.head.data(), B.incl.data(), n1, false);
    if (rc) return rc;
    uint32_t n_hit32 = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_hit32, B.incl.data() + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h, M.f_cnt.data(), sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const int64_t n_hit = n_hit32;
    for (int a = 0; a < 3; ++a) { nw.lo[a] = h[kVfNew + a]; nw.hi[a] = h[kVfNew + 3 + a]; }
    if ((double)n_hit > c->opt_voxels_follow_full_share * (double)n) {      // past the share: the keep itself, with the same bits
        dcreg_voxel_map_info info{};
        rc = voxel_map_keep(c, &prm, &info);
        if (rc) return rc;
        F.n_refit = info.n_voxels; F.n_carried = 0; F.n_kept = info.n_kept; F.followed = 2;
        return DCREG_OK;
    }
    // ---- the subset through the keep's order and reduction, unchanged: one cloud, keys relative to the touched box's minimum
    int64_t n_vox = 0;
    int bits[3] = {0, 0, 0};
    const uint32_t *ord = nullptr;
    if (n_hit > 0) {
        const size_t nc = (size_t)kCnt + kTail;
        if (vf_ensure(c, M.f_sub, (size_t)n_hit) || vf_ensure(c, B.seg, (size_t)n_hit) || vf_ensure(c, B.rel, (size_t)n_hit) ||
            vf_ensure(c, B.start, (size_t)n_hit + 1) || vf_ensure(c, B.keep, (size_t)n_hit) || vf_ensure(c, B.pos, (size_t)n_hit) || B.cnt.ensure(c, nc) ||
            vf_ensure(c, c->d_mkeys, (size_t)n_hit) || vf_ensure(c, c->d_mkeys2, (size_t)n_hit) || vf_ensure(c, c->d_vals, (size_t)n_hit) ||
            vf_ensure(c, c->d_vals2, (size_t)n_hit) || M.cls.ensure(c, 2))
            return DCREG_E_NOMEM;
        hipLaunchKernelGGL(k_vfollow_gather, dim3(blocks(n, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, pts, n, B.head.data(), B.incl.data(), M.f_sub.data());
        int64_t hc[kCnt + kTail] = {};
        for (int a = 0; a < 3; ++a) { hc[a] = tb.lo[a]; hc[3 + a] = tb.hi[a]; bits[a] = bits_for(tb.hi[a] - tb.lo[a]); }
        HIP_TRY(c, hipMemcpyAsync(B.cnt.data(), hc, sizeof(hc), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(B.seg.data(), 0, (size_t)n_hit * sizeof(uint32_t), c->stream));       // (all of cloud 0)
        HIP_TRY(c, hipMemsetAsync(M.cls.data(), 0, 2 * sizeof(unsigned long long), c->stream));
        rc = vox_order(c, M.f_sub.data(), n_hit, 1, l, l, l, bits[0], bits[1], bits[2], ord);
        if (rc) return rc;
        uint32_t n_vox32 = 0;
        HIP_TRY(c, hipMemcpyAsync(&n_vox32, B.incl.data() + (n_hit - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        n_vox = n_vox32;
        if (vf_ensure(c, M.tmp, 3 * (size_t)n_vox)) return DCREG_E_NOMEM;
        hipLaunchKernelGGL(k_vmap_reduce, dim3(blocks(n_vox, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, M.f_sub.data(), ord, n_vox, B.start.data(), prm.min_points,
                           prm.epsilon, M.tmp.data(), B.keep.data(), M.cls.data());
        rc = scan_u32(c, B.keep.data(), B.pos.data(), (size_t)n_vox, false);
        if (rc) return rc;
    }
    // ---- the old records: carried or gone
    const size_t nk1 = (size_t)nk + 1;
    if (vf_ensure(c, M.f_flag, 2 * nk1)) return DCREG_E_NOMEM;
    uint32_t *cflag = M.f_flag.data(), *cpos = cflag + nk1;
    hipLaunchKernelGGL(k_vfollow_carry, dim3(blocks((int64_t)nk1, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, M.vkeys.data(), nk, old, uni, tb, M.f_set.data(), fmask, cflag);
    rc = scan_u32(c, cflag, cpos, nk1, false);
    if (rc) return rc;
    uint32_t n_a32 = 0, last[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&n_a32, cpos + nk, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (n_vox > 0) {
        HIP_TRY(c, hipMemcpyAsync(&last[0], B.keep.data() + (n_vox - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&last[1], B.pos.data() + (n_vox - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const int64_t n_a = n_a32, n_b = (int64_t)last[0] + (int64_t)last[1], n_kept = n_a + n_b;
    F.n_refit = n_vox; F.n_carried = n_a; F.n_kept = n_kept; F.followed = 1;
    M.n_kept = 0;
    if (n_kept == 0) return DCREG_OK;                  // (nothing kept: no member, as after a keep that keeps nothing)
    // ---- the next member beside the current one: merge, records, keys, table
    size_t slots = 2;
    while (slots < 2 * (size_t)n_kept) slots <<= 1;
    if (vf_ensure(c, M.f_akeys, (size_t)nk) || vf_ensure(c, M.f_asrc, (size_t)nk) || vf_ensure(c, M.f_bkeys, (size_t)n_vox) || vf_ensure(c, M.f_bsrc, (size_t)n_vox) ||
        vf_ensure(c, M.recs_alt, 3 * (size_t)n_kept) || vf_ensure(c, M.vkeys_alt, (size_t)n_kept) || M.t_keys_alt.ensure(c, slots) || M.t_vals_alt.ensure(c, slots))
        return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(M.t_keys_alt.data(), 0xFF, slots * sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_vfollow_runs, dim3(blocks(nk + n_vox, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, M.vkeys.data(), nk, cflag, cpos, old, nw, n_vox, B.keep.data(),
                       B.pos.data(), ord, B.start.data(), B.rel.data(), bits[0], bits[1], tb, M.f_akeys.data(), M.f_asrc.data(), M.f_bkeys.data(), M.f_bsrc.data());
    hipLaunchKernelGGL(k_vfollow_write, dim3(blocks(n_kept, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, n_a, n_b, M.f_akeys.data(), M.f_asrc.data(), M.f_bkeys.data(),
                       M.f_bsrc.data(), M.recs.data(), M.tmp.data(), M.recs_alt.data(), M.vkeys_alt.data(), M.t_keys_alt.data(), M.t_vals_alt.data(),
                       (uint32_t)(slots - 1));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    M.recs.swap(M.recs_alt); M.vkeys.swap(M.vkeys_alt); M.t_keys.swap(M.t_keys_alt); M.t_vals.swap(M.t_vals_alt);
    for (int a = 0; a < 3; ++a) { M.mn[a] = nw.lo[a]; M.mx[a] = nw.hi[a]; }
    M.mask = (uint32_t)(slots - 1); M.n_kept = n_kept; M.kept = true;
    return DCREG_OK;
}

}  // namespace

bool voxels_follow_wanted(const dcreg_ctx *c) { return c->opt_voxels_follow && c->vmap.kept && c->vmap.n_kept > 0; }

// (the update stands whatever happens here: a failure leaves the member dropped, as map_changed left it, and says so in the info)
void voxels_follow_update(dcreg_ctx *c, const FollowChange &ch, bool wanted) {
    dcreg_ctx::VoxelMapBufs &M = c->vmap;
    M.follow = dcreg_voxels_follow_info{};
    M.follow.n_target = c->map.n;
    if (!wanted) return;
    if (follow_run(c, ch) == DCREG_OK) return;
    (void)hipGetLastError();
    M.kept = false; M.n_kept = 0;
    M.follow = dcreg_voxels_follow_info{};
    M.follow.n_target = c->map.n;
}

// the parameter refusals of dcreg_target_voxels_keep on their own, in its order (dcreg_register_pairs_voxels makes them before its empty
// call returns; pairs_voxels_build before it touches anything)
int voxel_map_params_check(dcreg_ctx *c, const dcreg_voxel_map_params *p) {
    if (!c) return DCREG_E_INVALID;
    if (!p) { c->fail("null voxel map parameters"); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->leaf) && p->leaf > 0.0)) { c->fail("voxel map leaf is %g: finite and > 0 expected", p->leaf); return DCREG_E_INVALID; }
    if (!(p->epsilon >= 1.0e-6 && p->epsilon <= 1.0)) { c->fail("voxel map epsilon is %g: 1e-6 .. 1 expected", p->epsilon); return DCREG_E_INVALID; }
    if (p->min_points < 2) { c->fail("voxel map min_points is %d: at least 2 expected", p->min_points); return DCREG_E_INVALID; }
    return DCREG_OK;
}

// What the voxel box of a cloud with these float bounds refuses (floor((double)x / leaf) is monotonic in the float x: the box of a cloud's
// voxels is exactly the voxels of its coordinate-wise minimum and maximum): a coordinate of magnitude 2^62 or more, 2^21 or more voxels
// on an axis.  dcreg_register_pairs_voxels checks the targets of its later build batches with it on the host, before anything is queued;
// the device's own counters (k_vox_coords) refuse the same targets in a build.  `t`: the target's number in the message
int voxel_box_check(dcreg_ctx *c, const float mn[3], const float mx[3], double leaf, int t) {
    for (int a = 0; a < 3; ++a) {
        const double lo = std::floor((double)mn[a] / leaf), hi = std::floor((double)mx[a] / leaf);
        if (!(std::fabs(lo) < kVoxLimit) || !(std::fabs(hi) < kVoxLimit)) {
            c->fail("a voxel coordinate of pair target %d reaches 2^62 (leaf too small for the coordinates)", t);
            return DCREG_E_INVALID;
        }
        const int64_t d = (int64_t)hi - (int64_t)lo;
        if (d + 1 > kSpanMax) {
            c->fail("pair target %d spans %lld voxels on axis %d (at most 2^21 - 1 = %lld)", t, (long long)d + 1, a, (long long)kSpanMax);
            return DCREG_E_INVALID;
        }
    }
    return DCREG_OK;
}

// The kept voxel maps of one build batch of pair targets (xyz: HOST memory, target t = points [off[t], off[t + 1]), off[0] = 0): target
// t's member is bitwise what dcreg_set_target(target t) + dcreg_target_voxels_keep(p) keep - a voxel map depends on the target's points
// in upload order only, so no grid, no cell table and no normals are built.  All targets at once: ONE upload, ONE pack with the float
// bounds (k_pairs_pack), ONE k_vox_coords, the order of vox_order (ONE sort when target and voxel bits fit 64, else TWO; ONE scan), ONE
// k_vmap_reduce over the voxels of all targets - unchanged: its per-voxel rule and summation order are the contract - ONE scan of the
// keep flags, ONE k_pvmap_count, ONE k_pvmap_write.  FOUR stream synchronises (bounds and voxel boxes; the voxel count; the per-target
// counters; the end), whatever the number of targets.  Everything is refused before the batch on the device is replaced: a non-finite
// coordinate, a voxel coordinate of 2^62, a target of 2^21 voxels on an axis (DCREG_E_INVALID).  infos (may be null): one record per
// target, as dcreg_target_voxels_keep fills it
int pairs_voxels_build(dcreg_ctx *c, int n_t, const float *xyz, const int64_t *off, int64_t stride, const dcreg_voxel_map_params *p,
                       dcreg_voxel_map_info *infos) {
    if (int rc = voxel_map_params_check(c, p)) return rc;
    if (n_t < 0 || !off || stride < 3 || off[0] != 0) { c->fail("invalid pair target arguments"); return DCREG_E_INVALID; }
    for (int t = 0; t < n_t; ++t)
        if (off[t + 1] < off[t]) { c->fail("pair target offsets decrease at target %d", t); return DCREG_E_INVALID; }
    const int64_t n = n_t > 0 ? off[n_t] : 0;
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    if (n >= ((int64_t)1 << 31) - 1) { c->fail("the pair targets of one build batch hold too many points (%lld)", (long long)n); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    dcreg_ctx::PairVoxBufs &V = c->pvox;
    dcreg_ctx::VoxelBufs &B = c->vox;
    std::vector<PairVoxMap> maps((size_t)n_t);
    std::memset(maps.data(), 0, sizeof(PairVoxMap) * (size_t)n_t);
    std::vector<unsigned long long> pc((size_t)4 * std::max(n_t, 1), 0ull);
    const double l = p->leaf;
    // the targets' records to the device (a target without a member is a record of zeros)
    auto upload_maps = [&]() -> int {
        if (V.d_maps.ensure(c, (size_t)std::max(n_t, 1))) return DCREG_E_NOMEM;
        HIP_TRY(c, hipMemcpyAsync(V.d_maps.data(), maps.data(), sizeof(PairVoxMap) * (size_t)n_t, hipMemcpyHostToDevice, c->stream));
        return DCREG_OK;
    };
    // the end of a build: the last wait (maps is the source of the copy above), the infos, the batch
    auto finish = [&]() -> int {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        for (int t = 0; infos && t < n_t; ++t) {
            infos[t].n_points = off[t + 1] - off[t]; infos[t].n_voxels = (int64_t)pc[(size_t)4 * t]; infos[t].n_small = (int64_t)pc[(size_t)4 * t + 1];
            infos[t].n_degenerate = (int64_t)pc[(size_t)4 * t + 2]; infos[t].n_kept = (int64_t)pc[(size_t)4 * t + 3];
        }
        V.maps = std::move(maps);
        V.leaf = l;
        V.n = n_t;
        return DCREG_OK;
    };
    HIP_TRY(c, hipSetDevice(c->device));
    if (n == 0) {                                          // (no points at all: every target without a member)
        V.n = 0;
        if (n_t > 0) if (int rc = upload_maps()) return rc;
        return finish();
    }
    const size_t nc = (size_t)kCnt * n_t + kTail;
    if (B.pts.ensure(c, (size_t)n) || B.seg.ensure(c, (size_t)n) || B.rel.ensure(c, (size_t)n) || B.head.ensure(c, (size_t)n) ||
        B.incl.ensure(c, (size_t)n) || B.start.ensure(c, (size_t)n + 1) || B.keep.ensure(c, (size_t)n) || B.pos.ensure(c, (size_t)n) ||
        B.d_off.ensure(c, (size_t)n_t + 1) || B.cnt.ensure(c, nc) || c->d_mkeys.ensure(c, (size_t)n) || c->d_mkeys2.ensure(c, (size_t)n) ||
        c->d_vals.ensure(c, (size_t)n) || c->d_vals2.ensure(c, (size_t)n) ||
        V.d_words.ensure(c, (size_t)6 * n_t) || V.d_cnt.ensure(c, (size_t)4 * n_t + 2))
        return DCREG_E_NOMEM;
    // ---- upload, pack and float bounds, voxel boxes: one readback
    const float *staged = nullptr;
    if (int rc = caller_rows(c, xyz, n, stride, stride, false, c->d_stage, &staged)) return rc;
    HIP_TRY(c, hipMemcpyAsync(B.d_off.data(), off, sizeof(int64_t) * ((size_t)n_t + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(V.d_words.data(), 0xFF, sizeof(uint32_t) * 3 * (size_t)n_t, c->stream));
    HIP_TRY(c, hipMemsetAsync(V.d_words.data() + 3 * (size_t)n_t, 0, sizeof(uint32_t) * 3 * (size_t)n_t, c->stream));
    HIP_TRY(c, hipMemsetAsync(V.d_cnt.data(), 0, sizeof(unsigned long long) * (4 * (size_t)n_t + 2), c->stream));     // (+ 2: k_vmap_reduce's own two counts)
    hipLaunchKernelGGL(k_pairs_pack, dim3(blocks(n, 256)), dim3(256), 0, c->stream, staged, n, stride, B.d_off.data(), n_t, B.pts.data(), V.d_words.data());
    hipLaunchKernelGGL(k_vox_init, dim3(blocks((int64_t)nc * 2, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, B.cnt.data(), n_t);
    hipLaunchKernelGGL(k_vox_coords, dim3(blocks(n, kVoxBlock * kVoxPerThread)), dim3(kVoxBlock), 0, c->stream, B.pts.data(), n, B.d_off.data(), n_t, l, l, l,
                       B.seg.data(), B.cnt.data());
    std::vector<uint32_t> words((size_t)6 * n_t);
    std::vector<int64_t> h(nc);
    HIP_TRY(c, hipMemcpyAsync(words.data(), V.d_words.data(), sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h.data(), B.cnt.data(), sizeof(int64_t) * nc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    // ---- the refusals of the batch (the batch a previous build left is still whole)
    for (int t = 0; t < n_t; ++t) {
        if (off[t + 1] == off[t]) continue;
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(ord2f(words[(size_t)3 * t + a])) || !std::isfinite(ord2f(words[(size_t)3 * n_t + 3 * t + a]))) { c->fail("pair target %d has non-finite coordinates", t); return DCREG_E_INVALID; }
    }
    uint32_t tail[2 * kTail];
    std::memcpy(tail, h.data() + (size_t)kCnt * n_t, sizeof(tail));
    if (tail[6]) { c->fail("a voxel coordinate of a pair target reaches 2^62 (leaf too small for the coordinates)"); return DCREG_E_INVALID; }
    int64_t span[3] = {0, 0, 0};
    for (int t = 0; t < n_t; ++t) {
        const int64_t *q = h.data() + (size_t)kCnt * t;
        if (q[6] == 0) continue;
        for (int a = 0; a < 3; ++a) {
            const int64_t d = q[3 + a] - q[a];
            if (d + 1 > kSpanMax) {                           // (d = maximum - minimum: d + 1 voxels)
                c->fail("pair target %d spans %lld voxels on axis %d (at most 2^21 - 1 = %lld)", t, (long long)d + 1, a, (long long)kSpanMax);
                return DCREG_E_INVALID;
            }
            span[a] = std::max(span[a], d);
            maps[(size_t)t].mn[a] = q[a]; maps[(size_t)t].mx[a] = q[3 + a];
        }
    }
    V.n = 0;                                               // (the member's arrays are rewritten from here on: a failure leaves no batch)
    const int bx = bits_for(span[0]), by = bits_for(span[1]), bz = bits_for(span[2]);
    // ---- keys, stable sort, voxel heads and starts over all targets; the voxel count
    const uint32_t *ord;
    int rc = vox_order(c, B.pts.data(), n, n_t, l, l, l, bx, by, bz, ord);
    if (rc) return rc;
    uint32_t n_vox32 = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_vox32, B.incl.data() + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    const int64_t n_vox = n_vox32;
    // ---- one lane per voxel of any target, the scan of the keep flags, the per-target counters
    if (V.tmp.ensure(c, 3 * (size_t)n_vox)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_vmap_reduce, dim3(blocks(n_vox, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, B.pts.data(), ord, n_vox, B.start.data(), p->min_points,
                       p->epsilon, V.tmp.data(), B.keep.data(), V.d_cnt.data() + 4 * (size_t)n_t);
    rc = scan_u32(c, B.keep.data(), B.pos.data(), (size_t)n_vox, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pvmap_count, dim3(blocks(n_vox, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, ord, n_vox, B.seg.data(), B.start.data(), B.keep.data(),
                       p->min_points, V.d_cnt.data());
    HIP_TRY(c, hipMemcpyAsync(pc.data(), V.d_cnt.data(), sizeof(unsigned long long) * 4 * (size_t)n_t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    // ---- the members: every target's first record, and its table of the power of two at or above twice its kept voxels
    size_t n_kept = 0, n_slots = 0;
    for (int t = 0; t < n_t; ++t) {
        PairVoxMap &m = maps[(size_t)t];
        const size_t k = (size_t)pc[(size_t)4 * t + 3];
        if (k == 0) continue;
        size_t slots = 2;
        while (slots < 2 * k) slots <<= 1;
        m.first = (uint32_t)n_kept; m.base = (uint32_t)n_slots; m.mask = (uint32_t)(slots - 1); m.n_kept = (uint32_t)k;
        n_kept += k; n_slots += slots;
    }
    if ((rc = upload_maps())) return rc;
    if (n_kept == 0) return finish();                      // (no target keeps a voxel: no member anywhere)
    if (n_slots > 0xFFFFFFFFull) { c->fail("the pair targets' lookup tables hold too many slots (%zu)", n_slots); return DCREG_E_INVALID; }
    if (V.recs.ensure(c, 3 * n_kept) || V.vkeys.ensure(c, n_kept) || V.t_keys.ensure(c, n_slots) || V.t_vals.ensure(c, n_slots)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(V.t_keys.data(), 0xFF, n_slots * sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL(k_pvmap_write, dim3(blocks(n_vox, kVoxBlock)), dim3(kVoxBlock), 0, c->stream, V.tmp.data(), B.keep.data(), B.pos.data(), n_vox, ord, B.seg.data(),
                       B.start.data(), B.rel.data(), bx, by, V.d_maps.data(), V.recs.data(), V.vkeys.data(), V.t_keys.data(), V.t_vals.data());
    HIP_TRY(c, hipGetLastError());
    return finish();                                       // (waits for the stream)
}

// dcreg_pairs_voxels_get: one target's member of the batch to the host, unpacked as voxel_map_get unpacks the map's
static int pairs_voxels_get(dcreg_ctx *c, int target, int64_t *coords, int32_t *count, float *mean, float *cov, int64_t capacity) {
    if (!c) return DCREG_E_INVALID;
    if (!coords || !count || !mean || !cov) { c->fail("null argument"); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    const dcreg_ctx::PairVoxBufs &V = c->pvox;
    if (V.n <= 0) { c->fail("no pair voxel batch built: dcreg_pairs_voxels_build first"); return DCREG_E_STATE; }
    if (target < 0 || target >= V.n) { c->fail("pair target %d is not in the batch", target); return DCREG_E_INVALID; }
    const PairVoxMap &m = V.maps[(size_t)target];
    if (capacity < (int64_t)m.n_kept) { c->fail("the output holds %lld voxels, the target keeps %u", (long long)capacity, m.n_kept); return DCREG_E_INVALID; }
    if (m.n_kept == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nk = m.n_kept;
    std::vector<float> rec(12 * nk);
    std::vector<uint64_t> keys(nk);
    HIP_TRY(c, hipMemcpyAsync(rec.data(), V.recs.data() + 3 * (size_t)m.first, sizeof(float) * 12 * nk, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(keys.data(), V.vkeys.data() + m.first, sizeof(uint64_t) * nk, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t am = (1ull << kVmapAxisBits) - 1ull;
    for (size_t j = 0; j < nk; ++j) {
        const float *r = rec.data() + 12 * j;
        coords[3 * j] = m.mn[0] + (int64_t)(keys[j] & am);
        coords[3 * j + 1] = m.mn[1] + (int64_t)((keys[j] >> kVmapAxisBits) & am);
        coords[3 * j + 2] = m.mn[2] + (int64_t)(keys[j] >> (2 * kVmapAxisBits));
        std::memcpy(mean + 3 * j, r, 3 * sizeof(float));
        std::memcpy(cov + 6 * j, r + 3, 6 * sizeof(float));
        std::memcpy(count + j, r + 9, sizeof(int32_t));
    }
    return DCREG_OK;
}

}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_voxel_map_params_check(dcreg_ctx *c, const dcreg_voxel_map_params *p) { return voxel_map_params_check(c, p); }
int dcreg_pairs_voxels_build(dcreg_ctx *c, int n_targets, const float *xyz, const int64_t *tgt_offsets, int64_t stride_floats,
                             const dcreg_voxel_map_params *p, dcreg_voxel_map_info *infos) {
    return c ? pairs_voxels_build(c, n_targets, xyz, tgt_offsets, stride_floats, p, infos) : DCREG_E_INVALID;
}
int dcreg_pairs_voxels_get(dcreg_ctx *c, int target, int64_t *coords, int32_t *count, float *mean, float *cov, int64_t capacity_voxels) {
    return pairs_voxels_get(c, target, coords, count, mean, cov, capacity_voxels);
}
int dcreg_pairs_voxels_kept(const dcreg_ctx *c, int target) {
    return c && target >= 0 && target < c->pvox.n ? (int)c->pvox.maps[(size_t)target].n_kept : 0;
}
int dcreg_pairs_voxels_box_check(dcreg_ctx *c, const float mn[3], const float mx[3], double leaf, int target) {
    return c && mn && mx ? voxel_box_check(c, mn, mx, leaf, target) : DCREG_E_INVALID;
}
int dcreg_voxel_downsample(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_voxel_params *p,
                           float *out_xyz, int64_t capacity_points, int64_t *out_offsets, dcreg_voxel_info *info) {
    return voxel_downsample_to(c, n_clouds, xyz, offsets, stride_floats, false, p, out_xyz, capacity_points, out_offsets, info);
}
int dcreg_voxel_downsample_device(dcreg_ctx *c, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                  const dcreg_voxel_params *p, float *d_out_xyz, int64_t capacity_points, int64_t *out_offsets, dcreg_voxel_info *info) {
    return voxel_downsample_to(c, n_clouds, d_xyz, offsets, stride_floats, true, p, d_out_xyz, capacity_points, out_offsets, info);
}
int dcreg_default_voxel_map_params(dcreg_voxel_map_params *p) {
    if (!p) return DCREG_E_INVALID;
    p->leaf = 1.0; p->epsilon = 1.0e-3; p->min_points = 6; p->reserved_ = 0;
    return DCREG_OK;
}
int dcreg_target_voxels_keep(dcreg_ctx *c, const dcreg_voxel_map_params *p, dcreg_voxel_map_info *info) { return voxel_map_keep(c, p, info); }
int dcreg_target_voxels_get(dcreg_ctx *c, int64_t *coords, int32_t *count, float *mean, float *cov, int64_t capacity_voxels) {
    return voxel_map_get(c, coords, count, mean, cov, capacity_voxels);
}
int dcreg_target_voxels_kept(const dcreg_ctx *c) { return c && c->vmap.kept ? (int)c->vmap.n_kept : 0; }
int dcreg_target_voxels_drop(dcreg_ctx *c) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    dcreg_ctx::VoxelMapBufs &M = c->vmap;
    M.kept = false; M.n_kept = 0;
    M.recs.reset(); M.tmp.reset(); M.vkeys.reset(); M.t_keys.reset(); M.t_vals.reset();
    M.recs_alt.reset(); M.vkeys_alt.reset(); M.t_keys_alt.reset(); M.t_vals_alt.reset(); M.f_sub.reset(); M.f_set.reset(); M.f_flag.reset();
    M.f_akeys.reset(); M.f_asrc.reset(); M.f_bkeys.reset(); M.f_bsrc.reset();
    return DCREG_OK;
}
int dcreg_target_voxels_follow_info(const dcreg_ctx *c, dcreg_voxels_follow_info *info) {
    if (!c || !info) return DCREG_E_INVALID;
    *info = c->vmap.follow;
    return DCREG_OK;
}
}
