// Per-thread device function of the second engine (include/dcreg.h: dcreg_linearize_normals): one source point against the map's kept
// normals - transform, exact 1-NN on the cell grid, radius gate, the stored normal of the nearest point, residual, weight, row.  The
// rule is the header's, operation by operation; tests/normal_icp_ref.py states it in numpy.  Included by normal_icp.hip (the kernel and
// the reductions) and, like search.hpp, compiled for the host under DCREG_HOST_EMUL by the test suite's replay (tests/host_emul/).
#pragma once
#include "search.hpp"

namespace dcreg {

// The smallest (d2, index) key of the candidates below a start key, with its position in the sorted array: HeapExact's 64-bit key in one
// slot (search.hpp; the interface of its heaps).  `start` is set by the caller before the search: the walk's init() takes it, not the
// float bound.  A slot that was never filled keeps position kNoIdx.
struct HeapOne {
    static constexpr int K = 1;
    static constexpr bool kDeferred = false;
    uint64_t key, start;
    uint32_t pos;
    uint32_t n_eval, n_shell;
    DCREG_DEVFN void init(float /*bound_f*/, float = 1.f, float = 0.f) { key = start; pos = kNoIdx; n_eval = 0; n_shell = 1; }
    DCREG_DEVFN void push(float d2, uint32_t idx, uint32_t p, bool valid = true) {
        n_eval += valid ? 1u : 0u;                  // (statistics of the host replay; dead code on the device)
        const uint64_t kk = ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)idx;
        if (valid && kk < key) { key = kk; pos = p; }
    }
    DCREG_DEVFN float worst_d2() const { return __uint_as_float((uint32_t)(key >> 32)); }
};

struct NlinArgs {
    double radius_sq;             // R^2 in double: the gate (double)d2 < R^2
    float bound_f;                // the cold search bound: the smallest float >= R^2 (a d2 below R^2 is below it; d2 == bound stays out)
    int max_ring;                 // rings that cover it
    double w_slope, w_min;
    int use_wd;
    int robust = 0;               // "robust_kernel" (DCREG_ROBUST_*): 0 multiplies nothing
    double robust_c2 = 1.0;       // c * c of "robust_scale", formed once on the host
};

// what the debug dump shows of a point (flag 0: idx kNoIdx, d2 +inf; no normal: NaN components as stored)
struct NlinPoint {
    uint32_t idx, pos;            // original index of the nearest point and its position in the sorted array (kNoIdx: none inside the bound)
    float d2;
    double n[3], r, s;
    uint32_t n_eval;              // candidates the search evaluated (host replay)
};

// The robust kernels of the second and third engine (include/dcreg.h, "robust kernels"): k = sqrt(rho'(r) / r) of the kernel `kind` (1 Huber,
// 2 Cauchy, 3 Geman-McClure) at u2 = (r / c)^2.  Every operation rounds once; division and square root are IEEE double.
DCREG_DEVFN double robust_factor(int kind, double u2) {
#pragma clang fp contract(off)
    if (kind == 1) {
        const double u = sqrt(u2);
        return u <= 1.0 ? 1.0 : sqrt(1.0 / u);
    }
    if (kind == 2) return 1.0 / sqrt(1.0 + u2);
    return 1.0 / (1.0 + u2);
}

DCREG_DEVFN bool nlin_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// One point of dcreg_linearize_normals.  warm_pos: the sorted position of the point's nearest neighbour at its last search (kNoIdx, or
// anything beyond the map: none) - the search then starts bounded by that point's distance from the new position, inclusive: the point
// itself is a candidate inside the bound, so the minimum key over the bounded candidates is the minimum over the map - the result does
// not depend on warm_pos.  normals: float4 {nx, ny, nz, curvature} per map point in index order.  Returns the flag (0 radius gate, 2 no
// normal, 4 weight gate, 1 effective); the row is zero unless the flag is 1.  With a robust kernel on, slots 0..6 of a flag-1 row are
// multiplied by the kernel's factor at r; slot 7 stays r.
DCREG_DEVFN uint8_t nlin_point(const GridDev &g, RunList &rl, const float4 *normals, const PoseArg &P, const NlinArgs &a, const float4 &s4,
                               uint32_t warm_pos, double (&row)[8], NlinPoint &o) {
#pragma clang fp contract(off)
    const double px = (double)s4.x, py = (double)s4.y, pz = (double)s4.z;
    float qx, qy, qz;
    body_to_global(P, px, py, pz, qx, qy, qz);
    HeapOne hp;
    float bound_f = a.bound_f;
    hp.start = (uint64_t)__float_as_uint(bound_f) << 32;                   // index 0: d2 == bound does not enter
    if (warm_pos < g.n_pts) {
        const float d2w = dist2_nofma(qx, qy, qz, g.pts[warm_pos]);
        if (d2w < bound_f) {                                               // (finite and >= 0: its bit pattern + 1 is the next float up)
            const uint32_t up = __float_as_uint(d2w) + 1u;
            bound_f = __uint_as_float(up);
            hp.start = (uint64_t)up << 32;                                 // every key (d2w, any index) enters
        }
    }
    knn_search<HeapOne>(g, rl, qx, qy, qz, bound_f, a.max_ring, hp);
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = 0.0;
    o.idx = kNoIdx; o.pos = kNoIdx; o.d2 = __builtin_inff(); o.n_eval = hp.n_eval;
    o.n[0] = o.n[1] = o.n[2] = 0.0; o.r = 0.0; o.s = 0.0;
    if (hp.pos == kNoIdx) return 0;
    const float d2 = __uint_as_float((uint32_t)(hp.key >> 32));
    if (!((double)d2 < a.radius_sq)) return 0;
    o.pos = hp.pos; o.idx = (uint32_t)hp.key; o.d2 = d2;
    const float4 tj = g.pts[hp.pos];
    const float4 n4 = normals[o.idx];
    const double nx = (double)n4.x, ny = (double)n4.y, nz = (double)n4.z;
    o.n[0] = nx; o.n[1] = ny; o.n[2] = nz;
    if (!(nlin_finite(n4.x) && nlin_finite(n4.y) && nlin_finite(n4.z))) return 2;
    const double ex = (double)qx - (double)tj.x, ey = (double)qy - (double)tj.y, ez = (double)qz - (double)tj.z;
    const double r = (nx * ex + ny * ey) + nz * ez;
    double s = 1.0 - a.w_slope * fabs(r);
    s = s < 0.0 ? 0.0 : s;
    double ds = 0.0;
    if (a.use_wd && s > 0.0 && s < 1.0) ds = -a.w_slope * (r > 0.0 ? 1.0 : -1.0);
    o.r = r; o.s = s;
    if (!(s > a.w_min)) return 4;
    const double m0 = (P.R[0] * nx + P.R[3] * ny) + P.R[6] * nz;
    const double m1 = (P.R[1] * nx + P.R[4] * ny) + P.R[7] * nz;
    const double m2 = (P.R[2] * nx + P.R[5] * ny) + P.R[8] * nz;
    const double w = s + r * ds;
    row[0] = w * (py * m2 - pz * m1); row[1] = w * (pz * m0 - px * m2); row[2] = w * (px * m1 - py * m0);
    row[3] = w * m0; row[4] = w * m1; row[5] = w * m2;
    row[6] = -(s * r);
    row[7] = r;
    if (a.robust) {                                                        // (launch-uniform) after the gathers: nothing of it is live across the search
        const double k = robust_factor(a.robust, (r * r) / a.robust_c2);
#pragma unroll
        for (int j = 0; j < 7; ++j) row[j] = k * row[j];
    }
    return 1;
}

#if !defined(DCREG_HOST_EMUL)
// The cloud of block (x, pose) in a batched launch of any engine (k_nlin_batch, k_glin_batch, k_vlin_batch, k_vlin_pairs): slices[pose] =
// {first point, points} of the set the launch reads.  false: the block lies past the end of its pose's slice and exits before it touches
// anything (uniform per block); else the slice's points become n_src and `first` is where they start in the set's arrays
__device__ __forceinline__ bool batch_slice(const uint2 *__restrict__ slices, uint32_t &first, uint32_t &n_src) {
    const uint2 sl = slices[blockIdx.y];
    if (blockIdx.x >= (sl.y + kLinBlock - 1) / kLinBlock) return false;
    first = sl.x; n_src = sl.y;
    return true;
}
#endif

}  // namespace dcreg
