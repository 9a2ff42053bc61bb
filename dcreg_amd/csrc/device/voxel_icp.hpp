// Per-thread device functions of the fourth engine (include/dcreg.h: dcreg_linearize_voxels): one source point against the map's kept
// voxel distributions - transform, the voxel the transformed point falls into (a lookup, no search), three 16-byte gathers of that
// voxel's record, the covariance of the pair (the record's alone, or with the source's plane covariance on top), then the third engine's
// Cholesky factor, whitening matrix and rows (gicp.hpp glin_row, glin_row_scale).  The rule is the header's, operation by operation;
// tests/voxels_ref.py states it in numpy.  With "voxels_neighbors" = 7 / 27 the same per voxel of a stencil around the point's own: the
// lookup by voxel coordinates (vmap_find_voxel), the stencil (vlin_offset), the point's normal once (vlin_normal) and one correspondence
// (vlin_corr), of which vlin_point is the S = 1 composition; tests/voxels_stencil_ref.py states that in numpy.  Included by voxel_icp.hip (the kernel and the run) and by voxel.hip (the table's fill) and,
// like gicp.hpp, compiled for the host under DCREG_HOST_EMUL by the test suite's replay (tests/host_emul/).
#pragma once
#include "gicp.hpp"

namespace dcreg {

constexpr int kVmapAxisBits = 21;                        // a map spans fewer than 2^21 voxels per axis (the voxel pass's limit)
constexpr uint64_t kVmapEmpty = ~0ull;                   // an empty slot of the lookup table (no key has bit 63 set)
constexpr uint32_t kVmapRecWords = 3;                    // float4 per kept voxel: {mu_x mu_y mu_z cxx} {cxy cxz cyy cyz} {czz n 0 0}

// The kept voxel map as a kernel reads it: the records in dcreg_target_voxels_get order and an open-addressing table over the kept
// voxels' keys - (v - mn) per axis, 21 bits each, z y x - that holds each one's record number; linear probing, at most half full.
// mn / mx: the voxel box of ALL map points (a query outside it answers "none" before the table is read).
struct VoxMapDev {
    const float4 *recs;
    const uint64_t *keys;
    const uint32_t *vals;
    uint32_t mask;                                       // slots - 1 (a power of two)
    long long mn[3], mx[3];
    double leaf;
};
// ... formed on the host from the context's kept map and in k_vlin_pairs from a pair target's record (voxel_icp.hip)
#if !defined(DCREG_HOST_EMUL)
__host__ __device__ __forceinline__ VoxMapDev vox_map_dev(const float4 *recs, const uint64_t *keys, const uint32_t *vals, uint32_t mask,
                                                          const long long (&mn)[3], const long long (&mx)[3], double leaf) {
    VoxMapDev vm;
    vm.recs = recs; vm.keys = keys; vm.vals = vals; vm.mask = mask; vm.leaf = leaf;
#pragma unroll
    for (int k = 0; k < 3; ++k) { vm.mn[k] = mn[k]; vm.mx[k] = mx[k]; }
    return vm;
}
#endif

DCREG_DEVFN uint64_t vmap_key(uint64_t rx, uint64_t ry, uint64_t rz) { return (rz << (2 * kVmapAxisBits)) | (ry << kVmapAxisBits) | rx; }
// where a key's probe sequence starts (the finaliser of MurmurHash3: neighbouring voxels land far apart)
DCREG_DEVFN uint32_t vmap_slot(uint64_t key, uint32_t mask) {
    key ^= key >> 33; key *= 0xff51afd7ed558ccdull;
    key ^= key >> 33; key *= 0xc4ceb9fe1a85ec53ull;
    key ^= key >> 33;
    return (uint32_t)key & mask;
}

// the record number of the kept voxel at the voxel coordinates (v0, v1, v2) - whole numbers as doubles, or not finite - kNoIdx when there
// is none: coordinates outside the map's voxel box answer before the table is read, so the key is never formed from a negative difference
DCREG_DEVFN uint32_t vmap_find_voxel(const VoxMapDev &m, double v0, double v1, double v2) {
    // (the box's corners are voxels of map points: exact as doubles; a NaN fails every comparison)
    if (!(v0 >= (double)m.mn[0] && v0 <= (double)m.mx[0] && v1 >= (double)m.mn[1] && v1 <= (double)m.mx[1] && v2 >= (double)m.mn[2] &&
          v2 <= (double)m.mx[2]))
        return kNoIdx;
    const uint64_t key = vmap_key((uint64_t)((long long)v0 - m.mn[0]), (uint64_t)((long long)v1 - m.mn[1]), (uint64_t)((long long)v2 - m.mn[2]));
    uint32_t s = vmap_slot(key, m.mask);
    for (;;) {                                           // (ends: the table is at most half full)
        const uint64_t k = m.keys[s];
        if (k == key) return m.vals[s];
        if (k == kVmapEmpty) return kNoIdx;
        s = (s + 1u) & m.mask;
    }
}
// the record number of the kept voxel that holds q, kNoIdx when there is none: v_a = floor((double)q_a / leaf) as voxel.hip's voxel_of
DCREG_DEVFN uint32_t vmap_find(const VoxMapDev &m, float qx, float qy, float qz) {
    return vmap_find_voxel(m, floor((double)qx / m.leaf), floor((double)qy / m.leaf), floor((double)qz / m.leaf));
}

// Offset j of the stencil of S voxels around a point's own ("voxels_neighbors": 1, 7 or 27), as doubles.  Offset 0 is the point's own voxel.
// S = 7: +x -x +y -y +z -z follow; S = 27: the other 26 of the 3^3 block in ascending (dz, dy, dx).  Arithmetic only: no table is indexed.
DCREG_DEVFN void vlin_offset(int S, int j, double &dx, double &dy, double &dz) {
    int o[3] = {0, 0, 0};
    if (S == 7) {
        if (j > 0) o[(j - 1) >> 1] = (j & 1) ? 1 : -1;
    } else if (S == 27 && j > 0) {
        const int c = j <= 13 ? j - 1 : j;               // (position in the block's (dz, dy, dx) order: the centre, 13, is left out)
        o[0] = c % 3 - 1; o[1] = (c / 3) % 3 - 1; o[2] = c / 9 - 1;
    }
    dx = (double)o[0]; dy = (double)o[1]; dz = (double)o[2];
}

struct VlinArgs {
    int source_cov;               // "voxels_source_cov": 0 point-to-distribution, 1 distribution-to-distribution
    double c;                     // 1 - epsilon ("gicp_epsilon"), formed once on the host
    int robust = 0;               // "robust_kernel" (DCREG_ROBUST_*): 0 multiplies nothing
    double robust_c2 = 1.0;       // c * c of "gicp_robust_scale", formed once on the host
};

// what a point leaves for the debug dump beside its GlinPoint (m, w, e, k): the voxel and its record, widened
struct VlinPoint {
    uint32_t vidx;                // position in dcreg_target_voxels_get order (kNoIdx: none)
    double mean[3], cov[6];
};

// The source normal of a point in mode 1, read and formed once per point: m, and u = R m with each component summed as glin_point sums
// it.  Returns whether the normal is there (every component finite); u is formed either way and read only when it is.
DCREG_DEVFN bool vlin_normal(const PoseArg &P, const float4 &m4, double (&m)[3], double (&u)[3]) {
#pragma clang fp contract(off)
    const double mx = (double)m4.x, my = (double)m4.y, mz = (double)m4.z;
    m[0] = mx; m[1] = my; m[2] = mz;
    u[0] = (P.R[0] * mx + P.R[1] * my) + P.R[2] * mz;
    u[1] = (P.R[3] * mx + P.R[4] * my) + P.R[5] * mz;
    u[2] = (P.R[6] * mx + P.R[7] * my) + P.R[8] * mz;
    return nlin_finite(m4.x) && nlin_finite(m4.y) && nlin_finite(m4.z);
}

// One correspondence of dcreg_linearize_voxels up to its whitening matrix: the transformed point q against the kept voxel with record
// number vidx (kNoIdx: none) - the three gathers of its record, the covariance of the pair, its factor, W, e and the robust factor.
// normal_of(u): the point's own normal in mode 1 (vlin_normal) - whether it is there, and u = R m; called behind the gathers, by a found
// voxel only, never in mode 0.  Returns the correspondence's flag (0 no kept voxel, 3 the source point has no normal, 5 the covariance is
// not positive definite, 1 effective) and leaves w, e and k in o (zero, zero and 1 unless the flag is 1 - k as glin_point leaves it) and
// the voxel and its record in x; of o it writes nothing else.
template <class NormalOf>
DCREG_DEVFN uint8_t vlin_corr(const VoxMapDev &vm, const VlinArgs &a, uint32_t vidx, float qx, float qy, float qz, NormalOf normal_of,
                              GlinPoint &o, VlinPoint &x) {
#pragma clang fp contract(off)
    o.k = 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.e[k] = 0.0; x.mean[k] = 0.0;
        o.w[k][0] = o.w[k][1] = o.w[k][2] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) x.cov[k] = 0.0;
    x.vidx = vidx;
    if (vidx == kNoIdx) return 0;
    const float4 *rec = vm.recs + (size_t)vidx * kVmapRecWords;
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    const double mux = (double)r0.x, muy = (double)r0.y, muz = (double)r0.z;
    double s00 = (double)r0.w, s10 = (double)r1.x, s20 = (double)r1.y, s11 = (double)r1.z, s21 = (double)r1.w, s22 = (double)r2.x;
    x.mean[0] = mux; x.mean[1] = muy; x.mean[2] = muz;
    x.cov[0] = s00; x.cov[1] = s10; x.cov[2] = s20; x.cov[3] = s11; x.cov[4] = s21; x.cov[5] = s22;
    if (a.source_cov) {                                                    // (launch-uniform)
        double u[3];
        if (!normal_of(u)) return 3;
        const double ux = u[0], uy = u[1], uz = u[2];
        // S = C' + (I - c u u^T), lower triangle
        s00 = s00 + (1.0 - a.c * (ux * ux));
        s10 = s10 + (0.0 - a.c * (uy * ux));
        s11 = s11 + (1.0 - a.c * (uy * uy));
        s20 = s20 + (0.0 - a.c * (uz * ux));
        s21 = s21 + (0.0 - a.c * (uz * uy));
        s22 = s22 + (1.0 - a.c * (uz * uz));
    }
    // S = L L^T and W = L^-1: the third engine's formulas in its order (gicp.hpp glin_point)
    const double l00 = sqrt(s00);
    const double l10 = s10 / l00;
    const double l20 = s20 / l00;
    const double d11 = s11 - l10 * l10;
    const double l11 = sqrt(d11);
    const double l21 = (s21 - l20 * l10) / l11;
    const double d22 = (s22 - l20 * l20) - l21 * l21;
    const double l22 = sqrt(d22);
    if (!(s00 > 0.0 && d11 > 0.0 && d22 > 0.0)) return 5;
    const double w00 = 1.0 / l00, w11 = 1.0 / l11, w22 = 1.0 / l22;
    const double w10 = -(l10 * w00) * w11;
    const double w21 = -(l21 * w11) * w22;
    const double w20 = -(l20 * w00 + l21 * w10) * w22;
    o.w[0][0] = w00;
    o.w[1][0] = w10; o.w[1][1] = w11;
    o.w[2][0] = w20; o.w[2][1] = w21; o.w[2][2] = w22;
    o.e[0] = (double)qx - mux; o.e[1] = (double)qy - muy; o.e[2] = (double)qz - muz;
    if (a.robust) {                                                        // (launch-uniform) one factor per correspondence, as glin_point forms it
        const double r0_ = (o.w[0][0] * o.e[0] + o.w[0][1] * o.e[1]) + o.w[0][2] * o.e[2];
        const double r1_ = (o.w[1][0] * o.e[0] + o.w[1][1] * o.e[1]) + o.w[1][2] * o.e[2];
        const double r2_ = (o.w[2][0] * o.e[0] + o.w[2][1] * o.e[1]) + o.w[2][2] * o.e[2];
        const double m2 = (r0_ * r0_ + r1_ * r1_) + r2_ * r2_;
        o.k = robust_factor(a.robust, m2 / a.robust_c2);
    }
    return 1;
}

// One point of dcreg_linearize_voxels with "voxels_neighbors" = 1, up to its whitening matrix: the one correspondence with the voxel the
// transformed point falls into.  m4p: where the point's own kept normal lies (read in mode 1 only, and only by a point that found a voxel;
// null in mode 0).  Returns the flag (0 no kept voxel, 3 the source point has no normal, 5 the covariance is not positive definite,
// 1 effective).  o: m, w, e and k as glin_point leaves them (glin_block_rows reads them); with a robust kernel on (a.robust), a flag-1
// point leaves the kernel's factor at its squared whitened distance in o.k.
DCREG_DEVFN uint8_t vlin_point(const VoxMapDev &vm, const PoseArg &P, const VlinArgs &a, const float4 &s4, const float4 *m4p, GlinPoint &o,
                               VlinPoint &x) {
#pragma clang fp contract(off)
    const double px = (double)s4.x, py = (double)s4.y, pz = (double)s4.z;
    float qx, qy, qz;
    body_to_global(P, px, py, pz, qx, qy, qz);
    o.idx = kNoIdx; o.pos = kNoIdx; o.d2 = 0.f; o.n_eval = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.n[k] = 0.0; o.m[k] = 0.0; }
    return vlin_corr(vm, a, vmap_find(vm, qx, qy, qz), qx, qy, qz, [&](double (&u)[3]) { return vlin_normal(P, *m4p, o.m, u); }, o, x);
}

}  // namespace dcreg
