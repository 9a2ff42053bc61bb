// Per-thread device functions of the third engine (include/dcreg.h: dcreg_linearize_gicp): one source point against the map's kept
// normals AND the source's own - transform, exact 1-NN on the cell grid, radius gate (all three nlin_point's), then the plane-to-plane
// covariance of the pair formed from the two normals in registers, its Cholesky factor, the whitening matrix W = L^-1 and the three
// point-to-plane rows whose pseudo-normals are W's rows.  The rule is the header's, operation by operation; tests/gicp_ref.py states
// it in numpy.  Included by gicp.hip (the kernels) and, like normal_icp.hpp, compiled for the host under DCREG_HOST_EMUL by the test
// suite's replay (tests/host_emul/).  The device-only part at the end is the block tail of the engines with three rows per point
// (WaveGram, wave_gram3_mfma, glin_block_rows, glin_block_tail), shared with voxel_icp.hip.
#pragma once
#include "normal_icp.hpp"

namespace dcreg {

struct GlinArgs {
    double radius_sq;             // R^2 in double: the gate (double)d2 < R^2
    float bound_f;                // the cold search bound: the smallest float >= R^2
    int max_ring;                 // rings that cover it
    double c;                     // 1 - epsilon ("gicp_epsilon"), formed once on the host
    int robust = 0;               // "robust_kernel" (DCREG_ROBUST_*): 0 multiplies nothing
    double robust_c2 = 1.0;       // c * c of "gicp_robust_scale", formed once on the host
};

// what a point leaves for its rows and for the debug dump (flag 0: idx kNoIdx, d2 +inf; the normals as stored for every point that
// passed the radius gate; w and e are zero unless the flag is 1)
struct GlinPoint {
    uint32_t idx, pos;            // original index of the nearest point and its position in the sorted array (kNoIdx: none inside the bound)
    float d2;
    double n[3], m[3];            // the kept normal of the nearest map point, the kept normal of the source point
    double w[3][3];               // W = L^-1, lower triangular: row k is the pseudo-normal a_k
    double e[3];                  // (double)q - (double)t_j
    double k;                     // the robust kernel's factor for the point's three rows (1 with no kernel, and unless the flag is 1)
    uint32_t n_eval;              // candidates the search evaluated (host replay)
};

// One point of dcreg_linearize_gicp up to its whitening matrix.  warm_pos: as nlin_point's - it bounds the search, never decides it.
// normals: float4 per map point in index order; m4p: where the point's own kept normal lies (read after the two gathers, and only by a
// point that passed the radius gate: nothing of it is live across the search).  Returns the flag (0 radius gate, 2 the nearest map
// point has no normal, 3 the source point has none, 5 the covariance is not positive definite, 1 effective).  With a robust kernel on
// (a.robust), a flag-1 point also leaves the kernel's factor at its squared whitened distance in o.k.
DCREG_DEVFN uint8_t glin_point(const GridDev &g, RunList &rl, const float4 *normals, const PoseArg &P, const GlinArgs &a, const float4 &s4,
                               const float4 *m4p, uint32_t warm_pos, GlinPoint &o) {
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
    o.idx = kNoIdx; o.pos = kNoIdx; o.d2 = __builtin_inff(); o.n_eval = hp.n_eval;
    o.k = 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.n[k] = 0.0; o.m[k] = 0.0; o.e[k] = 0.0;
        o.w[k][0] = o.w[k][1] = o.w[k][2] = 0.0;
    }
    if (hp.pos == kNoIdx) return 0;
    const float d2 = __uint_as_float((uint32_t)(hp.key >> 32));
    if (!((double)d2 < a.radius_sq)) return 0;
    o.pos = hp.pos; o.idx = (uint32_t)hp.key; o.d2 = d2;
    const float4 tj = g.pts[hp.pos];
    const float4 n4 = normals[o.idx];
    const float4 m4 = *m4p;
    const double nx = (double)n4.x, ny = (double)n4.y, nz = (double)n4.z;
    const double mx = (double)m4.x, my = (double)m4.y, mz = (double)m4.z;
    o.n[0] = nx; o.n[1] = ny; o.n[2] = nz;
    o.m[0] = mx; o.m[1] = my; o.m[2] = mz;
    if (!(nlin_finite(n4.x) && nlin_finite(n4.y) && nlin_finite(n4.z))) return 2;
    if (!(nlin_finite(m4.x) && nlin_finite(m4.y) && nlin_finite(m4.z))) return 3;
    // u = R m, each component summed as body_to_global sums it
    const double ux = (P.R[0] * mx + P.R[1] * my) + P.R[2] * mz;
    const double uy = (P.R[3] * mx + P.R[4] * my) + P.R[5] * mz;
    const double uz = (P.R[6] * mx + P.R[7] * my) + P.R[8] * mz;
    // S = 2 I - c (n n^T + u u^T), lower triangle
    const double s00 = 2.0 - a.c * (nx * nx + ux * ux);
    const double s10 = 0.0 - a.c * (ny * nx + uy * ux);
    const double s11 = 2.0 - a.c * (ny * ny + uy * uy);
    const double s20 = 0.0 - a.c * (nz * nx + uz * ux);
    const double s21 = 0.0 - a.c * (nz * ny + uz * uy);
    const double s22 = 2.0 - a.c * (nz * nz + uz * uz);
    // S = L L^T
    const double l00 = sqrt(s00);
    const double l10 = s10 / l00;
    const double l20 = s20 / l00;
    const double d11 = s11 - l10 * l10;
    const double l11 = sqrt(d11);
    const double l21 = (s21 - l20 * l10) / l11;
    const double d22 = (s22 - l20 * l20) - l21 * l21;
    const double l22 = sqrt(d22);
    if (!(s00 > 0.0 && d11 > 0.0 && d22 > 0.0)) return 5;
    // W = L^-1
    const double w00 = 1.0 / l00, w11 = 1.0 / l11, w22 = 1.0 / l22;
    const double w10 = -(l10 * w00) * w11;
    const double w21 = -(l21 * w11) * w22;
    const double w20 = -(l20 * w00 + l21 * w10) * w22;
    o.w[0][0] = w00;
    o.w[1][0] = w10; o.w[1][1] = w11;
    o.w[2][0] = w20; o.w[2][1] = w21; o.w[2][2] = w22;
    o.e[0] = (double)qx - (double)tj.x; o.e[1] = (double)qy - (double)tj.y; o.e[2] = (double)qz - (double)tj.z;
    if (a.robust) {                                                        // (launch-uniform) one factor per point, from the three residuals as glin_row forms them
        const double r0 = (o.w[0][0] * o.e[0] + o.w[0][1] * o.e[1]) + o.w[0][2] * o.e[2];
        const double r1 = (o.w[1][0] * o.e[0] + o.w[1][1] * o.e[1]) + o.w[1][2] * o.e[2];
        const double r2 = (o.w[2][0] * o.e[0] + o.w[2][1] * o.e[1]) + o.w[2][2] * o.e[2];
        const double m2 = (r0 * r0 + r1 * r1) + r2 * r2;
        o.k = robust_factor(a.robust, m2 / a.robust_c2);
    }
    return 1;
}

// Row k of a flag-1 point: the second engine's row with weight 1 for the pseudo-normal a = (ax, ay, az), row k of W (its structural
// zeros are multiplied and added like any other value).  p: the source point, e: q - t_j.
DCREG_DEVFN void glin_row(const PoseArg &P, double px, double py, double pz, double ax, double ay, double az, double ex, double ey, double ez,
                          double (&row)[8]) {
#pragma clang fp contract(off)
    const double r = (ax * ex + ay * ey) + az * ez;
    const double m0 = (P.R[0] * ax + P.R[3] * ay) + P.R[6] * az;
    const double m1 = (P.R[1] * ax + P.R[4] * ay) + P.R[7] * az;
    const double m2 = (P.R[2] * ax + P.R[5] * ay) + P.R[8] * az;
    row[0] = py * m2 - pz * m1; row[1] = pz * m0 - px * m2; row[2] = px * m1 - py * m0;
    row[3] = m0; row[4] = m1; row[5] = m2;
    row[6] = -r;
    row[7] = r;
}

// ... with a robust kernel on: slots 0..6 times the point's factor (GlinPoint::k), slot 7 stays r_k
DCREG_DEVFN void glin_row_scale(double k, double (&row)[8]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 7; ++j) row[j] = k * row[j];
}

#if !defined(DCREG_HOST_EMUL)
// ---- the block tail of the engines with three rows per point (gicp.hip k_glin / k_glin_batch, voxel_icp.hip k_vlin): device only
}  // namespace dcreg
#include "kernels.hpp"
namespace dcreg {

// wave_gram_mfma (kernels.hpp) for several rows per lane, one pass each: pass() stages one row of all 64 lanes and runs the 8 MFMA steps on
// the accumulator the pass before left; end() makes the two DPP adds - the Gram matrix of all the rows the wave passed, summed in the fixed
// order (pass, step).  A pass's operand reads are other lanes' stores: within the wave the LDS executes in program order, and the wavefront
// fences keep the compiler from moving a pass's stores above the reads of the pass before (or its reads above its own stores).  Every lane
// of the wave makes every pass (a lane without a row passes zeros); a pass whose rows are all zero adds +0.0 products to an accumulator
// that started at +0.0, so leaving it out moves no bit.
struct WaveGram {
    const double *op;
    mfma_d4 acc;
    __device__ __forceinline__ void begin(const double *stage, int lane) {
        const int c16 = lane & 15, k = lane >> 4;
        op = stage + (2 * k + (c16 >> 3)) * kRowStride + (c16 & 7);
        acc = mfma_d4{0.0, 0.0, 0.0, 0.0};
    }
    __device__ __forceinline__ void pass(const double (&row)[8], double *stage, int lane) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // the reads of the pass before are over
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < 8; ++c) stage[lane * kRowStride + c] = row[c];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // every lane's row is staged
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            const double x = op[kb * 8 * kRowStride];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
        }
    }
    // u0 / u1 as wave_gram_mfma returns them
    __device__ __forceinline__ void end(int lane, double &u0, double &u1) const {
        const bool even = (lane & 15) < 8;
        u0 = even ? acc[0] : acc[2];
        u1 = even ? acc[1] : acc[3];
        u0 = dpp_add<0x128, 0xF>(u0);      // row_ror:8 - the lane holding the other half's block entry
        u1 = dpp_add<0x128, 0xF>(u1);
    }
};

// ... for three rows per lane: the rows of a pass are built just before it (row_of(pass, row)); the Gram matrix of the wave's 192 rows
template <class RowOf>
__device__ __forceinline__ void wave_gram3_mfma(RowOf row_of, double *stage, int lane, double &u0, double &u1) {
    WaveGram G;
    G.begin(stage, lane);
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        double row[8];
        row_of(pass, row);
        G.pass(row, stage, lane);
    }
    G.end(lane, u0, u1);
}

// What a block does with its waves' Gram matrices (u0 / u1 of WaveGram::end) and its points' two counts - eff: the lane's point is
// effective, inr: it has a correspondence at all: the wave's matrix and counts in LDS, added in wave order, and the block row at `out`
__device__ __forceinline__ void glin_block_tail(double u0, double u1, bool eff_pt, bool inr_pt, double (*gm)[64], double (*cnt)[2],
                                                double *__restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // (the wave's Gram matrix, M[a][b] at a * 8 + b, and its counts: what wave_rows_to_lds leaves)
    if ((lane & 15) < 8) {
        gm[wave][(lane >> 4) * 8 + (lane & 7)] = u0;
        gm[wave][32 + (lane >> 4) * 8 + (lane & 7)] = u1;
    }
    const unsigned long long eff = __builtin_amdgcn_ballot_w64(eff_pt), inr = __builtin_amdgcn_ballot_w64(inr_pt);
    if (lane == 0) { cnt[wave][0] = (double)__builtin_popcountll(eff); cnt[wave][1] = (double)__builtin_popcountll(inr); }
    __syncthreads();
    if (threadIdx.x < kSlots) out[threadIdx.x] = block_slot_sum(&gm[0][0], 64, cnt);
}

// What a block does with its points once glin_point has run (k_glin and k_glin_batch): the three rows of every flag-1 point through
// wave_gram3_mfma (stage: the wave's staging area of kWave * kRowStride doubles - a RunList that is free now serves; a lane past the cloud's end or with another flag than 1 carries
// zero rows), the wave's Gram matrix and counts in LDS, added in wave order, and the block row at `out`.  note(k, row): the dump's hook.
// robust: the launch's kernel (GlinArgs::robust); a row is then scaled by the factor glin_point left in o.k before it is noted and staged.
template <class Note>
__device__ __forceinline__ void glin_block_rows(const PoseArg &P, int robust, uint8_t flag, float sx, float sy, float sz, const GlinPoint &o, double *stage,
                                                double (*gm)[64], double (*cnt)[2], double *__restrict__ out, Note note) {
    const int lane = threadIdx.x & 63;
    auto row_of = [&](int k, double (&row)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = 0.0;
        if (flag == 1) {
            glin_row(P, (double)sx, (double)sy, (double)sz, o.w[k][0], o.w[k][1], o.w[k][2], o.e[0], o.e[1], o.e[2], row);
            if (robust) glin_row_scale(o.k, row);        // (launch-uniform; with no kernel nothing is multiplied)
        }
        note(k, row);
    };
    double u0, u1;
    wave_gram3_mfma(row_of, stage, lane, u0, u1);
    glin_block_tail(u0, u1, flag == 1, flag != 0, gm, cnt, out);
}
#endif  // !DCREG_HOST_EMUL

}  // namespace dcreg
