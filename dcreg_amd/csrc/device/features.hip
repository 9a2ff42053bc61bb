// FPFH descriptors and feature-space matching on the device (include/dcreg.h: dcreg_fpfh*, dcreg_target_fpfh*, dcreg_feature_match*): the
// first two stages of a correspondence-based global alignment, with the rules of the header, bitwise the numpy reference of
// tests/fpfh_ref.py up to the header's one freedom (atan2 at an interior bin edge of theta).
//   (cloud form)    the cloud packed, the points without a finite normal made non-finite (k_fpfh_unuse), the used points compacted and
//                   indexed: the shared first step of scratch.hip (cloud_index_used); normals == NULL: dcreg_normals first,
//                   on the same index (normals.hip normals_to_scratch).  The map form searches the map's own index
//   k_fpfh_spfh<K>  one lane per used point, in the index's cell order: the ring walk of k_nrm with its heap (heap_nrm.hpp); the lane
//                   writes its neighbour list - position and d2, rank order, k slots - and walks it once more for the pair features.
//                   The 33 counters are indexed by a computed bin: they live as bytes in the lane's column of the wave's RunList, which
//                   is free once the search is over (9 words of s[][lane]), never in a register array
//   k_fpfh_sum      behind it (every point needs its neighbours' counts): one lane per used point gathers them through the list and
//                   accumulates 33 doubles in rank order (statically indexed: registers), normalises and writes at the input index
//   k_match         one query row per lane, its 33 values as doubles in registers; the candidates go through LDS in tiles of kMatchTile
//                   rows widened to double once, every lane reading the same row (a broadcast); the lane keeps its best two (D, j).
//                   blockIdx.y takes a range of candidates ("split"): many blocks for few queries against many candidates
//   k_match_merge   the partial winners of the splits merged in ascending split order - candidates arrive in ascending j everywhere, so
//                   a strict < keeps the lowest index among equal distances and the result does not depend on the split
//   (mutual)        k_match + k_match_merge with the roles swapped, then k_match_mutual
//   (radius rule)   dcreg_fpfh_radius*: the same cloud and map forms with every point within the radius as the support, through kernels of
//                   their own - one wave per point, integer sums (k_fpfh_rspfh, k_fpfh_rsum; described where they stand)
// A result depends on the inputs and the parameters only: the index decides how fast the neighbours are found, never which.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../../include/dcreg_debug.h"
#include "context.hpp"
#include "heap_nrm.hpp"

// every multiply and add below rounds once: the rules are stated operation by operation
#pragma clang fp contract(off)

namespace dcreg {
namespace {

constexpr int kMinK = 3, kMaxK = 32;
constexpr int kDim = 33;                                 // DCREG_FPFH_DIM
constexpr int kCountWords = 9;                           // 33 byte counters
constexpr int kMatchBlock = 256, kMatchTile = 128;       // queries per block, candidate rows per LDS tile (33 KiB of doubles)
constexpr double kPi = 3.14159265358979323846;

DCREG_DEVFN bool finitef(float x) { return fabsf(x) <= 3.4028235e38f; }

// a point without a finite normal is not used: its x becomes NaN before the used points are compacted
static __global__ void k_fpfh_unuse(float4 *__restrict__ pts, int64_t n, const float *__restrict__ nrm, int64_t nstride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *q = nrm + (size_t)i * (size_t)nstride;
    if (!(finitef(q[0]) && finitef(q[1]) && finitef(q[2]))) pts[i].x = __builtin_nanf("");
}

// the map form: cnt[2] += kept normals that are not finite (one atomic per wave)
static __global__ void k_fpfh_bad(const float4 *__restrict__ nrm, int64_t n, unsigned long long *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) { const float4 v = nrm[i]; bad = !(finitef(v.x) && finitef(v.y) && finitef(v.z)); }
    const unsigned long long B = __ballot(bad);
    if (B != 0ull && (int)(threadIdx.x & 63) == __ffsll(B) - 1) atomicAdd(cnt + 2, (unsigned long long)__popcll(B));
}

DCREG_DEVFN int fpfh_bin(double x) { return (int)fmin(fmax(floor(x), 0.0), 10.0); }

// The body of one lane of k_fpfh_spfh: the point at position i of the index's cell order (its input index in w).  nrm: the normals by
// input index, nstride floats apart.  nb_pos / nb_d2: [slot][point] lists of nq points; a slot that was never filled keeps position
// kNoIdx.  spfh: 3 uint4 per point - nine words of byte counts (bin b in byte b & 3 of word b >> 2), then m | has << 8
// (one body for the cloud form and the map form: they differ in where the index and the normals come from)
template <int K>
DCREG_DEVFN void spfh_point(uint32_t i, uint32_t nq, const float4 s4, const GridDev &g, RunList &rl, float bound_f, int max_ring, int k,
                            const float *__restrict__ nrm, int64_t nstride, uint32_t *nb_pos, float *nb_d2, uint4 *__restrict__ spfh) {
    HeapNrm<K> hp;
    hp.k = k;
    knn_search<HeapNrm<K>>(g, rl, s4.x, s4.y, s4.z, bound_f, max_ring, hp);
    int m = 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j >= K - k) {
            const size_t at = (size_t)(j - (K - k)) * nq + i;
            nb_pos[at] = hp.pos[j];
            nb_d2[at] = __uint_as_float((uint32_t)(hp.key[j] >> 32));
            m += hp.pos[j] != kNoIdx ? 1 : 0;         // (sorted: the filled slots come first)
        }
    // the search is over: the lane's column of the run list holds its 33 counters now
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int w = 0; w < kCountWords; ++w) rl.s[w][lane] = 0u;
    const uint32_t self = __float_as_uint(s4.w);
    const float *np_ = nrm + (size_t)self * (size_t)nstride;
    const double px = (double)s4.x, py = (double)s4.y, pz = (double)s4.z;
    const double npx = (double)np_[0], npy = (double)np_[1], npz = (double)np_[2];
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
        const size_t at = (size_t)j * nq + i;
        const float d2 = nb_d2[at];
        if (!(d2 > 0.f)) continue;
        const float4 c = g.pts[nb_pos[at]];
        const float *nq_ = nrm + (size_t)__float_as_uint(c.w) * (size_t)nstride;
        const double nqx = (double)nq_[0], nqy = (double)nq_[1], nqz = (double)nq_[2];
        double dx = (double)c.x - px, dy = (double)c.y - py, dz = (double)c.z - pz;
        const double f4 = sqrt((dx * dx + dy * dy) + dz * dz);
        if (f4 == 0.0) continue;
        const double a1 = ((npx * dx + npy * dy) + npz * dz) / f4;
        const double a2 = ((nqx * dx + nqy * dy) + nqz * dz) / f4;
        const bool sw = fabs(a1) < fabs(a2);
        const double n1x = sw ? nqx : npx, n1y = sw ? nqy : npy, n1z = sw ? nqz : npz;
        const double n2x = sw ? npx : nqx, n2y = sw ? npy : nqy, n2z = sw ? npz : nqz;
        const double phi = sw ? -a2 : a1;
        if (sw) { dx = -dx; dy = -dy; dz = -dz; }
        double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
        const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
        if (vn == 0.0) continue;
        vx = vx / vn; vy = vy / vn; vz = vz / vn;
        const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
        const double alpha = (vx * n2x + vy * n2y) + vz * n2z;
        const double theta = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
        const int b0 = fpfh_bin(11.0 * ((theta + kPi) / (2.0 * kPi)));
        const int b1 = 11 + fpfh_bin(11.0 * ((alpha + 1.0) * 0.5));
        const int b2 = 22 + fpfh_bin(11.0 * ((phi + 1.0) * 0.5));
        rl.s[b0 >> 2][lane] += 1u << ((b0 & 3) * 8);
        rl.s[b1 >> 2][lane] += 1u << ((b1 & 3) * 8);
        rl.s[b2 >> 2][lane] += 1u << ((b2 & 3) * 8);
    }
    uint32_t w[kCountWords], any = 0u;
#pragma unroll
    for (int u = 0; u < kCountWords; ++u) { w[u] = rl.s[u][lane]; any |= w[u]; }
    const uint32_t has = (m >= 2 && any != 0u) ? 1u : 0u;
    spfh[3 * (size_t)i] = make_uint4(w[0], w[1], w[2], w[3]);
    spfh[3 * (size_t)i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    spfh[3 * (size_t)i + 2] = make_uint4(w[8], (uint32_t)m | (has << 8), 0u, 0u);
}

template <int K>
static __global__ __launch_bounds__(kBlock) void k_fpfh_spfh(const float4 *__restrict__ q, uint32_t n, GridDev g, float bound_f, int max_ring, int k,
                                                             const float *__restrict__ nrm, int64_t nstride, uint32_t *nb_pos, float *nb_d2,
                                                             uint4 *__restrict__ spfh) {
    __shared__ RunList runs[kBlock / kWave];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    spfh_point<K>(i, n, q[i], g, runs[threadIdx.x / kWave], bound_f, max_ring, k, nrm, nstride, nb_pos, nb_d2, spfh);
}

// One lane per used point, in cell order: F_b over the list in rank order, the three blocks normalised, 33 floats at the point's input
// index.  cnt[0] += points with a descriptor, cnt[1] += empty points (one atomic pair per wave)
static __global__ __launch_bounds__(kBlock) void k_fpfh_sum(const float4 *__restrict__ q, uint32_t n, int k, const uint32_t *__restrict__ nb_pos,
                                                            const float *__restrict__ nb_d2, const uint4 *__restrict__ spfh, float *__restrict__ out,
                                                            unsigned long long *__restrict__ cnt) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    // (-0.0 is the identity of the IEEE addition: the sums start with their first term)
    double acc[kDim];
#pragma unroll
    for (int b = 0; b < kDim; ++b) acc[b] = -0.0;
#pragma unroll 1
    for (int j = 0; j < k; ++j) {
        const size_t at = (size_t)j * n + i;
        const uint32_t pos = nb_pos[at];
        if (pos == kNoIdx) break;
        const float d2 = nb_d2[at];
        if (!(d2 > 0.f)) continue;
        const uint4 r2 = spfh[3 * (size_t)pos + 2];
        if ((r2.y >> 8) == 0u) continue;
        const uint4 r0 = spfh[3 * (size_t)pos], r1 = spfh[3 * (size_t)pos + 1];
        const uint32_t w[kCountWords] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
        const double wt = 1.0 / (double)d2;
        const double sc = 100.0 / (double)((int)(r2.y & 0xffu) - 1);
#pragma unroll
        for (int b = 0; b < kDim; ++b) {
            const double s = (double)((w[b >> 2] >> ((b & 3) * 8)) & 0xffu) * sc;
            acc[b] = acc[b] + wt * s;
        }
    }
    double S[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        double s = acc[11 * t];
#pragma unroll
        for (int b = 1; b < 11; ++b) s = s + acc[11 * t + b];
        S[t] = s;
    }
    const bool full = S[0] > 0.0 && S[1] > 0.0 && S[2] > 0.0;
    if (full) {
        float *o = out + (size_t)kDim * (size_t)__float_as_uint(q[i].w);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const double f = 100.0 / S[t];
#pragma unroll
            for (int b = 0; b < 11; ++b) o[11 * t + b] = (float)(acc[11 * t + b] * f);
        }
    }
    const unsigned long long A = __ballot(true), F = __ballot(full);
    if ((int)(threadIdx.x & 63) == __ffsll(A) - 1) {
        const unsigned long long nf = (unsigned long long)__popcll(F), ne = (unsigned long long)__popcll(A) - nf;
        if (nf) atomicAdd(cnt, nf);
        if (ne) atomicAdd(cnt + 1, ne);
    }
}

// dcreg_fpfh_debug_counts: the SPFH record of the point at sorted position i, 36 bytes at its input index (33 counts, m, has, 0)
static __global__ void k_fpfh_counts(const float4 *__restrict__ q, uint32_t n, const uint4 *__restrict__ spfh, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r0 = spfh[3 * (size_t)i], r1 = spfh[3 * (size_t)i + 1], r2 = spfh[3 * (size_t)i + 2];
    uint32_t *o = out + (size_t)kCountWords * (size_t)__float_as_uint(q[i].w);
    o[0] = r0.x; o[1] = r0.y; o[2] = r0.z; o[3] = r0.w; o[4] = r1.x; o[5] = r1.y; o[6] = r1.z; o[7] = r1.w;
    o[8] = (r2.x & 0xffu) | ((r2.y & 0xffu) << 8) | ((r2.y >> 8) << 16);
}

// ------------------------------------------------------------------------------------------ descriptors over a radius support
// dcreg_fpfh_radius*: every used point within the radius is a neighbour - hundreds per point, so ONE WAVE serves one point and its lanes
// take the candidates of the ball side by side.  Both sums of the rule are integers: no order is part of it, and the lanes' shares meet in
// LDS counters (pass 1) and in a butterfly of 64-bit adds (pass 2).
//   ball_walk      the (y, z) rows of the grid that the ball reaches, 64 per batch, one per lane: the row's x-run trimmed to the ball in
//                  sub-cells (conservative; the float d2 < R2 of the rule decides).  The runs of a batch are laid end to end - their
//                  starts and an exclusive scan of their lengths in LDS - and the lanes walk that one sequence 64 candidates a trip,
//                  each finding its run by six halving steps: dense lanes whether a row holds two points or two hundred
//   k_fpfh_rspfh   pass 1: m by ballot, the pair features in the lanes whose candidate is inside, 33 LDS counters per wave bumped by
//                  ds_add; then lane b writes q_b, and the counts for dcreg_fpfh_radius_debug_counts.  Past the cap the walk stops
//   k_fpfh_rsum    pass 2, a kernel boundary behind: the same walk; a lane whose candidate counts gathers its record (nine 16-byte loads,
//                  consecutive positions in consecutive lanes) and adds w q_b to 33 statically indexed uint64 registers; the wave's
//                  totals by xor shuffles, lane b normalises and writes value b at the input index
//   k_fpfh_rstats  one lane per used point: n_out, n_crowded, m_max, m_sum (one atomic each per wave)
// Per used point 144 + 132 bytes, whatever the radius.
constexpr int kRecWords = 36;                            // q[33], m, has, 0: nine uint4
constexpr int kTeams = kBlock / kWave;                   // points per block
constexpr double kWeightOne = 16384.0, kWeightCap = 1073741824.0;      // 2^14, 2^30

struct BallLds { uint32_t start[kWave], base[kWave], bins[kDim]; };

DCREG_DEVFN void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// floor(x) as a cell index of an axis of n cells, clamped as k_cell_keys clamps a point's
DCREG_DEVFN int ball_cell(double x, int n) { return (int)fmin(fmax(floor(x), 0.0), (double)(n - 1)); }

// Every point of the grid that can have d2 < R2 from (qx, qy, qz), a point of the grid itself, goes through visit(position, valid) once:
// all 64 lanes call it together, valid says whether the lane holds a candidate (position 0 otherwise).  visit returns whether to stop,
// the same in every lane.  Margins: 1e-5 relative and 1e-4 of a (sub-)cell, against 1e-7 of float rounding in d2
template <class Visit>
DCREG_DEVFN void ball_walk(const GridDev &g, float qx, float qy, float qz, float R2, BallLds &L, Visit &&visit) {
    const int lane = threadIdx.x & (kWave - 1);
    const int nxf = g.nx * g.sx;
    const double fxs = ((double)qx - g.ox) * g.inv_h * (double)g.sx, fy = ((double)qy - g.oy) * g.inv_h, fz = ((double)qz - g.oz) * g.inv_h;
    const double reach = sqrt((double)R2) * g.inv_h * 1.00001 + 1e-4;                  // cells
    const int cy = ball_cell(fy, g.ny), cz = ball_cell(fz, g.nz);
    const int y0 = ball_cell(fy - reach, g.ny), y1 = ball_cell(fy + reach, g.ny), z0 = ball_cell(fz - reach, g.nz), z1 = ball_cell(fz + reach, g.nz);
    const int nyr = y1 - y0 + 1, nrows = nyr * (z1 - z0 + 1);
    for (int r0 = 0; r0 < nrows; r0 += kWave) {
        const int r = r0 + lane;
        uint32_t s = 0u, len = 0u;
        if (r < nrows) {
            const int z = z0 + r / nyr, y = y0 + r % nyr;
            // the row's slab: its distance from the query in y and z (cells), then what is left of the ball along x
            const double gy = y < cy ? fy - (double)(y + 1) : (y > cy ? (double)y - fy : 0.0);
            const double gz = z < cz ? fz - (double)(z + 1) : (z > cz ? (double)z - fz : 0.0);
            const double left = (double)R2 - ((gy * gy + gz * gz) * (g.h * g.h)) * 0.99999;
            if (left >= 0.0) {
                const double rx = sqrt(left) * g.inv_h * (double)g.sx * 1.00001 + 1e-4;      // sub-cells
                const int x0 = ball_cell(fxs - rx, nxf), x1 = ball_cell(fxs + rx, nxf);
                const size_t row = ((size_t)z * (size_t)g.ny + (size_t)y) * (size_t)nxf;
                s = g.cell_start[row + (size_t)x0];
                len = g.cell_start[row + (size_t)x1 + 1] - s;
            }
        }
        uint32_t incl = len;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o);
            incl += lane >= o ? v : 0u;
        }
        const uint32_t total = __builtin_amdgcn_readlane(incl, kWave - 1);
        wave_sync();                                      // (the lists of the batch before are read no more)
        L.start[lane] = s; L.base[lane] = incl - len;
        wave_sync();
        for (uint32_t t0 = 0; t0 < total; t0 += kWave) {
            const uint32_t t = t0 + lane;
            const bool valid = t < total;
            // the last run that starts at or before t: it is not empty, because the next one starts beyond t
            int rr = 0;
#pragma unroll
            for (int step = kWave / 2; step > 0; step >>= 1) rr += L.base[rr + step] <= t ? step : 0;
            const uint32_t pos = valid ? L.start[rr] + (t - L.base[rr]) : 0u;
            if (visit(pos, valid)) return;
        }
    }
}

// the three bins of the pair (p, q), the pair features of the header's FPFH rule; false: the pair is skipped (f4 == 0 or vn == 0)
DCREG_DEVFN bool pair_bins(double px, double py, double pz, double npx, double npy, double npz, const float4 c, const float *__restrict__ nq_, int &b0,
                           int &b1, int &b2) {
    const double nqx = (double)nq_[0], nqy = (double)nq_[1], nqz = (double)nq_[2];
    double dx = (double)c.x - px, dy = (double)c.y - py, dz = (double)c.z - pz;
    const double f4 = sqrt((dx * dx + dy * dy) + dz * dz);
    if (f4 == 0.0) return false;
    const double a1 = ((npx * dx + npy * dy) + npz * dz) / f4;
    const double a2 = ((nqx * dx + nqy * dy) + nqz * dz) / f4;
    const bool sw = fabs(a1) < fabs(a2);
    const double n1x = sw ? nqx : npx, n1y = sw ? nqy : npy, n1z = sw ? nqz : npz;
    const double n2x = sw ? npx : nqx, n2y = sw ? npy : nqy, n2z = sw ? npz : nqz;
    const double phi = sw ? -a2 : a1;
    if (sw) { dx = -dx; dy = -dy; dz = -dz; }
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
    const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
    if (vn == 0.0) return false;
    vx = vx / vn; vy = vy / vn; vz = vz / vn;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
    const double alpha = (vx * n2x + vy * n2y) + vz * n2z;
    const double theta = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
    b0 = fpfh_bin(11.0 * ((theta + kPi) / (2.0 * kPi)));
    b1 = 11 + fpfh_bin(11.0 * ((alpha + 1.0) * 0.5));
    b2 = 22 + fpfh_bin(11.0 * ((phi + 1.0) * 0.5));
    return true;
}

// Pass 1.  Wave w of block b: the point at position 4 b + w of the index's cell order.  rec: kRecWords words per point (q_b, then the m
// that is reported - min(m, cap + 1) -, then has); counts: 33 words per point
static __global__ __launch_bounds__(kBlock) void k_fpfh_rspfh(const float4 *__restrict__ q, uint32_t n, GridDev g, float R2, uint32_t cap,
                                                              const float *__restrict__ nrm, int64_t nstride, uint32_t *__restrict__ rec,
                                                              uint32_t *__restrict__ counts) {
    __shared__ BallLds lds[kTeams];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x & (kWave - 1);
    const uint32_t i = blockIdx.x * kTeams + wave;
    if (i >= n) return;
    BallLds &L = lds[wave];
    if (lane < (uint32_t)kDim) L.bins[lane] = 0u;
    wave_sync();
    const float4 s4 = q[i];
    const float *np_ = nrm + (size_t)__float_as_uint(s4.w) * (size_t)nstride;
    const double px = (double)s4.x, py = (double)s4.y, pz = (double)s4.z;
    const double npx = (double)np_[0], npy = (double)np_[1], npz = (double)np_[2];
    uint32_t m = 0u;
    ball_walk(g, s4.x, s4.y, s4.z, R2, L, [&](uint32_t pos, bool valid) {
        const float4 c = g.pts[pos];
        const float d2 = dist2_nofma(s4.x, s4.y, s4.z, c);
        const bool in = valid && d2 < R2;
        m += (uint32_t)__popcll(__ballot(in));
        if (in && d2 > 0.f) {
            int b0, b1, b2;
            if (pair_bins(px, py, pz, npx, npy, npz, c, nrm + (size_t)__float_as_uint(c.w) * (size_t)nstride, b0, b1, b2)) {
                atomicAdd(&L.bins[b0], 1u); atomicAdd(&L.bins[b1], 1u); atomicAdd(&L.bins[b2], 1u);
            }
        }
        return m > cap;
    });
    wave_sync();
    const bool crowded = m > cap;
    const uint32_t cb = (lane < (uint32_t)kDim && !crowded) ? L.bins[lane] : 0u;
    const bool has = m >= 2u && __ballot(cb != 0u) != 0ull;
    // c_b <= m - 1 <= 65534: c_b << 16 fits 32 bits
    uint32_t word = has ? (cb << 16) / (m - 1u) : 0u;
    if (lane == (uint32_t)kDim) word = crowded ? cap + 1u : m;
    if (lane == (uint32_t)kDim + 1u) word = has ? 1u : 0u;
    if (lane < (uint32_t)kRecWords) rec[(size_t)kRecWords * i + lane] = word;
    if (lane < (uint32_t)kDim) counts[(size_t)kDim * i + lane] = cb;
}

// Pass 2.  The same wave for the same point; rec as uint4, nine per point.  A crowded point walks nothing and stays NaN
static __global__ __launch_bounds__(kBlock) void k_fpfh_rsum(const float4 *__restrict__ q, uint32_t n, GridDev g, float R2, uint32_t cap,
                                                             const uint4 *__restrict__ rec, float *__restrict__ out) {
    __shared__ BallLds lds[kTeams];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x & (kWave - 1);
    const uint32_t i = blockIdx.x * kTeams + wave;
    if (i >= n) return;
    const float4 s4 = q[i];
    if (rec[9 * (size_t)i + 8].y > cap) return;
    unsigned long long acc[kDim];
#pragma unroll
    for (int b = 0; b < kDim; ++b) acc[b] = 0ull;
    const double R2d = (double)R2;
    ball_walk(g, s4.x, s4.y, s4.z, R2, lds[wave], [&](uint32_t pos, bool valid) {
        const float4 c = g.pts[pos];
        const float d2 = dist2_nofma(s4.x, s4.y, s4.z, c);
        if (valid && d2 < R2 && d2 > 0.f) {
            const uint4 *r = rec + 9 * (size_t)pos;
            const uint4 r8 = r[8];
            if (r8.z != 0u) {
                // one IEEE division; the multiply is by a power of two; the clamp before the conversion (the quotient may pass 2^64)
                const uint32_t w = (uint32_t)fmin(floor((R2d / (double)d2) * kWeightOne), kWeightCap);
                uint4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = r[u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    acc[4 * u] += (unsigned long long)w * v[u].x; acc[4 * u + 1] += (unsigned long long)w * v[u].y;
                    acc[4 * u + 2] += (unsigned long long)w * v[u].z; acc[4 * u + 3] += (unsigned long long)w * v[u].w;
                }
                acc[32] += (unsigned long long)w * r8.x;
            }
        }
        return false;
    });
#pragma unroll
    for (int b = 0; b < kDim; ++b) {
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) acc[b] += __shfl_xor(acc[b], o);
    }
    unsigned long long S[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        S[t] = 0ull;
#pragma unroll
        for (int b = 0; b < 11; ++b) S[t] += acc[11 * t + b];
    }
    if (S[0] == 0ull || S[1] == 0ull || S[2] == 0ull) return;
    unsigned long long F = 0ull, St = 1ull;
#pragma unroll
    for (int b = 0; b < kDim; ++b)
        if (lane == (uint32_t)b) { F = acc[b]; St = S[b / 11]; }
    if (lane < (uint32_t)kDim) out[(size_t)kDim * (size_t)__float_as_uint(s4.w) + lane] = (float)((double)F * (100.0 / (double)St));
}

// cnt[0] += points with a descriptor, cnt[1] += crowded points, cnt[2] = max(cnt[2], m), cnt[3] += m (one atomic each per wave)
static __global__ void k_fpfh_rstats(const float4 *__restrict__ q, uint32_t n, uint32_t cap, const uint32_t *__restrict__ rec, const float *__restrict__ out,
                                     unsigned long long *__restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long m = 0ull;
    bool full = false;
    if (i < n) {
        m = rec[(size_t)kRecWords * i + kDim];
        const float f = out[(size_t)kDim * (size_t)__float_as_uint(q[i].w)];
        full = f == f;
    }
    const unsigned long long Fm = __ballot(full), Cm = __ballot(m > (unsigned long long)cap);
    unsigned long long mx = m, sum = m;
    for (int o = 32; o > 0; o >>= 1) { mx = max(mx, __shfl_xor(mx, o)); sum += __shfl_xor(sum, o); }
    if ((threadIdx.x & 63) == 0) {
        if (Fm) atomicAdd(cnt, (unsigned long long)__popcll(Fm));
        if (Cm) atomicAdd(cnt + 1, (unsigned long long)__popcll(Cm));
        atomicMax(cnt + 2, mx);
        atomicAdd(cnt + 3, sum);
    }
}

// dcreg_fpfh_radius_debug_counts: 35 words at the input index of the point at sorted position i (33 counts, m, has)
static __global__ void k_fpfh_rcounts(const float4 *__restrict__ q, uint32_t n, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ counts,
                                      uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t *o = out + (size_t)(kDim + 2) * (size_t)__float_as_uint(q[i].w);
    for (int b = 0; b < kDim; ++b) o[b] = counts[(size_t)kDim * i + b];
    o[kDim] = rec[(size_t)kRecWords * i + kDim];
    o[kDim + 1] = rec[(size_t)kRecWords * i + kDim + 1];
}

// ------------------------------------------------------------------------------------------ matching
// flag[i] = row i holds 33 finite values; *cnt += their number (one atomic per wave)
static __global__ void k_match_valid(const float *__restrict__ rows, int64_t n, int64_t stride, uint8_t *__restrict__ flag,
                                     unsigned long long *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const float *r = rows + (size_t)i * (size_t)stride;
        ok = true;
        for (int c = 0; c < kDim; ++c) ok = ok && finitef(r[c]);
        flag[i] = ok ? 1 : 0;
    }
    const unsigned long long V = __ballot(ok);
    if (V != 0ull && (int)(threadIdx.x & 63) == __ffsll(V) - 1) atomicAdd(cnt, (unsigned long long)__popcll(V));
}

// the running best two of a lane: candidates arrive in ascending j, so strict comparisons rank by (D, j)
DCREG_DEVFN void best_two(double D, int32_t j, double &d1, int32_t &j1, double &d2, int32_t &j2) {
    // (selects, not branches: behind branches the compiler addresses the four values through memory)
    const bool first = D < d1, second = D < d2;
    d2 = first ? d1 : (second ? D : d2); j2 = first ? j1 : (second ? j : j2);
    d1 = first ? D : d1; j1 = first ? j : j1;
}

// Block (x, y): queries [256 x, 256 x + 256) of a against the candidates [chunk y, chunk y + chunk) of b; ok_b: b's valid flags.  The
// partial winners of split y and query i go to part_d[2 (y n_a + i) ..] (D1, D2) and part_i[2 (y n_a + i) ..] (j1, j2; -1: none).  A
// query with a non-finite value computes NaN distances, which win nothing
static __global__ __launch_bounds__(kMatchBlock) void k_match(const float *__restrict__ a, uint32_t n_a, int64_t stride_a, const float *__restrict__ b,
                                                              uint32_t n_b, int64_t stride_b, const uint8_t *__restrict__ ok_b, uint32_t chunk,
                                                              double *__restrict__ part_d, int32_t *__restrict__ part_i) {
    __shared__ double tile[kMatchTile * kDim];
    __shared__ uint8_t ok[kMatchTile];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * kMatchBlock + tid;
    const bool live = i < n_a;
    double q[kDim];
    {
        const float *r = a + (size_t)(live ? i : 0u) * (size_t)stride_a;
#pragma unroll
        for (int c = 0; c < kDim; ++c) q[c] = (double)r[c];
    }
    const uint32_t j_begin = blockIdx.y * chunk, j_end = n_b - j_begin > chunk ? j_begin + chunk : n_b;      // (j_begin < n_b: the grid's y)
    double d1 = __builtin_inf(), d2 = __builtin_inf();
    int32_t j1 = -1, j2 = -1;
    for (uint32_t t0 = j_begin; t0 < j_end; t0 += kMatchTile) {
        const uint32_t rows = min((uint32_t)kMatchTile, j_end - t0);
        __syncthreads();                                  // (the tile of the trip before is read no more)
        for (uint32_t e = tid; e < rows * kDim; e += kMatchBlock) {
            const uint32_t r = e / kDim, c = e - r * kDim;
            tile[e] = (double)b[(size_t)(t0 + r) * (size_t)stride_b + c];
        }
        if (tid < rows) ok[tid] = ok_b[t0 + tid];
        __syncthreads();
        for (uint32_t r = 0; r < rows; ++r) {
            if (!ok[r]) continue;                         // (uniform: every lane reads the same flag)
            const double *row = tile + r * kDim;
            double x = q[0] - row[0];
            double D = x * x;
#pragma unroll
            for (int c = 1; c < kDim; ++c) { x = q[c] - row[c]; D = D + x * x; }
            best_two(D, (int32_t)(t0 + r), d1, j1, d2, j2);
        }
    }
    if (live) {
        const size_t at = 2 * ((size_t)blockIdx.y * n_a + i);
        part_d[at] = d1; part_d[at + 1] = d2;
        part_i[at] = j1; part_i[at + 1] = j2;
    }
}

// the splits' winners of query i merged in ascending split order; an invalid query gets -1 and NaN.  Any output may be null
static __global__ void k_match_merge(uint32_t n_a, uint32_t n_split, const double *__restrict__ part_d, const int32_t *__restrict__ part_i,
                                     const uint8_t *__restrict__ ok_a, int32_t *__restrict__ idx, double *__restrict__ dist, int32_t *__restrict__ idx2,
                                     double *__restrict__ dist2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_a) return;
    double d1 = __builtin_inf(), d2 = __builtin_inf();
    int32_t j1 = -1, j2 = -1;
    for (uint32_t s = 0; s < n_split; ++s) {
        const size_t at = 2 * ((size_t)s * n_a + i);
        if (part_i[at] >= 0) best_two(part_d[at], part_i[at], d1, j1, d2, j2);
        if (part_i[at + 1] >= 0) best_two(part_d[at + 1], part_i[at + 1], d1, j1, d2, j2);
    }
    if (!ok_a[i]) { d1 = d2 = __builtin_nan(""); j1 = j2 = -1; }
    if (idx) idx[i] = j1;
    if (dist) dist[i] = d1;
    if (idx2) idx2[i] = j2;
    if (dist2) dist2[i] = d2;
}

// mutual[i] = the best row of a for b[idx[i]] is i; cnt[2] += their number
static __global__ void k_match_mutual(uint32_t n_a, const int32_t *__restrict__ idx, const int32_t *__restrict__ idx_b, uint8_t *__restrict__ mutual,
                                      unsigned long long *__restrict__ cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool mu = false;
    if (i < n_a) {
        const int32_t j = idx[i];
        mu = j >= 0 && idx_b[j] == (int32_t)i;
        mutual[i] = mu ? 1 : 0;
    }
    const unsigned long long M = __ballot(mu);
    if (M != 0ull && (int)(threadIdx.x & 63) == __ffsll(M) - 1) atomicAdd(cnt + 2, (unsigned long long)__popcll(M));
}

// ------------------------------------------------------------------------------------------ descriptors: the host side
// which rule a descriptor call follows: the k nearest (p) or the radius support (rp), with the info block of that rule
struct FpfhRule {
    const dcreg_fpfh_params *p = nullptr;
    dcreg_fpfh_info *info = nullptr;
    const dcreg_fpfh_radius_params *rp = nullptr;
    dcreg_fpfh_radius_info *rinfo = nullptr;
    bool radius = false;
    double hint() const { return radius ? rp->radius : p->search_radius; }            // the index's cell edge is capped by it
    void clear_info() const {
        if (info) std::memset(info, 0, sizeof(*info));
        if (rinfo) std::memset(rinfo, 0, sizeof(*rinfo));
    }
};

int fpfh_check(dcreg_ctx *c, const dcreg_fpfh_params *p) {
    if (!p) { c->fail("null fpfh parameters"); return DCREG_E_INVALID; }
    if (p->k < kMinK || p->k > kMaxK) { c->fail("fpfh k is %d: %d .. %d expected", p->k, kMinK, kMaxK); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->search_radius) && p->search_radius >= 0.0)) { c->fail("fpfh search_radius is %g: finite and >= 0 expected", p->search_radius); return DCREG_E_INVALID; }
    return DCREG_OK;
}

constexpr int kMinCap = 2, kMaxCap = 65535;
int fpfh_radius_check(dcreg_ctx *c, const dcreg_fpfh_radius_params *p) {
    if (!p) { c->fail("null fpfh radius parameters"); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->radius) && p->radius > 0.0)) { c->fail("fpfh radius is %g: finite and > 0 expected", p->radius); return DCREG_E_INVALID; }
    const float R2 = (float)(p->radius * p->radius);
    if (!(R2 > 0.f && R2 < 3.0e38f)) { c->fail("fpfh radius is %g: its square is not a float in (0, 3.0e38)", p->radius); return DCREG_E_INVALID; }
    if (p->max_neighbors < kMinCap || p->max_neighbors > kMaxCap) { c->fail("fpfh max_neighbors is %d: %d .. %d expected", p->max_neighbors, kMinCap, kMaxCap); return DCREG_E_INVALID; }
    return DCREG_OK;
}
int fpfh_check(dcreg_ctx *c, const FpfhRule &r) { return r.radius ? fpfh_radius_check(c, r.rp) : fpfh_check(c, r.p); }

template <int K>
void launch_spfh(dcreg_ctx *c, const float4 *q, int64_t nq, const GridDev &g, float bound, int max_ring, int k, const float *nrm, int64_t nstride) {
    dcreg_ctx::FeatureBufs &F = c->feat;
    hipLaunchKernelGGL(k_fpfh_spfh<K>, dim3(blocks(nq, kBlock)), dim3(kBlock), 0, c->stream, q, (uint32_t)nq, g, bound, max_ring, k, nrm, nstride,
                       F.nb_pos.data(), F.nb_d2.data(), F.spfh.data());
}

// The outputs of n points start as NaN; the nq used points at q (cell order, w = the output index) behind the grid g get theirs from the
// normals at nrm (by input index); then the copy to the caller and the counts.  nq = 0: no used point.  The queries ARE the grid's points:
// a neighbour's position in the sorted array is also its lane in both kernels, which is how k_fpfh_sum finds its counts
int fpfh_run(dcreg_ctx *c, int64_t nq, const GridDev &g, int64_t n, const float *nrm, int64_t nstride, const dcreg_fpfh_params *p,
             float *out, bool on_device, dcreg_fpfh_info *info) {
    dcreg_ctx::FeatureBufs &F = c->feat;
    const size_t k = (size_t)p->k, nqs = (size_t)std::max<int64_t>(nq, 1);
    if (F.out.ensure(c, (size_t)kDim * (size_t)n) || F.cnt.ensure(c, 3) || F.nb_pos.ensure(c, k * nqs) || F.nb_d2.ensure(c, k * nqs) ||
        F.spfh.ensure(c, 3 * nqs))
        return DCREG_E_NOMEM;
    fill_f32(c, F.out.data(), (int64_t)kDim * n, __builtin_nanf(""));
    HIP_TRY(c, hipMemsetAsync(F.cnt.data(), 0, 2 * sizeof(unsigned long long), c->stream));
    unsigned long long cnt[2] = {0, 0};
    F.last_q = nq > 0 ? g.pts : nullptr; F.last_nq = nq; F.last_n = n;      // (dcreg_fpfh_debug_counts)
    F.rlast_n = 0; F.last_epoch = c->index_epoch;
    if (nq > 0) {
        const float4 *q = g.pts;
        const SearchBound s = search_bound(p->search_radius, &g);
        with_heap_k(p->k, [&](auto K) { launch_spfh<decltype(K)::value>(c, q, nq, g, s.bound, s.max_ring, p->k, nrm, nstride); });
        hipLaunchKernelGGL(k_fpfh_sum, dim3(blocks(nq, kBlock)), dim3(kBlock), 0, c->stream, q, (uint32_t)nq, p->k, F.nb_pos.data(), F.nb_d2.data(),
                           F.spfh.data(), F.out.data(), F.cnt.data());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(cnt, F.cnt.data(), sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    }
    if (int rc = caller_out(c, out, F.out.data(), sizeof(float) * (size_t)kDim * (size_t)n, on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (info) { info->n_in = n; info->n_used = nq; info->n_empty = (int64_t)cnt[1]; info->n_out = (int64_t)cnt[0]; }
    return DCREG_OK;
}

// fpfh_run under the radius rule: pass 1, pass 2, the statistics
int fpfh_radius_run(dcreg_ctx *c, int64_t nq, const GridDev &g, int64_t n, const float *nrm, int64_t nstride, const dcreg_fpfh_radius_params *p,
                    float *out, bool on_device, dcreg_fpfh_radius_info *info) {
    dcreg_ctx::FeatureBufs &F = c->feat;
    const size_t nqs = (size_t)std::max<int64_t>(nq, 1);
    if (F.out.ensure(c, (size_t)kDim * (size_t)n) || F.cnt.ensure(c, 4) || F.rrec.ensure(c, 9 * nqs) || F.rcounts.ensure(c, (size_t)kDim * nqs))
        return DCREG_E_NOMEM;
    fill_f32(c, F.out.data(), (int64_t)kDim * n, __builtin_nanf(""));
    HIP_TRY(c, hipMemsetAsync(F.cnt.data(), 0, 4 * sizeof(unsigned long long), c->stream));
    unsigned long long cnt[4] = {0, 0, 0, 0};
    F.rlast_q = nq > 0 ? g.pts : nullptr; F.rlast_nq = nq; F.rlast_n = n;      // (dcreg_fpfh_radius_debug_counts)
    F.last_n = 0; F.last_epoch = c->index_epoch;
    if (nq > 0) {
        const float4 *q = g.pts;
        const float R2 = (float)(p->radius * p->radius);
        const uint32_t cap = (uint32_t)p->max_neighbors;
        hipLaunchKernelGGL(k_fpfh_rspfh, dim3(blocks(nq, kTeams)), dim3(kBlock), 0, c->stream, q, (uint32_t)nq, g, R2, cap, nrm, nstride,
                           (uint32_t *)F.rrec.data(), F.rcounts.data());
        hipLaunchKernelGGL(k_fpfh_rsum, dim3(blocks(nq, kTeams)), dim3(kBlock), 0, c->stream, q, (uint32_t)nq, g, R2, cap, (const uint4 *)F.rrec.data(),
                           F.out.data());
        hipLaunchKernelGGL(k_fpfh_rstats, dim3(blocks(nq, 256)), dim3(256), 0, c->stream, q, (uint32_t)nq, cap, (const uint32_t *)F.rrec.data(),
                           (const float *)F.out.data(), F.cnt.data());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(cnt, F.cnt.data(), sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    }
    if (int rc = caller_out(c, out, F.out.data(), sizeof(float) * (size_t)kDim * (size_t)n, on_device)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (info) {
        info->n_in = n; info->n_used = nq; info->n_out = (int64_t)cnt[0]; info->n_empty = nq - (int64_t)cnt[0]; info->n_crowded = (int64_t)cnt[1];
        info->m_max = (int64_t)cnt[2]; info->m_sum = (int64_t)cnt[3];
    }
    return DCREG_OK;
}

int fpfh_run(dcreg_ctx *c, int64_t nq, const GridDev &g, int64_t n, const float *nrm, int64_t nstride, const FpfhRule &r, float *out, bool on_device) {
    return r.radius ? fpfh_radius_run(c, nq, g, n, nrm, nstride, r.rp, out, on_device, r.rinfo) : fpfh_run(c, nq, g, n, nrm, nstride, r.p, out, on_device, r.info);
}

// the n packed points at pts lose those without a finite normal, the rest is compacted and indexed in the cloud scratch
int fpfh_index(dcreg_ctx *c, float4 *pts, int64_t n, const float *nrm, int64_t nstride, double hint, int64_t *n_used) {
    hipLaunchKernelGGL(k_fpfh_unuse, dim3(blocks(n, 256)), dim3(256), 0, c->stream, pts, n, nrm, nstride);
    HIP_TRY(c, hipGetLastError());
    return cloud_index_used(c, pts, n, hint, 1, n_used);
}

// dcreg_fpfh*: the cloud packed, the normals given or estimated, the used points indexed, the two kernels, the copies
int fpfh_cloud(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const float *normals, int64_t nstride, bool on_device,
               const dcreg_normal_params *np, const FpfhRule &rule, float *out, float *normals_out) {
    if (!c) return DCREG_E_INVALID;
    rule.clear_info();                  // (a refused call leaves the info zero, whatever it held)
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = fpfh_check(c, rule)) return rc;
    if (!normals && !np) { c->fail("no normals and no normal parameters: one of them is expected"); return DCREG_E_INVALID; }
    if (!normals) if (int rc = normals_check(c, np)) return rc;
    if (n < 0 || stride < 3 || (normals && nstride < 3)) { c->fail("invalid fpfh arguments"); return DCREG_E_INVALID; }
    if (n > (int64_t)INT32_MAX) { c->fail("too many points for one descriptor call (%lld)", (long long)n); return DCREG_E_INVALID; }
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (n == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::CloudScratch &B = c->cloud;
    if (int rc = upload_cloud(c, xyz, n, stride, on_device, B.pts)) return rc;
    const double hint = rule.hint();
    int64_t n_used = 0;
    const float *nrm = normals;
    if (normals) {
        // (staged beside the cloud, which upload_cloud has just left in c->d_stage; device normals: upload_cloud has ordered the call)
        if (int rc = caller_rows(c, normals, n, nstride, 3, on_device, c->feat.nrm_in, &nrm, true)) return rc;
        if (int rc = fpfh_index(c, B.pts.data(), n, nrm, nstride, hint, &n_used)) return rc;
    } else {
        int64_t n_finite = 0;
        if (int rc = cloud_index_used(c, B.pts.data(), n, hint, 1, &n_finite)) return rc;
        dcreg_normal_info ni{};
        const bool indexed = n_finite >= np->k;            // (fewer: every point is sparse, as dcreg_normals says it)
        if (int rc = normals_to_scratch(c, indexed ? B.idx.sorted.data() : nullptr, indexed ? n_finite : 0, indexed ? B.idx.grid : GridDev{}, n, n_finite, np, &ni))
            return rc;
        nrm = c->nrm.normal.data();
        nstride = 3;
        if (normals_out)
            if (int rc = caller_out(c, normals_out, nrm, sizeof(float) * 3 * (size_t)n, on_device)) return rc;
        n_used = n_finite;
        // (a finite point without a normal is not used: the index over the finite points serves only when every one of them has one)
        if (ni.n_out != n_finite) if (int rc = fpfh_index(c, B.pts.data(), n, nrm, nstride, hint, &n_used)) return rc;
    }
    return fpfh_run(c, n_used, n_used > 0 ? B.idx.grid : GridDev{}, n, nrm, nstride, rule, out, on_device);
}

// dcreg_target_fpfh*: the whole map's points through the map's own index and its kept normals
int fpfh_map(dcreg_ctx *c, bool on_device, const FpfhRule &rule, float *out, int64_t capacity) {
    if (!c) return DCREG_E_INVALID;
    rule.clear_info();                  // (as the cloud form: zero behind every refusal)
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = fpfh_check(c, rule)) return rc;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    if (!c->nicp.kept) { c->fail("no kept normals: dcreg_target_normals_keep or dcreg_target_normals_set first"); return DCREG_E_STATE; }
    const dcreg_ctx::IndexSet &wm = c->roi_active ? c->roi_store : c->map;      // the whole map's index, whichever is active
    const int64_t n = wm.n;
    if (capacity < n) { c->fail("the map holds %lld points, the capacity is %lld", (long long)n, (long long)capacity); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::FeatureBufs &F = c->feat;
    if (F.cnt.ensure(c, 3)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(F.cnt.data() + 2, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_fpfh_bad, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->nicp.normals.data(), n, F.cnt.data());
    HIP_TRY(c, hipGetLastError());
    unsigned long long bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, F.cnt.data() + 2, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const float *nrm = (const float *)c->nicp.normals.data();
    if (bad == 0) return fpfh_run(c, n, wm.grid, n, nrm, 4, rule, out, on_device);
    // some map points have no normal: they are no candidates, so the others are indexed on their own, as a cloud's
    dcreg_ctx::CloudScratch &B = c->cloud;
    if (B.pts.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemcpyAsync(B.pts.data(), wm.raw.data(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    int64_t n_used = 0;
    if (int rc = fpfh_index(c, B.pts.data(), n, nrm, 4, rule.hint(), &n_used)) return rc;
    return fpfh_run(c, n_used, n_used > 0 ? B.idx.grid : GridDev{}, n, nrm, 4, rule, out, on_device);
}

// The reports read the sorted points of the index their call searched (last_q / rlast_q: the cloud scratch index or the map's own).  An
// index built since, an update of the map or a change of its active index (dcreg_ctx::index_epoch) leaves other points there, with input
// indices the export was not sized for: refused on the host, before anything is queued
int fpfh_report_stale(dcreg_ctx *c) {
    if (c->feat.last_epoch == c->index_epoch) return DCREG_OK;
    c->fail("the descriptor call's index has been rebuilt or its map changed since: the report is only valid directly behind that call");
    return DCREG_E_STATE;
}

// dcreg_fpfh_debug_counts (include/dcreg_debug.h)
int fpfh_debug_counts(dcreg_ctx *c, uint8_t *out, int64_t capacity) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    dcreg_ctx::FeatureBufs &F = c->feat;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (F.last_n <= 0) { c->fail("no descriptor call to report"); return DCREG_E_STATE; }
    if (int rc = fpfh_report_stale(c)) return rc;
    if (capacity < F.last_n) { c->fail("the call had %lld points, the capacity is %lld", (long long)F.last_n, (long long)capacity); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t words = (size_t)kCountWords * (size_t)F.last_n;
    if (F.dbg.ensure(c, words)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(F.dbg.data(), 0, sizeof(uint32_t) * words, c->stream));
    if (F.last_nq > 0)
        hipLaunchKernelGGL(k_fpfh_counts, dim3(blocks(F.last_nq, 256)), dim3(256), 0, c->stream, F.last_q, (uint32_t)F.last_nq, F.spfh.data(), F.dbg.data());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, F.dbg.data(), sizeof(uint32_t) * words, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

// dcreg_fpfh_radius_debug_counts (include/dcreg_debug.h)
int fpfh_radius_debug_counts(dcreg_ctx *c, uint32_t *out, int64_t capacity) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    dcreg_ctx::FeatureBufs &F = c->feat;
    if (!out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (F.rlast_n <= 0) { c->fail("no radius descriptor call to report"); return DCREG_E_STATE; }
    if (int rc = fpfh_report_stale(c)) return rc;
    if (capacity < F.rlast_n) { c->fail("the call had %lld points, the capacity is %lld", (long long)F.rlast_n, (long long)capacity); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t words = (size_t)(kDim + 2) * (size_t)F.rlast_n;
    if (F.dbg.ensure(c, words)) return DCREG_E_NOMEM;
    HIP_TRY(c, hipMemsetAsync(F.dbg.data(), 0, sizeof(uint32_t) * words, c->stream));
    if (F.rlast_nq > 0)
        hipLaunchKernelGGL(k_fpfh_rcounts, dim3(blocks(F.rlast_nq, 256)), dim3(256), 0, c->stream, F.rlast_q, (uint32_t)F.rlast_nq,
                           (const uint32_t *)F.rrec.data(), (const uint32_t *)F.rcounts.data(), F.dbg.data());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, F.dbg.data(), sizeof(uint32_t) * words, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

// ------------------------------------------------------------------------------------------ matching: the host side
// one direction: the best two rows of y for every row of x, through the partial winners; the outputs (device, may be null) are queued
int match_pass(dcreg_ctx *c, const float *x, int64_t n_x, int64_t stride_x, const uint8_t *ok_x, const float *y, int64_t n_y, int64_t stride_y,
               const uint8_t *ok_y, int32_t *idx, double *dist, int32_t *idx2, double *dist2) {
    dcreg_ctx::FeatureBufs &F = c->feat;
    const int64_t blocks_x = (n_x + kMatchBlock - 1) / kMatchBlock;
    int64_t chunk = c->opt_feature_match_split, n_split = 0;
    if (n_y > 0) {
        if (chunk <= 0) {                                   // about a thousand blocks, a split no shorter than a tile
            const int64_t want = std::max<int64_t>(1, 1024 / blocks_x), tiles = (n_y + kMatchTile - 1) / kMatchTile;
            chunk = (tiles + std::min(want, tiles) - 1) / std::min(want, tiles) * kMatchTile;
        }
        chunk = std::max<int64_t>(chunk, (n_y + 65534) / 65535);          // (blockIdx.y)
        n_split = (n_y + chunk - 1) / chunk;
    }
    const size_t parts = 2 * (size_t)std::max<int64_t>(n_split, 1) * (size_t)n_x;
    if (F.part_d.ensure(c, parts) || F.part_i.ensure(c, parts)) return DCREG_E_NOMEM;
    if (n_split > 0)
        hipLaunchKernelGGL(k_match, dim3((unsigned)blocks_x, (unsigned)n_split), dim3(kMatchBlock), 0, c->stream, x, (uint32_t)n_x, stride_x, y, (uint32_t)n_y,
                           stride_y, ok_y, (uint32_t)chunk, F.part_d.data(), F.part_i.data());
    hipLaunchKernelGGL(k_match_merge, dim3(blocks(n_x, 256)), dim3(256), 0, c->stream, (uint32_t)n_x, (uint32_t)n_split, F.part_d.data(), F.part_i.data(), ok_x,
                       idx, dist, idx2, dist2);
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

int feature_match(dcreg_ctx *c, const float *a, int64_t n_a, int64_t stride_a, const float *b, int64_t n_b, int64_t stride_b, bool on_device,
                  int32_t *idx_out, double *d_out, int32_t *idx2_out, double *d2nd_out, uint8_t *mutual_out, dcreg_match_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (n_a < 0 || n_b < 0 || stride_a < kDim || stride_b < kDim) { c->fail("invalid feature matching arguments"); return DCREG_E_INVALID; }
    if (n_a > (int64_t)INT32_MAX || n_b > (int64_t)INT32_MAX) { c->fail("too many rows for one feature matching call"); return DCREG_E_INVALID; }
    if ((n_a > 0 && !a) || (n_b > 0 && !b)) { c->fail("null descriptor buffer"); return DCREG_E_INVALID; }
    if (!idx_out || !d_out) { c->fail("null output buffer"); return DCREG_E_INVALID; }
    if (info) std::memset(info, 0, sizeof(*info));
    if (n_a == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    dcreg_ctx::FeatureBufs &F = c->feat;
    const size_t na = (size_t)n_a, nb = (size_t)std::max<int64_t>(n_b, 1);
    if (F.va.ensure(c, na) || F.vb.ensure(c, nb) || F.cnt.ensure(c, 3) || F.idx.ensure(c, na) || F.d1.ensure(c, na) || F.idx2.ensure(c, na) ||
        F.d2.ensure(c, na) || (mutual_out && (F.mutual.ensure(c, na) || F.idx_b.ensure(c, nb))))
        return DCREG_E_NOMEM;
    const float *da = nullptr, *db = nullptr;
    if (int rc = caller_rows(c, a, n_a, stride_a, kDim, on_device, F.a, &da)) return rc;
    if (int rc = caller_rows(c, b, n_b, stride_b, kDim, on_device, F.b, &db, true)) return rc;
    HIP_TRY(c, hipMemsetAsync(F.cnt.data(), 0, 3 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_match_valid, dim3(blocks(n_a, 256)), dim3(256), 0, c->stream, da, n_a, stride_a, F.va.data(), F.cnt.data());
    if (n_b > 0) hipLaunchKernelGGL(k_match_valid, dim3(blocks(n_b, 256)), dim3(256), 0, c->stream, db, n_b, stride_b, F.vb.data(), F.cnt.data() + 1);
    if (int rc = match_pass(c, da, n_a, stride_a, F.va.data(), db, n_b, stride_b, F.vb.data(), F.idx.data(), F.d1.data(), F.idx2.data(), F.d2.data())) return rc;
    if (mutual_out) {
        if (n_b > 0)
            if (int rc = match_pass(c, db, n_b, stride_b, F.vb.data(), da, n_a, stride_a, F.va.data(), F.idx_b.data(), nullptr, nullptr, nullptr)) return rc;
        hipLaunchKernelGGL(k_match_mutual, dim3(blocks(n_a, 256)), dim3(256), 0, c->stream, (uint32_t)n_a, F.idx.data(), F.idx_b.data(), F.mutual.data(), F.cnt.data());
        HIP_TRY(c, hipGetLastError());
    }
    unsigned long long cnt[3] = {0, 0, 0};
    if (int rc = caller_out(c, idx_out, F.idx.data(), sizeof(int32_t) * na, on_device)) return rc;
    if (int rc = caller_out(c, d_out, F.d1.data(), sizeof(double) * na, on_device)) return rc;
    if (idx2_out) if (int rc = caller_out(c, idx2_out, F.idx2.data(), sizeof(int32_t) * na, on_device)) return rc;
    if (d2nd_out) if (int rc = caller_out(c, d2nd_out, F.d2.data(), sizeof(double) * na, on_device)) return rc;
    if (mutual_out) if (int rc = caller_out(c, mutual_out, F.mutual.data(), na, on_device)) return rc;
    HIP_TRY(c, hipMemcpyAsync(cnt, F.cnt.data(), sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (info) { info->n_a_valid = (int64_t)cnt[0]; info->n_b_valid = (int64_t)cnt[1]; info->n_mutual = (int64_t)cnt[2]; }
    return DCREG_OK;
}

}  // namespace
}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_default_fpfh_params(dcreg_fpfh_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->k = 16; p->search_radius = 0.0;
    return DCREG_OK;
}
int dcreg_fpfh(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride_floats, const float *normals, int64_t normals_stride_floats,
               const dcreg_normal_params *np, const dcreg_fpfh_params *p, float *fpfh_out, float *normals_out, dcreg_fpfh_info *info) {
    FpfhRule r; r.p = p; r.info = info;
    return fpfh_cloud(c, xyz, n, stride_floats, normals, normals_stride_floats, false, np, r, fpfh_out, normals_out);
}
int dcreg_fpfh_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride_floats, const float *d_normals, int64_t normals_stride_floats,
                      const dcreg_normal_params *np, const dcreg_fpfh_params *p, float *d_fpfh_out, float *d_normals_out, dcreg_fpfh_info *info) {
    FpfhRule r; r.p = p; r.info = info;
    return fpfh_cloud(c, d_xyz, n, stride_floats, d_normals, normals_stride_floats, true, np, r, d_fpfh_out, d_normals_out);
}
int dcreg_target_fpfh(dcreg_ctx *c, const dcreg_fpfh_params *p, float *fpfh_out, int64_t capacity_points, dcreg_fpfh_info *info) {
    FpfhRule r; r.p = p; r.info = info;
    return fpfh_map(c, false, r, fpfh_out, capacity_points);
}
int dcreg_target_fpfh_device(dcreg_ctx *c, const dcreg_fpfh_params *p, float *d_fpfh_out, int64_t capacity_points, dcreg_fpfh_info *info) {
    FpfhRule r; r.p = p; r.info = info;
    return fpfh_map(c, true, r, d_fpfh_out, capacity_points);
}
int dcreg_fpfh_debug_counts(dcreg_ctx *c, uint8_t *counts_out, int64_t capacity_points) { return fpfh_debug_counts(c, counts_out, capacity_points); }
int dcreg_default_fpfh_radius_params(dcreg_fpfh_radius_params *p) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->radius = 1.0; p->max_neighbors = 65535;
    return DCREG_OK;
}
static FpfhRule radius_rule(const dcreg_fpfh_radius_params *p, dcreg_fpfh_radius_info *info) {
    FpfhRule r; r.rp = p; r.rinfo = info; r.radius = true;
    return r;
}
int dcreg_fpfh_radius(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride_floats, const float *normals, int64_t normals_stride_floats,
                      const dcreg_normal_params *np, const dcreg_fpfh_radius_params *p, float *fpfh_out, float *normals_out, dcreg_fpfh_radius_info *info) {
    return fpfh_cloud(c, xyz, n, stride_floats, normals, normals_stride_floats, false, np, radius_rule(p, info), fpfh_out, normals_out);
}
int dcreg_fpfh_radius_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride_floats, const float *d_normals, int64_t normals_stride_floats,
                             const dcreg_normal_params *np, const dcreg_fpfh_radius_params *p, float *d_fpfh_out, float *d_normals_out,
                             dcreg_fpfh_radius_info *info) {
    return fpfh_cloud(c, d_xyz, n, stride_floats, d_normals, normals_stride_floats, true, np, radius_rule(p, info), d_fpfh_out, d_normals_out);
}
int dcreg_target_fpfh_radius(dcreg_ctx *c, const dcreg_fpfh_radius_params *p, float *fpfh_out, int64_t capacity_points, dcreg_fpfh_radius_info *info) {
    return fpfh_map(c, false, radius_rule(p, info), fpfh_out, capacity_points);
}
int dcreg_target_fpfh_radius_device(dcreg_ctx *c, const dcreg_fpfh_radius_params *p, float *d_fpfh_out, int64_t capacity_points,
                                    dcreg_fpfh_radius_info *info) {
    return fpfh_map(c, true, radius_rule(p, info), d_fpfh_out, capacity_points);
}
int dcreg_fpfh_radius_debug_counts(dcreg_ctx *c, uint32_t *counts_out, int64_t capacity_points) { return fpfh_radius_debug_counts(c, counts_out, capacity_points); }
int dcreg_feature_match(dcreg_ctx *c, const float *a, int64_t n_a, int64_t stride_a, const float *b, int64_t n_b, int64_t stride_b, int32_t *idx_out,
                        double *d_out, int32_t *idx2_out, double *d2nd_out, uint8_t *mutual_out, dcreg_match_info *info) {
    return feature_match(c, a, n_a, stride_a, b, n_b, stride_b, false, idx_out, d_out, idx2_out, d2nd_out, mutual_out, info);
}
int dcreg_feature_match_device(dcreg_ctx *c, const float *d_a, int64_t n_a, int64_t stride_a, const float *d_b, int64_t n_b, int64_t stride_b,
                               int32_t *d_idx_out, double *d_d_out, int32_t *d_idx2_out, double *d_d2nd_out, uint8_t *d_mutual_out,
                               dcreg_match_info *info) {
    return feature_match(c, d_a, n_a, stride_a, d_b, n_b, stride_b, true, d_idx_out, d_d_out, d_idx2_out, d_d2nd_out, d_mutual_out, info);
}
}
