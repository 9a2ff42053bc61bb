// The part of the alignment rule (include/dcreg.h, "pose from correspondences") that the device and the host both run: the draws of a
// hypothesis and its pose from three pairs.  k_align_hypotheses decides with it which hypotheses survive, k_align_score computes the pose
// again from h alone (nothing but h is stored per survivor), and the host computes it a third time for the few records it returns
// (host/align_host.cpp).  Every operation is rounded once and none of them is a library function whose last bit is free, so the three
// agree bitwise.  Plain C++ but for the function attribute: the host translation units include it too.
#pragma once
#include <cmath>
#include <cstdint>
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define DCREG_ALIGN_FN __host__ __device__ inline
#else
#define DCREG_ALIGN_FN inline
#endif

#include "../../../include/dcreg.h"

namespace dcreg {

constexpr int kAlignPairFloats = 6;          // a used pair: p (x, y, z), then q

// splitmix64: x(k) = mix(seed + k * 0x9E3779B97F4A7C15)
DCREG_ALIGN_FN uint64_t align_x(uint64_t seed, uint64_t k) {
    uint64_t z = seed + k * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the three used pairs of hypothesis h among m_u
DCREG_ALIGN_FN void align_draw(uint64_t seed, uint64_t h, uint32_t m_u, uint32_t u[3]) {
    for (int j = 0; j < 3; ++j) u[j] = (uint32_t)(((align_x(seed, 3ull * h + (uint64_t)j + 1ull) >> 32) * (uint64_t)m_u) >> 32);
}

// e1, e2, e3 of the triad over (a0, a1, a2); false: degenerate
DCREG_ALIGN_FN bool align_triad(const double a0[3], const double a1[3], const double a2[3], double e[3][3]) {
#pragma clang fp contract(off)
    const double ux = a1[0] - a0[0], uy = a1[1] - a0[1], uz = a1[2] - a0[2];
    const double vx = a2[0] - a0[0], vy = a2[1] - a0[1], vz = a2[2] - a0[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double uu = (ux * ux + uy * uy) + uz * uz, vv = (vx * vx + vy * vy) + vz * vz, ww = (wx * wx + wy * wy) + wz * wz;
    if (ww <= 1e-4 * (uu * vv)) return false;
    const double nu = sqrt(uu), nw = sqrt(ww);
    e[0][0] = ux / nu; e[0][1] = uy / nu; e[0][2] = uz / nu;
    e[2][0] = wx / nw; e[2][1] = wy / nw; e[2][2] = wz / nw;
    e[1][0] = e[2][1] * e[0][2] - e[2][2] * e[0][1];
    e[1][1] = e[2][2] * e[0][0] - e[2][0] * e[0][2];
    e[1][2] = e[2][0] * e[0][1] - e[2][1] * e[0][0];
    return true;
}

DCREG_ALIGN_FN double align_edge(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrt((x * x + y * y) + z * z);
}

enum { kAlignOk = 0, kAlignDegenerate = 1, kAlignRejected = 2 };

// Steps 2 to 4 for hypothesis h over the used pairs P ([u] -> p, q): its draws in u, and for kAlignOk its pose q ~ R p + t (R row-major).
// s: edge_similarity (0: no pre-rejection - also how the scorer and the host skip a test the hypothesis has passed already)
DCREG_ALIGN_FN int align_hypothesis(const float *P, uint32_t m_u, uint64_t seed, uint64_t h, double s, uint32_t u[3], double R[9], double t[3]) {
#pragma clang fp contract(off)
    align_draw(seed, h, m_u, u);
    if (u[0] == u[1] || u[1] == u[2] || u[2] == u[0]) return kAlignDegenerate;
    double p[3][3], q[3][3];
    for (int j = 0; j < 3; ++j) {
        const float *r = P + (size_t)kAlignPairFloats * u[j];
        for (int c = 0; c < 3; ++c) { p[j][c] = (double)r[c]; q[j][c] = (double)r[3 + c]; }
    }
    if (s > 0.0) {
        bool keep = true;
        for (int j = 0; j < 3; ++j) {
            const int k = j == 2 ? 0 : j + 1;
            const double la = align_edge(p[j], p[k]), lb = align_edge(q[j], q[k]);
            keep = keep && la >= s * lb && lb >= s * la;
        }
        if (!keep) return kAlignRejected;
    }
    double e[3][3], f[3][3];
    const bool ok_p = align_triad(p[0], p[1], p[2], e), ok_q = align_triad(q[0], q[1], q[2], f);
    if (!(ok_p && ok_q)) return kAlignDegenerate;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (f[0][r] * e[0][c] + f[1][r] * e[1][c]) + f[2][r] * e[2][c];
    double cp[3], cq[3];
    for (int c = 0; c < 3; ++c) { cp[c] = ((p[0][c] + p[1][c]) + p[2][c]) / 3.0; cq[c] = ((q[0][c] + q[1][c]) + q[2][c]) / 3.0; }
    for (int r = 0; r < 3; ++r) t[r] = cq[r] - ((R[3 * r] * cp[0] + R[3 * r + 1] * cp[1]) + R[3 * r + 2] * cp[2]);
    return kAlignOk;
}

// the squared residual of the pair (p, q) under (R, t): r = ((R p) + t) - q, e2 = r.r
DCREG_ALIGN_FN double align_e2(const double R[9], const double t[3], double px, double py, double pz, double qx, double qy, double qz) {
#pragma clang fp contract(off)
    const double rx = (((R[0] * px + R[1] * py) + R[2] * pz) + t[0]) - qx;
    const double ry = (((R[3] * px + R[4] * py) + R[5] * pz) + t[1]) - qy;
    const double rz = (((R[6] * px + R[7] * py) + R[8] * pz) + t[2]) - qz;
    return (rx * rx + ry * ry) + rz * rz;
}

// one survivor: the ranking key (count descending, cost ascending, h ascending).  k_align_hypotheses writes h, k_align_score adds the rest
struct AlignKey {
    uint32_t count, h;
    unsigned long long cost;
};

// host/align_host.cpp: the records of the n_rec best survivors (keys, best first) from the m_u used pairs P and their correspondence
// numbers m_of_u - draws, pose, refinement, n_inliers and rmse, OpenMP over the records - and the mask of record 0 over the n_pairs
// correspondences (mask may be null; all zero when n_rec is 0)
void align_host_records(const float *P, const int32_t *m_of_u, int64_t m_u, int64_t n_pairs, const dcreg_align_params *prm, const AlignKey *keys,
                        int n_rec, dcreg_align_record *rec, uint8_t *mask);

// host/align_host.cpp: the least-squares fit of step 7 over the n used pairs idx (in the order given: ascending u) - centroids, S_ab,
// Horn's N, eight Jacobi sweeps, the quaternion, R and t.  The refinement calls it with the inliers, the consensus call with a set's members
void align_host_fit(const float *P, const uint32_t *idx, size_t n, double R[9], double t[3]);

// host/align_host.cpp, for the consensus call (device/consensus.hip).  One seed's set: its members as used-pair numbers in ascending u
constexpr int kConsMaxSet = 64, kConsMaxSeeds = 1024;
// the poses (R row-major, then t: 12 doubles) of the n sets whose member lists are mem[kConsMaxSet * set[i]] with n_mem[set[i]] entries
void consensus_host_fit(const float *P, const uint32_t *mem, const uint32_t *n_mem, const uint32_t *set, int n, double *pose);
// the records of the n_rec best sets: keys[k].h is the place i of the set among the scored ones (pose 12 i, rank set[i]); seed_u,
// seed_w: the seeds' used pair and weight by rank.  mask as align_host_records'; members (may be null): [n_best x consensus_size], -1 padded
void consensus_host_records(const float *P, const int32_t *m_of_u, int64_t m_u, int64_t n_pairs, const dcreg_consensus_params *prm, const AlignKey *keys,
                            int n_rec, const double *pose, const uint32_t *set, const uint32_t *seed_u, const uint32_t *seed_w, const uint32_t *mem,
                            const uint32_t *n_mem, dcreg_consensus_record *rec, uint8_t *mask, int32_t *members);

}  // namespace dcreg
