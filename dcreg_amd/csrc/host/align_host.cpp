// The host side of dcreg_align_correspondences (include/dcreg.h, "pose from correspondences", steps 6 and 7): the records of the few
// best hypotheses from the compacted used pairs - their draws and pose once more (device/align.hpp: bitwise what the device scored), the
// least-squares refinement over the inliers with Horn's quaternion through a cyclic Jacobi, n_inliers, rmse and the mask of the first
// record.  Everything is summed left to right as the header writes it; the records are independent, so OpenMP runs over them.
// dcreg_consensus_correspondences (device/consensus.hip) takes the same fit for its sets' poses and the same refinement for its records.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../device/align.hpp"

// every multiply and add below rounds once: the rule is stated operation by operation
#pragma clang fp contract(off)

namespace dcreg {
namespace {

// one rotation of the pair (p, q) of the symmetric 4x4 matrix a with the eigenvector columns v: jacobi_rot's formulas (device/jacobi.hpp)
// for t, c and s, the two remaining rows and the four rows of v
void jacobi4_rot(double a[4][4], double v[4][4], int p, int q) {
    const double apq = a[p][q];
    double t = 0.0;
    if (apq != 0.0) {
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    }
    const double c = 1.0 / std::sqrt(t * t + 1.0);
    const double s = t * c;
    const double tp = t * apq;
    a[p][p] = a[p][p] - tp;
    a[q][q] = a[q][q] + tp;
    a[p][q] = a[q][p] = 0.0;
    for (int r = 0; r < 4; ++r) {
        if (r == p || r == q) continue;
        const double rp = a[r][p], rq = a[r][q];
        a[r][p] = a[p][r] = c * rp - s * rq;
        a[r][q] = a[q][r] = s * rp + c * rq;
    }
    for (int k = 0; k < 4; ++k) {
        const double x = v[k][p], y = v[k][q];
        v[k][p] = c * x - s * y;
        v[k][q] = s * x + c * y;
    }
}

}  // namespace

void align_host_fit(const float *P, const uint32_t *idx, size_t n_idx, double R[9], double t[3]) {
    const double n = (double)n_idx;
    double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < n_idx; ++i) {
        const uint32_t u = idx[i];
        const float *r = P + (size_t)kAlignPairFloats * u;
        for (int c = 0; c < 3; ++c) { cp[c] = cp[c] + (double)r[c]; cq[c] = cq[c] + (double)r[3 + c]; }
    }
    for (int c = 0; c < 3; ++c) { cp[c] = cp[c] / n; cq[c] = cq[c] / n; }
    double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (size_t i = 0; i < n_idx; ++i) {
        const uint32_t u = idx[i];
        const float *r = P + (size_t)kAlignPairFloats * u;
        double dp[3], dq[3];
        for (int c = 0; c < 3; ++c) { dp[c] = (double)r[c] - cp[c]; dq[c] = (double)r[3 + c] - cq[c]; }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[a][b] = S[a][b] + dp[a] * dq[b];
    }
    double N[4][4], V[4][4];
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    N[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    N[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    N[0][1] = N[1][0] = S[1][2] - S[2][1];
    N[0][2] = N[2][0] = S[2][0] - S[0][2];
    N[0][3] = N[3][0] = S[0][1] - S[1][0];
    N[1][2] = N[2][1] = S[0][1] + S[1][0];
    N[1][3] = N[3][1] = S[2][0] + S[0][2];
    N[2][3] = N[3][2] = S[1][2] + S[2][1];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 8; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) jacobi4_rot(N, V, p, q);
    int best = 0;
    for (int k = 1; k < 4; ++k) if (N[k][k] > N[best][best]) best = k;
    double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double nq = std::sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nq; x = x / nq; y = y / nq; z = z / nq;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz); R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz); R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy); R[7] = 2.0 * (yz + wx); R[8] = 1.0 - 2.0 * (xx + yy);
    for (int r = 0; r < 3; ++r) t[r] = cq[r] - ((R[3 * r] * cp[0] + R[3 * r + 1] * cp[1]) + R[3 * r + 2] * cp[2]);
}

namespace {

// one refinement step over the inliers of (R, t) in ascending u; false: fewer than three inliers, the pose stays
bool refine_step(const float *P, int64_t m_u, double dd, double R[9], double t[3], std::vector<uint32_t> &in) {
    in.clear();
    for (int64_t u = 0; u < m_u; ++u) {
        const float *r = P + kAlignPairFloats * u;
        if (align_e2(R, t, r[0], r[1], r[2], r[3], r[4], r[5]) <= dd) in.push_back((uint32_t)u);
    }
    if (in.size() < 3) return false;
    align_host_fit(P, in.data(), in.size(), R, t);
    return true;
}

// what both calls do with a record's pose: the refinement steps, then n_inliers, rmse and T of the final pose, and the mask if it is record 0's
template <typename Record>
void finish_record(const float *P, const int32_t *m_of_u, int64_t m_u, double dd, int refine_iterations, double R[9], double t[3], Record &o, uint8_t *mask) {
    std::vector<uint32_t> in;
    for (int it = 0; it < refine_iterations; ++it) {
        if (!refine_step(P, m_u, dd, R, t, in)) break;
        o.refined += 1;
    }
    int64_t n_in = 0;
    double sum = 0.0;
    for (int64_t i = 0; i < m_u; ++i) {
        const float *r = P + kAlignPairFloats * i;
        const double e2 = align_e2(R, t, r[0], r[1], r[2], r[3], r[4], r[5]);
        if (e2 <= dd) {
            n_in += 1;
            sum = sum + e2;
            if (mask) mask[m_of_u[i]] = 1;
        }
    }
    o.n_inliers = (int32_t)n_in;
    o.rmse = n_in > 0 ? std::sqrt(sum / (double)n_in) : 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.T[4 * r + c] = R[3 * r + c];
        o.T[4 * r + 3] = t[r];
    }
    o.T[15] = 1.0;
}

}  // namespace

void align_host_records(const float *P, const int32_t *m_of_u, int64_t m_u, int64_t n_pairs, const dcreg_align_params *prm, const AlignKey *keys,
                        int n_rec, dcreg_align_record *rec, uint8_t *mask) {
    if (mask && n_pairs > 0) std::memset(mask, 0, (size_t)n_pairs);
    const double dd = prm->inlier_distance * prm->inlier_distance;
#pragma omp parallel for schedule(dynamic) num_threads(std::max(1, std::min(n_rec, omp_get_max_threads())))
    for (int k = 0; k < n_rec; ++k) {
        dcreg_align_record &o = rec[k];
        std::memset(&o, 0, sizeof(o));
        uint32_t u[3];
        double R[9], t[3];
        (void)align_hypothesis(P, (uint32_t)m_u, prm->seed, keys[k].h, 0.0, u, R, t);      // (a survivor: kAlignOk)
        o.hypothesis = (int64_t)keys[k].h;
        for (int j = 0; j < 3; ++j) o.pairs[j] = m_of_u[u[j]];
        o.count = (int32_t)keys[k].count;
        o.cost = (uint64_t)keys[k].cost;
        finish_record(P, m_of_u, m_u, dd, prm->refine_iterations, R, t, o, k == 0 ? mask : nullptr);
    }
}

void consensus_host_fit(const float *P, const uint32_t *mem, const uint32_t *n_mem, const uint32_t *set, int n, double *pose) {
#pragma omp parallel for schedule(dynamic) num_threads(std::max(1, std::min(n, omp_get_max_threads())))
    for (int i = 0; i < n; ++i) align_host_fit(P, mem + (size_t)kConsMaxSet * set[i], n_mem[set[i]], pose + 12 * (size_t)i, pose + 12 * (size_t)i + 9);
}

void consensus_host_records(const float *P, const int32_t *m_of_u, int64_t m_u, int64_t n_pairs, const dcreg_consensus_params *prm, const AlignKey *keys,
                            int n_rec, const double *pose, const uint32_t *set, const uint32_t *seed_u, const uint32_t *seed_w, const uint32_t *mem,
                            const uint32_t *n_mem, dcreg_consensus_record *rec, uint8_t *mask, int32_t *members) {
    if (mask && n_pairs > 0) std::memset(mask, 0, (size_t)n_pairs);
    if (members) std::fill(members, members + (size_t)prm->n_best * (size_t)prm->consensus_size, (int32_t)-1);
    const double dd = prm->inlier_distance * prm->inlier_distance;
#pragma omp parallel for schedule(dynamic) num_threads(std::max(1, std::min(n_rec, omp_get_max_threads())))
    for (int k = 0; k < n_rec; ++k) {
        dcreg_consensus_record &o = rec[k];
        std::memset(&o, 0, sizeof(o));
        const uint32_t i = keys[k].h, r = set[i];
        double R[9], t[3];
        for (int j = 0; j < 9; ++j) R[j] = pose[12 * (size_t)i + j];
        for (int j = 0; j < 3; ++j) t[j] = pose[12 * (size_t)i + 9 + j];
        o.seed = m_of_u[seed_u[r]];
        o.seed_rank = (int32_t)r;
        o.weight = (int32_t)seed_w[r];
        o.n_members = (int32_t)n_mem[r];
        o.count = (int32_t)keys[k].count;
        o.cost = (uint64_t)keys[k].cost;
        if (members)
            for (uint32_t j = 0; j < n_mem[r]; ++j) members[(size_t)k * (size_t)prm->consensus_size + j] = m_of_u[mem[(size_t)kConsMaxSet * r + j]];
        finish_record(P, m_of_u, m_u, dd, prm->refine_iterations, R, t, o, k == 0 ? mask : nullptr);
    }
}

}  // namespace dcreg
