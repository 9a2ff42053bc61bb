// TEST INFRASTRUCTURE ONLY: host replay of the fourth engine's per-correspondence functions (dcreg_amd/csrc/device/voxel_icp.hpp:
// vlin_offset - the stencil - vmap_find_voxel - the lookup of a neighbour voxel through the open-addressing table - vlin_normal and
// vlin_corr - the covariance of one correspondence, its factor and W; gicp.hpp: glin_row, glin_row_scale), in the order the device's
// block body takes them (voxel_icp.hip vlin_block<DUMP, S>), in a library of its own (tests/emul_vlin_stencil.py).  The replay's own
// C-ABI (emul.cpp) comes along unchanged.
#include "emul.cpp"
#include "../../dcreg_amd/csrc/device/voxel_icp.hpp"

extern "C" {

// emu_vlin (emul_vlin.cpp) with S = 1, 7 or 27 correspondences per point: the same arguments, then S.  The dump arrays hold S entries
// per point, correspondence j of the point with original index oi at oi * S + j; normal_src is per point.  sums: the 31 sums added row by
// row in (processing order, j, k); slots 29 / 30 count points.
int emu_vlin_stencil(const float *recs, const int64_t *coords, int64_t n_vox, double leaf, const int64_t *box, const float *src,
                     const float *src_normals4, const uint32_t *order, int64_t n, const double *R, const double *t, int mode, double eps, int robust,
                     double robust_scale, int S, int32_t *voxel_idx, uint8_t *flag, double *mean, double *cov, double *normal_src, double *w, double *r,
                     double *row, double *sums) {
    if (!(S == 1 || S == 7 || S == 27)) return 1;
    size_t slots = 2;
    while (slots < 2 * (size_t)n_vox) slots <<= 1;
    std::vector<uint64_t> keys(slots, kVmapEmpty);
    std::vector<uint32_t> vals(slots, 0u);
    VoxMapDev vm;
    vm.recs = (const float4 *)recs; vm.keys = keys.data(); vm.vals = vals.data(); vm.mask = (uint32_t)(slots - 1); vm.leaf = leaf;
    for (int a = 0; a < 3; ++a) { vm.mn[a] = box[a]; vm.mx[a] = box[3 + a]; }
    for (int64_t j = 0; j < n_vox; ++j) {                 // (the table as k_vmap_write fills it, one key after the other)
        const uint64_t key = vmap_key((uint64_t)(coords[3 * j] - box[0]), (uint64_t)(coords[3 * j + 1] - box[1]), (uint64_t)(coords[3 * j + 2] - box[2]));
        uint32_t s = vmap_slot(key, vm.mask);
        while (keys[s] != kVmapEmpty) s = (s + 1u) & vm.mask;
        keys[s] = key; vals[s] = (uint32_t)j;
    }
    VlinArgs a;
    a.source_cov = mode; a.c = 1.0 - eps; a.robust = robust; a.robust_c2 = robust_scale * robust_scale;
    PoseArg P{};
    std::memcpy(P.R, R, sizeof(P.R)); std::memcpy(P.t, t, sizeof(P.t));
    double acc[31];
    for (int k = 0; k < 31; ++k) sums[k] = 0.0;
    std::vector<uint32_t> vix((size_t)S);
    for (int64_t i = 0; i < n; ++i) {
        const size_t oi = order[i];
        const double px = (double)src[3 * i], py = (double)src[3 * i + 1], pz = (double)src[3 * i + 2];
        float qx, qy, qz;
        body_to_global(P, px, py, pz, qx, qy, qz);
        const double v0 = floor((double)qx / vm.leaf), v1 = floor((double)qy / vm.leaf), v2 = floor((double)qz / vm.leaf);
        bool any = false;
        for (int j = 0; j < S; ++j) {
            double dx, dy, dz;
            vlin_offset(S, j, dx, dy, dz);
            vix[(size_t)j] = vmap_find_voxel(vm, v0 + dx, v1 + dy, v2 + dz);
            any |= vix[(size_t)j] != kNoIdx;
        }
        bool has_normal = false;
        double m[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
        if (mode && any)
            has_normal = vlin_normal(P, float4{src_normals4[4 * i], src_normals4[4 * i + 1], src_normals4[4 * i + 2], src_normals4[4 * i + 3]}, m, u);
        for (int k = 0; k < 3; ++k) normal_src[3 * oi + k] = m[k];
        bool eff = false;
        for (int j = 0; j < S; ++j) {
            const size_t oj = oi * (size_t)S + (size_t)j;
            GlinPoint o;
            VlinPoint x;
            const uint8_t f = vlin_corr(vm, a, vix[(size_t)j], qx, qy, qz, [&](double (&uj)[3]) {
                uj[0] = u[0]; uj[1] = u[1]; uj[2] = u[2];
                return has_normal;
            }, o, x);
            eff |= f == 1;
            voxel_idx[oj] = x.vidx == kNoIdx ? -1 : (int32_t)x.vidx;
            flag[oj] = f;
            for (int k = 0; k < 6; ++k) cov[6 * oj + k] = x.cov[k];
            for (int k = 0; k < 3; ++k) {
                mean[3 * oj + k] = x.mean[k];
                for (int c = 0; c < 3; ++c) w[9 * oj + 3 * k + c] = o.w[k][c];
            }
            for (int k = 0; k < 3; ++k) {
                double rw[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                if (f == 1) {
                    glin_row(P, px, py, pz, o.w[k][0], o.w[k][1], o.w[k][2], o.e[0], o.e[1], o.e[2], rw);
                    if (a.robust) glin_row_scale(o.k, rw);
                }
                r[3 * oj + k] = rw[7];
                for (int c = 0; c < 8; ++c) row[(3 * oj + k) * 8 + c] = rw[c];
                row_products(rw, f, acc);
                for (int c = 0; c < 29; ++c) sums[c] += acc[c];
            }
        }
        sums[29] += eff ? 1.0 : 0.0;
        sums[30] += any ? 1.0 : 0.0;
    }
    return 0;
}

}
