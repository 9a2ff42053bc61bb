// TEST INFRASTRUCTURE ONLY: host replay of the fourth engine's per-point functions (dcreg_amd/csrc/device/voxel_icp.hpp: vmap_find - the
// lookup through the open-addressing table - and vlin_point - the covariance, its factor and W; gicp.hpp: glin_row, glin_row_scale), in a
// library of its own (tests/emul_vlin.py).  The replay's own C-ABI (emul.cpp) comes along unchanged.
#include "emul.cpp"
#include "../../dcreg_amd/csrc/device/voxel_icp.hpp"

extern "C" {

// One linearisation over the n source points at src (processing order, 3 floats each; order[i] = the point's original index) against
// n_vox records (12 floats each, as the device keeps them) at the voxel coordinates coords (3 int64 each); box: minimum and maximum voxel
// of the map (3 + 3).  The table is filled here as k_vmap_write fills it, one key after the other.  src_normals4: float4 per source
// point in PROCESSING order (mode 1; else null).  The dump arrays are in original source order; sums: the 31 sums added row by row in
// processing order.
int emu_vlin(const float *recs, const int64_t *coords, int64_t n_vox, double leaf, const int64_t *box, const float *src, const float *src_normals4,
             const uint32_t *order, int64_t n, const double *R, const double *t, int mode, double eps, int robust, double robust_scale,
             int32_t *voxel_idx, uint8_t *flag, double *mean, double *cov, double *normal_src, double *w, double *r, double *row, double *sums) {
    size_t slots = 2;
    while (slots < 2 * (size_t)n_vox) slots <<= 1;
    std::vector<uint64_t> keys(slots, kVmapEmpty);
    std::vector<uint32_t> vals(slots, 0u);
    VoxMapDev vm;
    vm.recs = (const float4 *)recs; vm.keys = keys.data(); vm.vals = vals.data(); vm.mask = (uint32_t)(slots - 1); vm.leaf = leaf;
    for (int a = 0; a < 3; ++a) { vm.mn[a] = box[a]; vm.mx[a] = box[3 + a]; }
    for (int64_t j = 0; j < n_vox; ++j) {
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
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t oi = order[i];
        const float4 s4{src[3 * i], src[3 * i + 1], src[3 * i + 2], __uint_as_float(oi)};
        float4 m4{0.f, 0.f, 0.f, 0.f};
        if (mode) m4 = float4{src_normals4[4 * i], src_normals4[4 * i + 1], src_normals4[4 * i + 2], src_normals4[4 * i + 3]};
        GlinPoint o;
        VlinPoint x;
        const uint8_t f = vlin_point(vm, P, a, s4, &m4, o, x);
        voxel_idx[oi] = x.vidx == kNoIdx ? -1 : (int32_t)x.vidx;
        flag[oi] = f;
        for (int k = 0; k < 6; ++k) cov[6 * (size_t)oi + k] = x.cov[k];
        for (int k = 0; k < 3; ++k) {
            mean[3 * (size_t)oi + k] = x.mean[k]; normal_src[3 * (size_t)oi + k] = o.m[k];
            for (int j = 0; j < 3; ++j) w[9 * (size_t)oi + 3 * k + j] = o.w[k][j];
        }
        for (int k = 0; k < 3; ++k) {
            double rw[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (f == 1) {
                glin_row(P, (double)s4.x, (double)s4.y, (double)s4.z, o.w[k][0], o.w[k][1], o.w[k][2], o.e[0], o.e[1], o.e[2], rw);
                if (a.robust) glin_row_scale(o.k, rw);
            }
            r[3 * (size_t)oi + k] = rw[7];
            for (int j = 0; j < 8; ++j) row[(3 * (size_t)oi + k) * 8 + j] = rw[j];
            row_products(rw, f, acc);
            for (int j = 0; j < 29; ++j) sums[j] += acc[j];
        }
        sums[29] += f == 1 ? 1.0 : 0.0;
        sums[30] += f != 0 ? 1.0 : 0.0;
    }
    return 0;
}

}
