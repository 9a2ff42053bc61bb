// The third engine's linearisation on the device (include/dcreg.h: dcreg_linearize_gicp): plane-to-plane (Generalized-ICP) rows from the
// map's kept normals and the source's own, with the rule of the header, bitwise the numpy reference of tests/gicp_ref.py.
//   glin_block<DUMP>  what every block of this engine does, in one place; k_glin and k_glin_batch are block-uniform prologues in front of it
//   k_glin<DUMP>   one lane per source point, in the context's curve order: glin_point (gicp.hpp) - transform, k_nlin's 1-NN search from
//                  the warm bound, one gather of the nearest point and one of its float4 normal, the coalesced float4 load of the point's
//                  own normal, the covariance of the pair from the two normals, its Cholesky factor and W = L^-1; then THREE rows per
//                  point, each built just before its pass over the matrix cores (gicp.hpp wave_gram3_mfma: row 0 of every point precedes
//                  row 1 of any, one accumulator through the 24 steps), and the block row in LDS, added in wave order
//   k_glin_batch   the same for many poses in ONE launch (dcreg_gicp_batch_begin: the engine of dcreg_register_frames_gicp): block (x, pose)
//                  runs glin_point on block x of the pose's own source slice and its kept normals, and leaves its row at partials[pose][x]
//   k_finalize     (kernels.hpp) the block rows in chunk order, as for k_nlin
// The host side is the seam of normal_icp.hip (context.hpp): one_nn_run for the single pose and one_nn_batch_begin / rows_batch_end for
// many - the 1-NN layer, shared with the second engine, on top of the rows_* layer all three row engines share - with this engine's
// refusal (gicp_refuse), its launch arguments (glin_args), its kernels and the fields of its dump; the block rows, the result row and
// the dump block are nicp's.
// No floating-point atomics anywhere: the sums are a function of the rows and their order.  The search reads and writes the warm words of
// k_nlin (context.hpp NormalIcpBufs::warm): both engines look for the same nearest point, and the word decides how fast, never which.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../../include/dcreg_debug.h"
#include "context.hpp"
#include "gicp.hpp"

namespace dcreg {
namespace {

struct GlinDump {
    int32_t *nn_idx; float *nn_d2; uint8_t *flag; double *normal_map, *normal_src, *w, *r, *row;
};

// The body of both kernels: block blockIdx.x of the n_src points at src against the index g and its kept normals at pose P; the block row
// goes to `out`.  warm_in / warm_out: as k_nlin's.  src_normals: float4 per source point in the order of src.  Slot 29 counts the effective
// POINTS (not rows), slot 30 the points inside the radius.
template <bool DUMP>
__device__ __forceinline__ void glin_block(const float4 *__restrict__ src, uint32_t n_src, const GridDev &g, const float4 *__restrict__ normals,
                                           const float4 *__restrict__ src_normals, const PoseArg &P, const GlinArgs &a, const uint32_t *warm_in,
                                           uint32_t *warm_out, double *__restrict__ out, const GlinDump &d) {
    __shared__ RunList runs[kLinBlock / kWave];
    __shared__ double gm[kLinBlock / kWave][64];
    __shared__ double cnt[kLinBlock / kWave][2];
    const int wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kLinBlock + threadIdx.x;
    uint8_t flag = 0;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    size_t oi = 0;
    GlinPoint o;
    if (i < n_src) {
        const float4 s4 = src[i];
        sx = s4.x; sy = s4.y; sz = s4.z;
        flag = glin_point(g, runs[wave], normals, P, a, s4, src_normals + i, warm_in ? warm_in[i] : kNoIdx, o);
        if (warm_out) warm_out[i] = o.pos;
        if constexpr (DUMP) {
            oi = __float_as_uint(s4.w);
            if (d.nn_idx) d.nn_idx[oi] = o.idx == kNoIdx ? -1 : (int32_t)o.idx;
            if (d.nn_d2) d.nn_d2[oi] = o.d2;
            if (d.flag) d.flag[oi] = flag;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (d.normal_map) d.normal_map[3 * oi + k] = o.n[k];
                if (d.normal_src) d.normal_src[3 * oi + k] = o.m[k];
#pragma unroll
                for (int j = 0; j < 3; ++j) if (d.w) d.w[9 * oi + 3 * k + j] = o.w[k][j];
            }
        }
    }
    glin_block_rows(P, a.robust, flag, sx, sy, sz, o, runs[wave].stage, gm, cnt, out, [&](int k, const double (&row)[8]) {
        if constexpr (DUMP) {
            if (i < n_src) {
                if (d.r) d.r[3 * oi + k] = row[7];
                if (d.row) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) d.row[(3 * oi + k) * 8 + j] = row[j];
                }
            }
        }
    });
}

template <bool DUMP>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_glin(const float4 *__restrict__ src, uint32_t n_src, GridDev g,
                                                                     const float4 *__restrict__ normals, const float4 *__restrict__ src_normals,
                                                                     PoseArg P, GlinArgs a, const uint32_t *warm_in, uint32_t *warm_out,
                                                                     double *__restrict__ partials, GlinDump d) {
    glin_block<DUMP>(src, n_src, g, normals, src_normals, P, a, warm_in, warm_out, partials + (size_t)blockIdx.x * kSlots, d);
}

// Many poses in one launch: k_glin as k_nlin_batch is k_nlin (normal_icp.hip).  Block (x, pose): pose = poses[blockIdx.y], read through a
// block-uniform index; its cloud is slices[pose] of src AND of src_normals (a frame of the loaded frames and that frame's kept normals:
// the same positions; normal_icp.hpp batch_slice) or, slices == null, the n_src points at src (the context's own source and its kept
// source normals).  The warm words are k_nlin_batch's slots: the pose's own array, read unless it is fresh.  The block row goes to
// partials[pose * n_blocks_x + x], where k_finalize<SLICE> finds it: the rows and additions of the pose's single launch.
// GRIDS (scan pairs: dcreg_pairs_gicp_batch_begin): as k_nlin_batch<GRIDS> - grids[grid_ids[pose]], read through a block-uniform index, holds
// the pose's own target: its grid, its rings and where its kept normals start in `normals`; src and src_normals are the pairs' sources.
template <bool GRIDS>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_glin_batch(const float4 *__restrict__ src, uint32_t n_src, GridDev g,
                                                                           const float4 *__restrict__ normals, const float4 *__restrict__ src_normals,
                                                                           const PoseArg *__restrict__ poses, const uint2 *__restrict__ slices,
                                                                           GlinArgs a, uint32_t *warm, uint32_t warm_stride,
                                                                           double *__restrict__ partials, uint32_t n_blocks_x,
                                                                           const OneNnGrid *__restrict__ grids, const uint32_t *__restrict__ grid_ids) {
    const uint32_t pose_id = blockIdx.y;
    if constexpr (GRIDS) {                           // (uniform per block)
        const OneNnGrid &og = grids[grid_ids[pose_id]];
        g = og.g; a.max_ring = og.max_ring; normals += og.normals_first;
    }
    if (slices) {
        uint32_t first;
        if (!batch_slice(slices, first, n_src)) return;
        src += first; src_normals += first;
    }
    const PoseArg &P = poses[pose_id];
    uint32_t *w = P.state != kNoIdx ? warm + (size_t)P.state * warm_stride : nullptr;
    glin_block<false>(src, n_src, g, normals, src_normals, P, a, P.fresh == 0u ? w : nullptr, w,
                      partials + ((size_t)pose_id * n_blocks_x + blockIdx.x) * kSlots, GlinDump{});
}

// the launch's arguments for a search within the bound b ("gicp_epsilon", "robust_kernel" and "gicp_robust_scale" are read at every call)
GlinArgs glin_args(const dcreg_ctx *c, const OneNnBound &b) {
    GlinArgs a;
    a.radius_sq = b.radius_sq; a.bound_f = b.bound_f; a.max_ring = b.max_ring;
    a.c = 1.0 - c->opt_gicp_epsilon;
    a.robust = c->opt_robust_kernel; a.robust_c2 = c->opt_gicp_robust_scale * c->opt_gicp_robust_scale;
    return a;
}

// this engine's state refusals, after "no kept normals": the single-pose call (fs == null) and the batched form over the loaded frames or
// the pairs' sources (the second engine's seam, normal_icp.hip one_nn_batch_begin)
int gicp_refuse(dcreg_ctx *c, const dcreg_ctx::FrameSet *fs) {
    if (fs == &c->pair_src && !fs->normals_kept) { c->fail("no kept pair source normals: dcreg_pairs_sources_normals_keep or dcreg_pairs_sources_normals_set first"); return DCREG_E_STATE; }
    if (fs && !fs->normals_kept) { c->fail("no kept frame normals: dcreg_frames_normals_keep or dcreg_frames_normals_set first"); return DCREG_E_STATE; }
    if (!fs && !c->gicp.src_kept) { c->fail("no kept source normals: dcreg_source_normals_keep or dcreg_source_normals_set first"); return DCREG_E_STATE; }
    return DCREG_OK;
}

int glin_run(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, dcreg_lin_out *out, dcreg_glin_debug *dbg) {
    GlinDump d{};
    const dcreg_glin_debug none{}, &h = dbg ? *dbg : none;
    const DumpField fields[] = {{h.normal_map, 24, &d.normal_map}, {h.normal_src, 24, &d.normal_src}, {h.w, 72, &d.w}, {h.r, 24, &d.r},
                                     {h.row, 192, &d.row}, {h.nn_idx, 4, &d.nn_idx}, {h.nn_d2, 4, &d.nn_d2}, {h.flag, 1, &d.flag}};
    return one_nn_run(c, R, t, p, out, "GICP", gicp_refuse, [&](const OneNnLaunch &L) {
        hipLaunchKernelGGL(L.dump ? k_glin<true> : k_glin<false>, dim3(L.nb), dim3(kLinBlock), 0, c->stream, c->d_src.data(), (uint32_t)c->n_src,
                           c->map.grid, c->nicp.normals.data(), c->gicp.src_normals.data(), L.P, glin_args(c, L.bound), L.warm_in, L.warm_out,
                           L.partials, d);
    }, dbg != nullptr, fields, 8);
}

void glin_batch_launch(dcreg_ctx *c, const OneNnBatch &L) {
    const GlinArgs a = glin_args(c, L.bound);
    hipLaunchKernelGGL(L.grids ? k_glin_batch<true> : k_glin_batch<false>, dim3(L.nbx, (unsigned)L.n_poses), dim3(kLinBlock), 0, c->stream, L.src, L.n_src,
                       L.g, L.normals, L.src_normals, L.poses, L.slices, a, L.warm, L.warm_stride, L.partials, L.nbx, L.grids, L.grid_ids);
}

}  // namespace
}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_linearize_gicp(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out) {
    return glin_run(c, R, t, p, out, nullptr);
}
int dcreg_gicp_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                           const int32_t *frame_ids, const dcreg_lin_params *p) {
    return one_nn_batch_begin(c, slot, n_poses, R9, t3, state_ids, c ? &c->frames : nullptr, frame_ids, nullptr, p, gicp_refuse, glin_batch_launch,
                              "the k_glin_batch launch");
}
int dcreg_pairs_gicp_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                                 const int32_t *source_ids, const int32_t *target_ids, const dcreg_lin_params *p) {
    if (c && (!source_ids || !target_ids)) { c->fail("null argument"); return DCREG_E_INVALID; }
    return one_nn_batch_begin(c, slot, n_poses, R9, t3, state_ids, c ? &c->pair_src : nullptr, source_ids, target_ids, p, gicp_refuse, glin_batch_launch,
                              "the k_glin_batch launch");
}
int dcreg_gicp_batch_end(dcreg_ctx *c, int slot, dcreg_lin_out *outs) { return rows_batch_end(c, slot, outs); }
int dcreg_linearize_gicp_debug(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out,
                               dcreg_glin_debug *dbg) {
    if (c && !dbg) { c->fail("null dump"); return DCREG_E_INVALID; }
    return glin_run(c, R, t, p, out, dbg);
}
}
