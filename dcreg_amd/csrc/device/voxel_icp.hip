// The fourth engine's linearisation on the device (include/dcreg.h: dcreg_linearize_voxels): rows against the map's kept voxel
// distributions (voxel.hip voxel_map_keep), with the rule of the header, bitwise the numpy reference of tests/voxels_ref.py
// (with neighbour voxels: tests/voxels_stencil_ref.py).
//   vlin_block<DUMP, S>  what every block of this engine does, in one place (S = "voxels_neighbors"; this is S = 1, S = 7 / 27 at the body): one lane per source point, in the cloud's curve order: vlin_point
//                  (voxel_icp.hpp) - transform, the lookup of the voxel the point falls into (no search: nothing is walked, nothing is
//                  kept between calls), three 16-byte gathers of its record, in mode 1 the coalesced float4 load of the point's own
//                  normal, the covariance, its Cholesky factor and W = L^-1; then the third engine's block tail (gicp.hpp
//                  glin_block_rows): three rows per point over the matrix cores, the block row in LDS, added in wave order.  Its LDS is
//                  the staging area of the Gram pass and the waves' sums - no RunList
// The three kernels are block-uniform prologues in front of it - they pick the cloud, the pose, the voxel map and the output row:
//   k_vlin<DUMP, S>  the context's source, pose and kept voxel map: block x leaves partials[x]
//   k_vlin_batch<S>  many poses in ONE launch (dcreg_voxels_batch_begin: the engine of dcreg_register_frames_voxels): block (x, pose), every
//                  pose its own cloud - a frame of the loaded frames or the context's source
//   k_vlin_pairs<S>  ... with a voxel map per pose (dcreg_pairs_voxels_batch_begin: the engine of dcreg_register_pairs_voxels): every pose
//                  its own source of the pairs' sources and its own target's map of the pairs' voxel batch (voxel.hip
//                  pairs_voxels_build), read through a block-uniform index
//   k_finalize     (kernels.hpp) the block rows in chunk order, as for k_glin
// On the host the engine brings its refusals, its launch and the fields of its dump to the seam all engines that leave block rows share
// (normal_icp.hip, declared in context.hpp): vlin_run ends in rows_run (buffers, dump block, launch, k_finalize, wait); the batched forms
// make the common refusals with rows_batch_check, resolve their clouds with rows_batch_clouds and queue through rows_batch_queue.
// The engine reads the source, the kept voxel map and - in mode 1 - the kept source normals; it neither reads nor writes warm words,
// warm slots, neighbour states, the window index (no roi_ensure) or the map's kept normals.
// No floating-point atomics anywhere: the sums are a function of the rows and their order.
#include <cmath>
#include <cstring>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "../../../include/dcreg_debug.h"
#include "context.hpp"
#include "voxel_icp.hpp"

namespace dcreg {
namespace {

struct VlinDump {
    int32_t *voxel_idx; uint8_t *flag; double *mean, *cov, *normal_src, *w, *r, *row;
};

// The body of the three kernels: block blockIdx.x of the n_src points at src against the voxel map vm at pose P; the block row goes to
// `out`.  src_normals: float4 per source point in the order of src (null in mode 0, and never read).  member == false (a pair target
// that kept no voxel): no table and no record is read, the points keep flag 0 and the block row is the zero row.  Slot 29 counts the
// effective POINTS (not rows), slot 30 the points with a correspondence (S = 1: the points that fall into a kept voxel).
// S = "voxels_neighbors".  S = 1 is the one correspondence of vlin_point and the third engine's block tail.  S = 7 / 27: the S lookups
// first - one record number per correspondence, kept in a lane-private column of LDS so that the loop over j stays rolled and indexes no
// register array - in mode 1 the point's normal once, then per j the correspondence (vlin_corr) just before its three passes; the
// accumulator of the matrix cores lives across all 3 S passes (pass 3 j + k).  The plain kernels leave out what a wave need not do: a j
// that none of its lanes found a voxel for is not built, and the three passes of a j with no effective lane are not made (their rows are
// zero: no bit moves).  The dump builds and passes every j.
template <bool DUMP, int S>
__device__ __forceinline__ void vlin_block(const float4 *__restrict__ src, uint32_t n_src, const VoxMapDev &vm, bool member,
                                           const float4 *__restrict__ src_normals, const PoseArg &P, const VlinArgs &a,
                                           double *__restrict__ out, const VlinDump &d) {
    __shared__ double stage[kLinBlock / kWave][kWave * kRowStride];
    __shared__ double gm[kLinBlock / kWave][64];
    __shared__ double cnt[kLinBlock / kWave][2];
    const int wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kLinBlock + threadIdx.x;
    if constexpr (S == 1) {
        uint8_t flag = 0;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        size_t oi = 0;
        GlinPoint o;
        if (i < n_src) {
            const float4 s4 = src[i];
            sx = s4.x; sy = s4.y; sz = s4.z;
            VlinPoint x;
            if (member) flag = vlin_point(vm, P, a, s4, src_normals + i, o, x);
            if constexpr (DUMP) {
                oi = __float_as_uint(s4.w);
                if (d.voxel_idx) d.voxel_idx[oi] = x.vidx == kNoIdx ? -1 : (int32_t)x.vidx;
                if (d.flag) d.flag[oi] = flag;
#pragma unroll
                for (int k = 0; k < 6; ++k) if (d.cov) d.cov[6 * oi + k] = x.cov[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (d.mean) d.mean[3 * oi + k] = x.mean[k];
                    if (d.normal_src) d.normal_src[3 * oi + k] = o.m[k];
#pragma unroll
                    for (int j = 0; j < 3; ++j) if (d.w) d.w[9 * oi + 3 * k + j] = o.w[k][j];
                }
            }
        }
        glin_block_rows(P, a.robust, flag, sx, sy, sz, o, stage[wave], gm, cnt, out, [&](int k, const double (&row)[8]) {
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
    } else {
        __shared__ uint32_t vix[S][kLinBlock];           // [j][thread]: the record number of the thread's correspondence j (kNoIdx: none)
        const int lane = threadIdx.x & 63;
        const bool live = i < n_src;
        float sx = 0.f, sy = 0.f, sz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
        size_t oi = 0;
        if (live) {
            const float4 s4 = src[i];
            sx = s4.x; sy = s4.y; sz = s4.z;
            oi = __float_as_uint(s4.w);
            body_to_global(P, (double)sx, (double)sy, (double)sz, qx, qy, qz);
        }
        // ---- the S lookups, ahead of everything that waits for a record
        bool any = false;
        if (live && member) {
            const double v0 = floor((double)qx / vm.leaf), v1 = floor((double)qy / vm.leaf), v2 = floor((double)qz / vm.leaf);
#pragma unroll 1
            for (int j = 0; j < S; ++j) {
                double dx, dy, dz;
                vlin_offset(S, j, dx, dy, dz);
                const uint32_t r = vmap_find_voxel(vm, v0 + dx, v1 + dy, v2 + dz);
                vix[j][threadIdx.x] = r;
                any |= r != kNoIdx;
            }
        } else {
#pragma unroll 1
            for (int j = 0; j < S; ++j) vix[j][threadIdx.x] = kNoIdx;
        }
        // ---- the point's own normal, once (mode 1, and only a point with a correspondence reads it)
        bool has_normal = false;
        double m[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
        if (a.source_cov && any) has_normal = vlin_normal(P, src_normals[i], m, u);
        if constexpr (DUMP) {
            if (live && d.normal_src) {
#pragma unroll
                for (int k = 0; k < 3; ++k) d.normal_src[3 * oi + k] = m[k];
            }
        }
        // ---- correspondence j just before its three passes
        WaveGram G;
        G.begin(stage[wave], lane);
        bool eff_pt = false;
#pragma unroll 1
        for (int j = 0; j < S; ++j) {
            const uint32_t vidx = vix[j][threadIdx.x];
            if constexpr (!DUMP) {
                if (__builtin_amdgcn_ballot_w64(vidx != kNoIdx) == 0ull) continue;      // (wave-uniform) nobody has this neighbour
            }
            GlinPoint o;
            VlinPoint x;
            const uint8_t flag = vlin_corr(vm, a, vidx, qx, qy, qz, [&](double (&uj)[3]) {
                uj[0] = u[0]; uj[1] = u[1]; uj[2] = u[2];
                return has_normal;
            }, o, x);
            eff_pt |= flag == 1;
            const size_t oj = oi * (size_t)S + (size_t)j;
            if constexpr (DUMP) {
                if (live) {
                    if (d.voxel_idx) d.voxel_idx[oj] = vidx == kNoIdx ? -1 : (int32_t)vidx;
                    if (d.flag) d.flag[oj] = flag;
#pragma unroll
                    for (int k = 0; k < 6; ++k) if (d.cov) d.cov[6 * oj + k] = x.cov[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (d.mean) d.mean[3 * oj + k] = x.mean[k];
#pragma unroll
                        for (int c = 0; c < 3; ++c) if (d.w) d.w[9 * oj + 3 * k + c] = o.w[k][c];
                    }
                }
            } else {
                if (__builtin_amdgcn_ballot_w64(flag == 1) == 0ull) continue;           // (wave-uniform) three passes of zero rows
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double row[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) row[c] = 0.0;
                if (flag == 1) {
                    glin_row(P, (double)sx, (double)sy, (double)sz, o.w[k][0], o.w[k][1], o.w[k][2], o.e[0], o.e[1], o.e[2], row);
                    if (a.robust) glin_row_scale(o.k, row);      // (launch-uniform; with no kernel nothing is multiplied)
                }
                if constexpr (DUMP) {
                    if (live) {
                        if (d.r) d.r[3 * oj + k] = row[7];
                        if (d.row) {
#pragma unroll
                            for (int c = 0; c < 8; ++c) d.row[(3 * oj + k) * 8 + c] = row[c];
                        }
                    }
                }
                G.pass(row, stage[wave], lane);
            }
        }
        double u0, u1;
        G.end(lane, u0, u1);
        glin_block_tail(u0, u1, eff_pt, any, gm, cnt, out);
    }
}

template <bool DUMP, int S>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_vlin(const float4 *__restrict__ src, uint32_t n_src, VoxMapDev vm,
                                                                     const float4 *__restrict__ src_normals, PoseArg P, VlinArgs a,
                                                                     double *__restrict__ partials, VlinDump d) {
    vlin_block<DUMP, S>(src, n_src, vm, true, src_normals, P, a, partials + (size_t)blockIdx.x * kSlots, d);
}

// Many poses in one launch: k_vlin as k_glin_batch is k_glin (gicp.hip).  Block (x, pose): pose = poses[blockIdx.y], read through a
// block-uniform index; its cloud is slices[pose] of src and - in mode 1 - of src_normals (a frame of the loaded frames and that frame's
// kept normals: the same positions; normal_icp.hpp batch_slice) or, slices == null, the n_src points at src (the context's own source
// and its kept source normals).  The block row goes to partials[pose * n_blocks_x + x], where k_finalize<SLICE> finds it: the rows and
// additions of the pose's single launch.  Nothing is kept between launches, so there are no warm words.
template <int S>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_vlin_batch(const float4 *__restrict__ src, uint32_t n_src, VoxMapDev vm,
                                                                           const float4 *__restrict__ src_normals,
                                                                           const PoseArg *__restrict__ poses, const uint2 *__restrict__ slices,
                                                                           VlinArgs a, double *__restrict__ partials, uint32_t n_blocks_x) {
    const uint32_t pose_id = blockIdx.y;
    if (slices) {
        uint32_t first;
        if (!batch_slice(slices, first, n_src)) return;
        src += first;
        if (src_normals) src_normals += first;       // (mode 0: null, and never read)
    }
    vlin_block<false, S>(src, n_src, vm, true, src_normals, poses[pose_id], a, partials + ((size_t)pose_id * n_blocks_x + blockIdx.x) * kSlots,
                         VlinDump{});
}

// Scan pairs in one launch (dcreg_pairs_voxels_batch_begin: the engine of dcreg_register_pairs_voxels): k_vlin_batch with a voxel map per
// pose.  Block (x, pose): its cloud is slices[pose] of the pairs' sources (and, in mode 1, of their kept normals); its target is
// maps[target_ids[pose]] of the pairs' voxel batch (voxel.hip pairs_voxels_build), read through a block-uniform index as
// k_nlin_batch<GRIDS> reads its OneNnGrid - the VoxMapDev that vlin_point takes is formed from that record: the target's own records, its
// own table, its own box; the leaf is the batch's.  A pose whose target has no member (n_kept 0) leaves the zero row.
template <int S>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_vlin_pairs(const float4 *__restrict__ src, const float4 *__restrict__ src_normals,
                                                                           const PairVoxMap *__restrict__ maps, const uint32_t *__restrict__ target_ids,
                                                                           const float4 *__restrict__ recs, const uint64_t *__restrict__ t_keys,
                                                                           const uint32_t *__restrict__ t_vals, double leaf,
                                                                           const PoseArg *__restrict__ poses, const uint2 *__restrict__ slices,
                                                                           VlinArgs a, double *__restrict__ partials, uint32_t n_blocks_x) {
    const uint32_t pose_id = blockIdx.y;
    uint32_t first, n_src;
    if (!batch_slice(slices, first, n_src)) return;
    src += first;
    if (src_normals) src_normals += first;           // (mode 0: null, and never read)
    const PairVoxMap &m = maps[target_ids[pose_id]];
    vlin_block<false, S>(src, n_src, vox_map_dev(recs + (size_t)m.first * kVmapRecWords, t_keys + m.base, t_vals + m.base, m.mask, m.mn, m.mx, leaf),
                         m.n_kept != 0u, src_normals, poses[pose_id], a, partials + ((size_t)pose_id * n_blocks_x + blockIdx.x) * kSlots, VlinDump{});
}

// "voxels_neighbors" picks the instantiation: f(std::integral_constant<int, S>) with the option's S (read at every call, as vlin_args)
template <class F>
void vlin_stencil(const dcreg_ctx *c, F f) {
    switch (c->opt_voxels_neighbors) {
    case 7: f(std::integral_constant<int, 7>{}); break;
    case 27: f(std::integral_constant<int, 27>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;      // (dcreg_set_option admits 1, 7 and 27)
    }
}

// the launch's arguments ("voxels_source_cov", "gicp_epsilon", "robust_kernel" and "gicp_robust_scale" are read at every call, and so is
// "voxels_neighbors": vlin_stencil)
VlinArgs vlin_args(const dcreg_ctx *c) {
    VlinArgs a;
    a.source_cov = c->opt_voxels_source_cov; a.c = 1.0 - c->opt_gicp_epsilon;
    a.robust = c->opt_robust_kernel; a.robust_c2 = c->opt_gicp_robust_scale * c->opt_gicp_robust_scale;
    return a;
}

int vlin_run(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, dcreg_lin_out *out, dcreg_vlin_debug *dbg) {
    // ---- dcreg_linearize_gicp's refusals in its order, with "no kept voxels" in place of "no kept normals"
    if (!c) return DCREG_E_INVALID;
    if (!R || !t || !p || !out) { c->fail("null linearisation arguments"); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    if (p->parameterization != DCREG_PARAM_SO3) { c->fail("the voxel linearisation has the SO(3) row only (parameterization %d)", p->parameterization); return DCREG_E_INVALID; }
    if (!finite_n(R, 9) || !finite_n(t, 3)) { c->fail("the pose is not finite"); return DCREG_E_INVALID; }
    if ((c->roi_active ? c->roi_store : c->map).n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    const dcreg_ctx::VoxelMapBufs &M = c->vmap;
    if (!M.kept) { c->fail("no kept voxels: dcreg_target_voxels_keep first"); return DCREG_E_STATE; }
    const VlinArgs a = vlin_args(c);
    if (a.source_cov && !c->gicp.src_kept) { c->fail("no kept source normals: dcreg_source_normals_keep or dcreg_source_normals_set first"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    VlinDump d{};
    const dcreg_vlin_debug none{}, &h = dbg ? *dbg : none;
    const size_t S = (size_t)c->opt_voxels_neighbors;      // the dump holds S correspondences per point; the source normal is the point's
    const DumpField fields[] = {{h.mean, 24 * S, &d.mean}, {h.cov, 48 * S, &d.cov}, {h.normal_src, 24, &d.normal_src}, {h.w, 72 * S, &d.w},
                                {h.r, 24 * S, &d.r}, {h.row, 192 * S, &d.row}, {h.voxel_idx, 4 * S, &d.voxel_idx}, {h.flag, S, &d.flag}};
    const VoxMapDev vm = vox_map_dev(M.recs.data(), M.t_keys.data(), M.t_vals.data(), M.mask, M.mn, M.mx, M.leaf);
    PoseArg P;
    std::memcpy(P.R, R, sizeof(P.R)); std::memcpy(P.t, t, sizeof(P.t));
    P.state = kNoIdx; P.fresh = 1;
    return rows_run(c, out, fields, dbg ? 8 : 0, [&](double *partials, uint32_t nb) {
        vlin_stencil(c, [&](auto s) {
            constexpr int S = decltype(s)::value;
            const auto kernel = dbg ? k_vlin<true, S> : k_vlin<false, S>;
            hipLaunchKernelGGL(kernel, dim3(nb), dim3(kLinBlock), 0, c->stream, c->d_src.data(),
                               (uint32_t)c->n_src, vm, a.source_cov ? c->gicp.src_normals.data() : (const float4 *)nullptr, P, a, partials, d);
        });
    });
}

// The batched launch (include/dcreg_debug.h: dcreg_voxels_batch_begin): every refusal in the header's order - the launch slots' and
// vlin_run's - before anything is queued, then the shared slot plumbing with k_vlin_batch as its kernel.  The options are read here.
int vlin_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *frame_ids, const dcreg_lin_params *p) {
    if (int rc = rows_batch_check(c, slot, n_poses, R9, t3, p, true, "voxel", false)) return rc;
    if ((c->roi_active ? c->roi_store : c->map).n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    const dcreg_ctx::VoxelMapBufs &M = c->vmap;
    if (!M.kept) { c->fail("no kept voxels: dcreg_target_voxels_keep first"); return DCREG_E_STATE; }
    dcreg_ctx::FrameSet *fs = frame_ids ? &c->frames : nullptr;
    int64_t n_max;
    if (int rc = rows_batch_clouds(c, fs, n_poses, frame_ids, "frame", nullptr, n_max)) return rc;
    const VlinArgs a = vlin_args(c);
    if (a.source_cov && fs && !fs->normals_kept) { c->fail("no kept frame normals: dcreg_frames_normals_keep or dcreg_frames_normals_set first"); return DCREG_E_STATE; }
    if (a.source_cov && !fs && !c->gicp.src_kept) { c->fail("no kept source normals: dcreg_source_normals_keep or dcreg_source_normals_set first"); return DCREG_E_STATE; }
    const VoxMapDev vm = vox_map_dev(M.recs.data(), M.t_keys.data(), M.t_vals.data(), M.mask, M.mn, M.mx, M.leaf);
    return rows_batch_queue(c, slot, n_poses, R9, t3, nullptr, fs, frame_ids, nullptr, n_max, [&](OneNnBatch &L) {
        vlin_stencil(c, [&](auto s) {
            hipLaunchKernelGGL(k_vlin_batch<decltype(s)::value>, dim3(L.nbx, (unsigned)L.n_poses), dim3(kLinBlock), 0, c->stream, L.src, L.n_src, vm,
                               a.source_cov ? L.src_normals : (const float4 *)nullptr, L.poses, L.slices, a, L.partials, L.nbx);
        });
    }, "the k_vlin_batch launch");
}

// The pairs launch (include/dcreg_debug.h: dcreg_pairs_voxels_batch_begin): vlin_batch_begin's refusals in its order - null ids are null
// arguments; "no pair voxel batch built" and "no pair sources" in place of "no target", "no kept voxels" and "no frames"; pose i's source
// is checked before its target - then the shared slot plumbing with k_vlin_pairs as its kernel; the pose's target rides where the 1-NN
// pairs launches carry theirs (OneNnBatch::grid_ids)
int vlin_pairs_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *source_ids, const int32_t *target_ids,
                           const dcreg_lin_params *p) {
    if (int rc = rows_batch_check(c, slot, n_poses, R9, t3, p, source_ids && target_ids, "voxel", false)) return rc;
    const dcreg_ctx::PairVoxBufs &V = c->pvox;
    if (V.n <= 0) { c->fail("no pair voxel batch built: dcreg_pairs_voxels_build first"); return DCREG_E_STATE; }
    dcreg_ctx::FrameSet *fs = &c->pair_src;
    int64_t n_max;
    if (int rc = rows_batch_clouds(c, fs, n_poses, source_ids, "pair source", [&](int i) {
            const int32_t t = target_ids[i];
            if (t < 0 || t >= V.n) { c->fail("pair target %d is not in the voxel batch", t); return DCREG_E_INVALID; }
            return DCREG_OK;
        }, n_max)) return rc;
    const VlinArgs a = vlin_args(c);
    if (a.source_cov && !fs->normals_kept) { c->fail("no kept pair source normals: dcreg_pairs_sources_normals_keep or dcreg_pairs_sources_normals_set first"); return DCREG_E_STATE; }
    return rows_batch_queue(c, slot, n_poses, R9, t3, nullptr, fs, source_ids, target_ids, n_max, [&](OneNnBatch &L) {
        vlin_stencil(c, [&](auto s) {
            hipLaunchKernelGGL(k_vlin_pairs<decltype(s)::value>, dim3(L.nbx, (unsigned)L.n_poses), dim3(kLinBlock), 0, c->stream, L.src,
                               a.source_cov ? L.src_normals : (const float4 *)nullptr, V.d_maps.data(), L.grid_ids, V.recs.data(), V.t_keys.data(),
                               V.t_vals.data(), V.leaf, L.poses, L.slices, a, L.partials, L.nbx);
        });
    }, "the k_vlin_pairs launch");
}

}  // namespace

// "voxels_source_cov" for the engine's batched calls (engine.cpp reads it once when a call starts)
int voxels_source_cov(const dcreg_ctx *c) { return c->opt_voxels_source_cov; }

}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_linearize_voxels(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out) {
    return vlin_run(c, R, t, p, out, nullptr);
}
int dcreg_voxels_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *frame_ids,
                             const dcreg_lin_params *p) {
    return vlin_batch_begin(c, slot, n_poses, R9, t3, frame_ids, p);
}
int dcreg_voxels_batch_end(dcreg_ctx *c, int slot, dcreg_lin_out *outs) { return rows_batch_end(c, slot, outs); }
int dcreg_pairs_voxels_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *source_ids,
                                   const int32_t *target_ids, const dcreg_lin_params *p) {
    return vlin_pairs_batch_begin(c, slot, n_poses, R9, t3, source_ids, target_ids, p);
}
int dcreg_linearize_voxels_debug(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out,
                                 dcreg_vlin_debug *dbg) {
    if (c && !dbg) { c->fail("null dump"); return DCREG_E_INVALID; }
    return vlin_run(c, R, t, p, out, dbg);
}
}
