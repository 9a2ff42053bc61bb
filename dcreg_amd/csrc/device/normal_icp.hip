// The second engine's linearisation on the device (include/dcreg.h: dcreg_linearize_normals): 1-NN point-to-plane rows against the map's
// kept normals, with the rule of the header, bitwise the numpy reference of tests/normal_icp_ref.py.
//   k_nlin<DUMP>   one lane per source point, in the context's curve order: nlin_point (normal_icp.hpp) - transform, the ring walk of k_knn
//                  with a one-slot heap on (d2, index) keys, started from the bound the point's last nearest neighbour gives when there is
//                  one, one gather of the nearest point and one of its float4 normal, the row; then the wave's rows on the matrix cores
//                  (kernels.hpp wave_gram_mfma) and the block row in LDS, added in wave order
//   k_nlin_batch   the same for many poses in ONE launch (dcreg_normals_batch_begin: the engine of dcreg_register_frames_normals): block
//                  (x, pose) runs nlin_point on block x of the pose's own source slice - a frame of the loaded frames, or the context's
//                  source - with the pose read from a device array, and leaves its row at partials[pose][x]; <GRIDS>: against the pose's
//                  own target and that target's kept normals (dcreg_pairs_normals_batch_begin: dcreg_register_pairs_normals)
//   k_finalize     (kernels.hpp) the block rows in chunk order, the additions of the first engine's batched launches
// Both kernels end in nlin_block_rows (the wave's rows to LDS, block_slot_sum of kernels.hpp, the block row); the batched kernels of all
// three engines find their block's cloud with batch_slice (normal_icp.hpp).
// This file also holds the host seam of the three engines that leave block rows (declared in context.hpp), in two layers:
//   rows_*     for every such engine, the fourth (voxel_icp.hip) included: rows_run - the back half of a single-pose call: buffers, the dump
//              block cut from a table of fields, launch, k_finalize, wait; rows_batch_check - the front of every batched begin's refusal
//              ladder; rows_batch_clouds - the frame / pair-source ids resolved to the launch's largest cloud; rows_batch_queue / _end -
//              the launch slots' plumbing
//   one_nn_*   what belongs to the 1-NN search, for this engine AND gicp.hip's: one_nn_run - one_nn_check, roi_ensure, the warm words and
//              the search bound in front of rows_run; one_nn_batch_begin - the state refusals, the targets and the warm slots between
//              rows_batch_check and rows_batch_queue.  An engine brings its extra refusal, its kernel launch and its dump fields.
// No floating-point atomics anywhere: the sums are a function of the rows and their order.  A point's row depends on the clouds, the
// normals and the pose only; the warm position decides how fast the neighbour is found, never which.
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../../include/dcreg_debug.h"
#include "context.hpp"
#include "normal_icp.hpp"

namespace dcreg {
namespace {

struct NlinDump {
    int32_t *nn_idx; float *nn_d2; uint8_t *flag; double *normal, *r, *s, *row;
};

// What a block does with its points' rows once nlin_point has run (k_nlin and k_nlin_batch; the shape of gicp.hip's glin_block_rows): the
// wave's rows through the matrix cores (the wave's RunList is free now: it stages the rows; the lanes past the cloud's end carry a zero
// row and flag 0), the wave's Gram matrix and counts in LDS, added in wave order, and the block row at `out`
__device__ __forceinline__ void nlin_block_rows(const double (&row)[8], uint8_t flag, RunList &rl, double (*gm)[64], double (*cnt)[2],
                                                double *__restrict__ out) {
    wave_rows_to_lds(row, flag, rl.stage, gm[threadIdx.x >> 6], cnt);
    __syncthreads();
    if (threadIdx.x < kSlots) out[threadIdx.x] = block_slot_sum(&gm[0][0], 64, cnt);
}

// warm_in: the positions of the last launch (null: search cold), warm_out: where this launch leaves its own (null: nowhere; the same
// array as warm_in in a plain call: a lane reads its word before it writes it, and no other lane's).  Block b
// leaves its row at partials[b]: slots 0..28 the Gram entries of gram_entry_of_slot, 29 effective points, 30 points inside the radius
template <bool DUMP>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_nlin(const float4 *__restrict__ src, uint32_t n_src, GridDev g,
                                                                     const float4 *__restrict__ normals, PoseArg P, NlinArgs a,
                                                                     const uint32_t *warm_in, uint32_t *warm_out,
                                                                     double *__restrict__ partials, NlinDump d) {
    __shared__ RunList runs[kLinBlock / kWave];
    __shared__ double gm[kLinBlock / kWave][64];
    __shared__ double cnt[kLinBlock / kWave][2];
    const int wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kLinBlock + threadIdx.x;
    double row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = 0.0;
    uint8_t flag = 0;
    if (i < n_src) {
        const float4 s4 = src[i];
        NlinPoint o;
        flag = nlin_point(g, runs[wave], normals, P, a, s4, warm_in ? warm_in[i] : kNoIdx, row, o);
        if (warm_out) warm_out[i] = o.pos;
        if constexpr (DUMP) {
            const size_t oi = __float_as_uint(s4.w);
            if (d.nn_idx) d.nn_idx[oi] = o.idx == kNoIdx ? -1 : (int32_t)o.idx;
            if (d.nn_d2) d.nn_d2[oi] = o.d2;
            if (d.flag) d.flag[oi] = flag;
            if (d.normal) { d.normal[3 * oi] = o.n[0]; d.normal[3 * oi + 1] = o.n[1]; d.normal[3 * oi + 2] = o.n[2]; }
            if (d.r) d.r[oi] = o.r;
            if (d.s) d.s[oi] = o.s;
            if (d.row) {
#pragma unroll
                for (int j = 0; j < 8; ++j) d.row[8 * oi + j] = row[j];
            }
        }
    }
    nlin_block_rows(row, flag, runs[wave], gm, cnt, partials + (size_t)blockIdx.x * kSlots);
}

// Many poses in one launch.  Block (x, pose): pose = poses[blockIdx.y]; its cloud is slices[pose] = {first point, points} of src (as k_lin's
// SLICE mode reads one; a block past the end of a short frame's slice exits at once) or, slices == null, the n_src points at src.  The
// pose's warm positions: warm + P.state * warm_stride (P.state == kNoIdx: search cold, keep nothing; P.fresh: the array holds nothing
// yet) - a lane reads its word before it writes it, and no other lane's.  The block row goes to partials[pose * n_blocks_x + x], where
// k_finalize<SLICE> finds it: the rows and additions of the pose's single launch.
// GRIDS (scan pairs: dcreg_pairs_normals_batch_begin): every pose also searches a target of its own - grids[grid_ids[pose]], read through a
// block-uniform index, holds its grid, the rings that cover the search bound in its cells and where its kept normals start in `normals`; the
// block takes them before anything else and runs as a slice block against that target (the warm words are then positions in that target's
// sorted points).  The search bound and the gate depend on the radius alone and stay in `a`.
template <bool GRIDS>
static __global__ __launch_bounds__(kLinBlock, kLinOcc) void k_nlin_batch(const float4 *__restrict__ src, uint32_t n_src, GridDev g,
                                                                           const float4 *__restrict__ normals,
                                                                           const PoseArg *__restrict__ poses, const uint2 *__restrict__ slices,
                                                                           NlinArgs a, uint32_t *warm, uint32_t warm_stride,
                                                                           double *__restrict__ partials, uint32_t n_blocks_x,
                                                                           const OneNnGrid *__restrict__ grids, const uint32_t *__restrict__ grid_ids) {
    __shared__ RunList runs[kLinBlock / kWave];
    __shared__ double gm[kLinBlock / kWave][64];
    __shared__ double cnt[kLinBlock / kWave][2];
    const uint32_t pose_id = blockIdx.y;
    if constexpr (GRIDS) {                           // (uniform per block)
        const OneNnGrid &og = grids[grid_ids[pose_id]];
        g = og.g; a.max_ring = og.max_ring; normals += og.normals_first;
    }
    if (slices) {
        uint32_t first;
        if (!batch_slice(slices, first, n_src)) return;
        src += first;
    }
    const PoseArg &P = poses[pose_id];
    const int wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kLinBlock + threadIdx.x;
    double row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = 0.0;
    uint8_t flag = 0;
    if (i < n_src) {
        uint32_t *w = P.state != kNoIdx ? warm + (size_t)P.state * warm_stride + i : nullptr;
        const float4 s4 = src[i];
        NlinPoint o;
        flag = nlin_point(g, runs[wave], normals, P, a, s4, (w && P.fresh == 0u) ? *w : kNoIdx, row, o);
        if (w) *w = o.pos;
    }
    nlin_block_rows(row, flag, runs[wave], gm, cnt, partials + ((size_t)pose_id * n_blocks_x + blockIdx.x) * kSlots);
}

// the launch's arguments for a search within the bound b ("robust_kernel" and "robust_scale" are read at every call)
NlinArgs nlin_args(const dcreg_ctx *c, const OneNnBound &b, const dcreg_lin_params *p) {
    NlinArgs a;
    a.radius_sq = b.radius_sq; a.bound_f = b.bound_f; a.max_ring = b.max_ring;
    a.w_slope = p->weight_slope; a.w_min = p->weight_min; a.use_wd = p->use_weight_derivative;
    a.robust = c->opt_robust_kernel; a.robust_c2 = c->opt_robust_scale * c->opt_robust_scale;
    return a;
}

int nlin_run(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, dcreg_lin_out *out, dcreg_nlin_debug *dbg) {
    NlinDump d{};
    const dcreg_nlin_debug none{}, &h = dbg ? *dbg : none;
    const DumpField fields[] = {{h.normal, 24, &d.normal}, {h.r, 8, &d.r}, {h.s, 8, &d.s}, {h.row, 64, &d.row},
                                     {h.nn_idx, 4, &d.nn_idx}, {h.nn_d2, 4, &d.nn_d2}, {h.flag, 1, &d.flag}};
    return one_nn_run(c, R, t, p, out, "normal", nullptr, [&](const OneNnLaunch &L) {
        const GridDev &g = c->map.grid;
        hipLaunchKernelGGL(L.dump ? k_nlin<true> : k_nlin<false>, dim3(L.nb), dim3(kLinBlock), 0, c->stream, c->d_src.data(), (uint32_t)c->n_src, g,
                           c->nicp.normals.data(), L.P, nlin_args(c, L.bound, p), L.warm_in, L.warm_out, L.partials, d);
    }, dbg != nullptr, fields, 7);
}

// the second engine's kernel for a batched launch (one_nn_batch_begin below)
void nlin_batch_launch(dcreg_ctx *c, const OneNnBatch &L) {
    const NlinArgs a = nlin_args(c, L.bound, L.p);
    hipLaunchKernelGGL(L.grids ? k_nlin_batch<true> : k_nlin_batch<false>, dim3(L.nbx, (unsigned)L.n_poses), dim3(kLinBlock), 0, c->stream, L.src, L.n_src,
                       L.g, L.normals, L.poses, L.slices, a, L.warm, L.warm_stride, L.partials, L.nbx, L.grids, L.grid_ids);
}

}  // namespace

// ---- the batched form (context.hpp NormalIcpBufs::BatchSlot), shared with gicp.hip.  begin: every refusal before anything is queued or
// changed, then the pose upload, the engine's batched kernel (`launch`: k_nlin_batch, k_glin_batch), k_finalize and the copy of the result
// rows to pinned memory on the context's stream, and the slot's event behind them; end waits for that event - never for what the other
// slot queued behind it.  The two launch slots serve the second, third and fourth engine: a pending slot of one refuses the others.
using BatchSlot = dcreg_ctx::NormalIcpBufs::BatchSlot;

// the front of every batched begin's refusals, in the order of include/dcreg_debug.h (context.hpp)
int rows_batch_check(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const dcreg_lin_params *p, bool ids_given, const char *what,
                     bool search) {
    if (!c) return DCREG_E_INVALID;
    if (slot < 0 || slot >= 2) { c->fail("invalid slot %d", slot); return DCREG_E_INVALID; }
    if (!R9 || !t3 || !p || !ids_given || n_poses < 1) { c->fail("null linearisation arguments"); return DCREG_E_INVALID; }
    if (n_poses > 65535) { c->fail("at most 65535 poses per batched launch (grid.y limit), got %d", n_poses); return DCREG_E_INVALID; }
    if (c->gate_slot >= 0) { c->fail("a gated linearisation still waits for its pose (dcreg_linearize_gate_open / _gate_abort first)"); return DCREG_E_STATE; }
    for (const LinSlot &S : c->slots) if (S.pending) { c->fail("a linearisation is still in flight"); return DCREG_E_STATE; }
    if (c->nicp.batch[slot].pending) { c->fail("slot %d still has a batched normal linearisation in flight", slot); return DCREG_E_STATE; }
    if (p->parameterization != DCREG_PARAM_SO3) { c->fail("the %s linearisation has the SO(3) row only (parameterization %d)", what, p->parameterization); return DCREG_E_INVALID; }
    if (search && !(std::isfinite(p->search_radius) && p->search_radius > 0.0)) { c->fail("search_radius is %g: finite and > 0 expected", p->search_radius); return DCREG_E_INVALID; }
    if (!finite_n(R9, 9 * (int64_t)n_poses) || !finite_n(t3, 3 * (int64_t)n_poses)) { c->fail("a pose is not finite"); return DCREG_E_INVALID; }
    return DCREG_OK;
}

// the clouds of a batched launch and the points of the largest (context.hpp)
int rows_batch_clouds(dcreg_ctx *c, const dcreg_ctx::FrameSet *fs, int n_poses, const int32_t *ids, const char *noun,
                      const std::function<int(int)> &pose_check, int64_t &n_max) {
    n_max = c->n_src;
    if (!fs) {
        if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
        return DCREG_OK;
    }
    const std::vector<uint2> &slice = fs->slice;
    if (slice.empty()) { c->fail(fs == &c->pair_src ? "no pair sources: dcreg_pairs_sources_load first" : "no frames: dcreg_frames_load first"); return DCREG_E_STATE; }
    n_max = 0;
    for (int i = 0; i < n_poses; ++i) {
        const int32_t f = ids[i];
        if (f < 0 || (size_t)f >= slice.size() || slice[(size_t)f].y == 0u) { c->fail("%s %d is not loaded or empty", noun, f); return DCREG_E_INVALID; }
        if (pose_check) if (int rc = pose_check(i)) return rc;
        n_max = std::max<int64_t>(n_max, slice[(size_t)f].y);
    }
    return DCREG_OK;
}

int one_nn_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids, dcreg_ctx::FrameSet *fs,
                       const int32_t *frame_ids, const int32_t *target_ids, const dcreg_lin_params *p,
                       int (*extra)(dcreg_ctx *, const dcreg_ctx::FrameSet *fs), void (*launch)(dcreg_ctx *, const OneNnBatch &), const char *kernel_name) {
    if (!c) return DCREG_E_INVALID;
    dcreg_ctx::NormalIcpBufs &B = c->nicp;
    using SlotsFor = dcreg_ctx::NormalIcpBufs::SlotsFor;
    if (!frame_ids) fs = nullptr;
    const bool pairs = fs == &c->pair_src;
    if (pairs != (target_ids != nullptr)) { c->fail("pair launches name a source and a target for every pose"); return DCREG_E_INVALID; }
    const SlotsFor slots_for = pairs ? SlotsFor::pairs : fs ? SlotsFor::frames : SlotsFor::source;
    if (int rc = rows_batch_check(c, slot, n_poses, R9, t3, p, true, "normal", true)) return rc;   // ("normal" for the third engine too)
    const dcreg_ctx::PairSet &ps = c->pairs;
    if (pairs) {
        if (ps.n <= 0) { c->fail("no pair batch built: dcreg_pairs_build first"); return DCREG_E_STATE; }
        if (!ps.normals_kept) { c->fail("no kept pair normals: dcreg_pairs_normals_keep or dcreg_pairs_normals_set first"); return DCREG_E_STATE; }
        if (p->search_radius != ps.search_radius) { c->fail("the pair targets were built for another search radius"); return DCREG_E_INVALID; }
        for (int i = 0; i < n_poses; ++i) {
            const int32_t t = target_ids[i];
            if (t < 0 || t >= ps.n || !ps.built[(size_t)t]) { c->fail("pair target %d is not built", t); return DCREG_E_INVALID; }
        }
    } else {
        if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
        if (!B.kept) { c->fail("no kept normals: dcreg_target_normals_keep or dcreg_target_normals_set first"); return DCREG_E_STATE; }
    }
    int64_t n_max;                                    // (every target above before any source: "frame %d" names a pair source too)
    if (int rc = rows_batch_clouds(c, fs, n_poses, frame_ids, "frame", nullptr, n_max)) return rc;
    if (extra) if (int rc = extra(c, fs)) return rc;
    if (state_ids) {
        std::vector<uint8_t> seen((size_t)std::max<int64_t>(B.n_slots, 1), 0);
        for (int i = 0; i < n_poses; ++i) {
            const int32_t sid = state_ids[i];
            if (sid < 0) continue;
            if ((int64_t)sid >= B.n_slots) { c->fail("warm slot %d was not reserved (dcreg_normals_reserve_slots: %lld)", sid, (long long)B.n_slots); return DCREG_E_INVALID; }
            if (seen[(size_t)sid]) { c->fail("warm slot %d is used by two poses of one launch", sid); return DCREG_E_INVALID; }
            if (B.slots_for != slots_for || (int64_t)B.slot_stride < n_max) {
                c->fail("the warm slots were reserved for other clouds (dcreg_normals_reserve_slots again)"); return DCREG_E_INVALID;
            }
            seen[(size_t)sid] = 1;
        }
    }
    // the whole map's index, wherever it lives (context.hpp roi_store): the window index stays as it is, active or not
    const dcreg_ctx::IndexSet &whole = c->roi_active ? c->roi_store : c->map;
    return rows_batch_queue(c, slot, n_poses, R9, t3, state_ids, fs, frame_ids, target_ids, n_max, [&](OneNnBatch &L) {
        L.g = pairs ? GridDev{} : whole.grid; L.normals = pairs ? ps.normals.data() : B.normals.data();
        L.grids = pairs ? ps.d_nn_grids.data() : nullptr;
        GridDev bound_grid = whole.grid;
        if (pairs) bound_grid.h = p->search_radius;                 // (the rings come with every pose's target: only the radius' part is used)
        L.bound = one_nn_bound(bound_grid, p->search_radius);
        L.warm = B.slots.data(); L.warm_stride = (uint32_t)B.slot_stride;
        L.p = p;
        launch(c, L);
    }, kernel_name);
}

// The slot plumbing of a batched launch, behind the engine's refusals (context.hpp): the slot's buffers sized for the largest cloud, the
// pinned pose and slice block and its upload, the engine's kernel (`launch` completes the record and queues it), k_finalize, the result copy
// and the slot's event.  n_max: the points of the launch's largest cloud.  A failure once something may be queued marks the launch's warm
// slots empty.
int rows_batch_queue(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids, dcreg_ctx::FrameSet *fs,
                     const int32_t *frame_ids, const int32_t *target_ids, int64_t n_max, const std::function<void(OneNnBatch &)> &launch,
                     const char *kernel_name) {
    dcreg_ctx::NormalIcpBufs &B = c->nicp;
    BatchSlot &S = B.batch[slot];
    const bool pairs = target_ids != nullptr;
    static const std::vector<uint2> no_slices;
    const std::vector<uint2> &slice = fs ? fs->slice : no_slices;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t nbx = (uint32_t)((n_max + kLinBlock - 1) / kLinBlock);
    const size_t np = (size_t)n_poses, pose_bytes = np * sizeof(PoseArg), slice_bytes = frame_ids ? np * sizeof(uint2) : 0,
                 bytes = pose_bytes + slice_bytes + (pairs ? np * sizeof(uint32_t) : 0);
    // (sized for the call's largest cloud and for what the slot has held: the engine's launches stop growing them after the first)
    const int64_t cloud_max = fs ? fs->max_points : c->n_src;
    const size_t rows_cap = std::max(np, S.d_out.cap() / kSlots) * (size_t)((cloud_max + kLinBlock - 1) / kLinBlock) * kSlots;
    if (S.partials.ensure(c, std::max(rows_cap, np * nbx * kSlots)) || S.d_out.ensure(c, np * kSlots)) return DCREG_E_NOMEM;
    if (S.h_out.cap() < np * kSlots) HIP_TRY(c, S.h_out.alloc(std::max<size_t>(np, 256) * kSlots, hipHostMallocDefault));
    if (bytes > S.d_poses.cap()) {
        const size_t cap = std::max<size_t>(bytes, 256 * (sizeof(PoseArg) + sizeof(uint2) + sizeof(uint32_t)));
        HIP_TRY(c, S.h_poses.alloc(cap, hipHostMallocDefault));
        if (S.d_poses.ensure(c, cap)) return DCREG_E_NOMEM;
    }
    if (!S.done) HIP_TRY(c, hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    const bool use_slots = state_ids && c->opt_warm;
    PoseArg *hp = (PoseArg *)S.h_poses.data();
    S.ids.clear();
    for (int i = 0; i < n_poses; ++i) {
        std::memcpy(hp[i].R, R9 + 9 * i, sizeof(hp[i].R)); std::memcpy(hp[i].t, t3 + 3 * i, sizeof(hp[i].t));
        const bool has = use_slots && state_ids[i] >= 0;
        hp[i].state = has ? (uint32_t)state_ids[i] : kNoIdx;
        hp[i].fresh = (has && B.slot_valid[(size_t)state_ids[i]] != 0) ? 0u : 1u;
        if (has) { B.slot_valid[(size_t)state_ids[i]] = 1; S.ids.push_back(state_ids[i]); }
    }
    const uint2 *d_slices = nullptr;
    if (frame_ids) {
        uint2 *hs = (uint2 *)(S.h_poses.data() + pose_bytes);
        for (int i = 0; i < n_poses; ++i) hs[i] = slice[(size_t)frame_ids[i]];
        d_slices = (const uint2 *)(S.d_poses.data() + pose_bytes);
    }
    const uint32_t *d_grid_ids = nullptr;
    if (pairs) {
        std::memcpy(S.h_poses.data() + pose_bytes + slice_bytes, target_ids, np * sizeof(uint32_t));
        d_grid_ids = (const uint32_t *)(S.d_poses.data() + pose_bytes + slice_bytes);
    }
    auto failed = [&](hipError_t e, const char *what) {          // something may be queued: what it leaves in the slots is unknown
        for (int32_t sid : S.ids) B.slot_valid[(size_t)sid] = 0;
        c->fail("%s failed: %s", what, hipGetErrorString(e));
        return DCREG_E_DEVICE;
    };
    hipError_t e = hipMemcpyAsync(S.d_poses.data(), S.h_poses.data(), bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return failed(e, "the pose upload");
    OneNnBatch L{};
    L.src = fs ? fs->src.data() : c->d_src.data(); L.n_src = (uint32_t)c->n_src;
    L.src_normals = fs ? fs->normals.data() : c->gicp.src_normals.data();
    L.grid_ids = d_grid_ids;
    L.poses = (const PoseArg *)S.d_poses.data(); L.slices = d_slices;
    L.partials = S.partials.data(); L.nbx = nbx; L.n_poses = n_poses;
    launch(L);
    if ((e = hipGetLastError()) != hipSuccess) return failed(e, kernel_name);
    if (frame_ids) hipLaunchKernelGGL(k_finalize<true>, dim3((unsigned)n_poses), dim3(kLinBlock), 0, c->stream, S.partials.data(), nbx, S.d_out.data(), 0ull, d_slices);
    else hipLaunchKernelGGL(k_finalize<false>, dim3((unsigned)n_poses), dim3(kLinBlock), 0, c->stream, S.partials.data(), nbx, S.d_out.data(), 0ull, (const uint2 *)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return failed(e, "the k_finalize launch");
    if ((e = hipMemcpyAsync(S.h_out.data(), S.d_out.data(), np * kSlots * sizeof(double), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return failed(e, "the result copy");
    if ((e = hipEventRecord(S.done, c->stream)) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);                    // (no event to wait for: nothing of this launch stays in flight)
        return failed(e, "hipEventRecord");
    }
    S.n_poses = n_poses;
    S.pending = true;
    return DCREG_OK;
}

int rows_batch_end(dcreg_ctx *c, int slot, dcreg_lin_out *outs) {
    if (!c) return DCREG_E_INVALID;
    if (slot < 0 || slot >= 2) { c->fail("invalid slot %d", slot); return DCREG_E_INVALID; }
    BatchSlot &S = c->nicp.batch[slot];
    if (!S.pending) { c->fail("slot %d has no batched normal linearisation in flight", slot); return DCREG_E_STATE; }
    if (!outs) { c->fail("null argument"); return DCREG_E_INVALID; }
    S.pending = false;
    const hipError_t e = hipEventSynchronize(S.done);
    if (e != hipSuccess) {
        c->nicp.drop_slots();                                     // what the launch left in the slots is unknown
        c->fail("device fault while waiting for a batched normal linearisation: %s", hipGetErrorString(e));
        return DCREG_E_DEVICE;
    }
    for (int i = 0; i < S.n_poses; ++i) lin_out_of_row(S.h_out.data() + (size_t)i * kSlots, outs[i]);
    return DCREG_OK;
}

// ---- shared with gicp.hip (context.hpp)
int one_nn_check(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, const dcreg_lin_out *out, const char *what) {
    if (!c) return DCREG_E_INVALID;
    if (!R || !t || !p || !out) { c->fail("null linearisation arguments"); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    if (p->parameterization != DCREG_PARAM_SO3) { c->fail("the %s linearisation has the SO(3) row only (parameterization %d)", what, p->parameterization); return DCREG_E_INVALID; }
    if (!(std::isfinite(p->search_radius) && p->search_radius > 0.0)) { c->fail("search_radius is %g: finite and > 0 expected", p->search_radius); return DCREG_E_INVALID; }
    if (!finite_n(R, 9) || !finite_n(t, 3)) { c->fail("the pose is not finite"); return DCREG_E_INVALID; }
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    if (c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    if (!c->nicp.kept) { c->fail("no kept normals: dcreg_target_normals_keep or dcreg_target_normals_set first"); return DCREG_E_STATE; }
    return DCREG_OK;
}
// The single-pose runner of both 1-NN engines (context.hpp): what belongs to the search, in front of rows_run.  The engine's kernel searches
// the index roi_ensure made the active one; a debug launch searches cold and keeps no positions, a plain one starts from the warm words
// and leaves its own there.
int one_nn_run(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, dcreg_lin_out *out, const char *what,
               int (*extra)(dcreg_ctx *, const dcreg_ctx::FrameSet *fs), const std::function<void(const OneNnLaunch &)> &launch, bool dump,
               const DumpField *fields, int n_fields) {
    if (int rc = one_nn_check(c, R, t, p, out, what)) return rc;
    if (extra) if (int rc = extra(c, nullptr)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // the index a single-pose linearisation searches: the window of a capped map, as dcreg_linearize (a swap drops the warm positions)
    if (int rc = roi_ensure(c, R, t, p->search_radius)) return rc;
    if (one_nn_warm_reserve(c)) return DCREG_E_NOMEM;
    OneNnLaunch L;
    L.bound = one_nn_bound(c->map.grid, p->search_radius);
    std::memcpy(L.P.R, R, sizeof(L.P.R)); std::memcpy(L.P.t, t, sizeof(L.P.t));
    L.P.state = kNoIdx; L.P.fresh = 1;
    L.dump = dump;
    const int rc = rows_run(c, out, fields, dump ? n_fields : 0, [&](double *partials, uint32_t nb) {
        L.warm_in = dump ? nullptr : one_nn_warm_take(c);
        L.warm_out = dump ? nullptr : c->nicp.warm.data();
        L.partials = partials; L.nb = nb;
        launch(L);
    });
    if (rc == DCREG_OK && !dump) one_nn_warm_done(c);
    return rc;
}
// The back half of every single-pose call that leaves block rows (context.hpp): all three engines end here
int rows_run(dcreg_ctx *c, dcreg_lin_out *out, const DumpField *fields, int n_fields, const std::function<void(double *partials, uint32_t nb)> &launch) {
    dcreg_ctx::NormalIcpBufs &B = c->nicp;
    const size_t N = (size_t)c->n_src;
    const uint32_t nb = (uint32_t)((N + kLinBlock - 1) / kLinBlock);
    if (B.partials.ensure(c, (size_t)nb * kSlots) || B.d_out.ensure(c, kSlots)) return DCREG_E_NOMEM;
    // one block of device memory for the dump, cut into its arrays in the table's order (8-byte ones first)
    size_t total = 0;
    for (int k = 0; k < n_fields; ++k) total += fields[k].bytes * N;
    if (n_fields && B.dbg.ensure(c, total)) return DCREG_E_NOMEM;
    unsigned char *b = B.dbg.data();
    for (int k = 0; k < n_fields; b += fields[k++].bytes * N)
        if (fields[k].host) std::memcpy(fields[k].dev, &b, sizeof(b));
    launch(B.partials.data(), nb);
    HIP_TRY(c, hipGetLastError());
    b = B.dbg.data();
    for (int k = 0; k < n_fields; b += fields[k++].bytes * N)
        if (fields[k].host) HIP_TRY(c, hipMemcpyAsync(fields[k].host, b, fields[k].bytes * N, hipMemcpyDeviceToHost, c->stream));
    hipLaunchKernelGGL(k_finalize<false>, dim3(1), dim3(kLinBlock), 0, c->stream, B.partials.data(), nb, B.d_out.data(), 0ull, (const uint2 *)nullptr);
    HIP_TRY(c, hipGetLastError());
    double row[kSlots];
    HIP_TRY(c, hipMemcpyAsync(row, B.d_out.data(), sizeof(row), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    lin_out_of_row(row, *out);
    return DCREG_OK;
}
OneNnBound one_nn_bound(const GridDev &g, double search_radius) {
    OneNnBound b;
    b.radius_sq = search_radius * search_radius;
    float bound = (float)b.radius_sq;
    if ((double)bound < b.radius_sq) bound = std::nextafterf(bound, __builtin_inff());     // the smallest float >= R^2
    if (!(bound <= 3.0e38f)) bound = 3.0e38f;
    b.bound_f = bound;
    b.max_ring = rings_for_bound(g, bound);
    return b;
}
int one_nn_warm_reserve(dcreg_ctx *c) {
    dcreg_ctx::NormalIcpBufs &B = c->nicp;
    if (!B.warm.holds((size_t)c->n_src)) B.warm_valid = false;          // (a new array holds nothing)
    return B.warm.ensure(c, (size_t)c->n_src) ? DCREG_E_NOMEM : DCREG_OK;
}
const uint32_t *one_nn_warm_take(dcreg_ctx *c) {
    dcreg_ctx::NormalIcpBufs &B = c->nicp;
    const bool warm = c->opt_warm && B.warm_valid;
    B.warm_valid = false;                 // (until the launch is known to have run)
    return warm ? B.warm.data() : nullptr;
}
void one_nn_warm_done(dcreg_ctx *c) { c->nicp.warm_valid = true; }
// the warm slots of the batched form: n_slots arrays sized for the largest cloud of `what` (nothing is reserved without such a cloud)
int one_nn_reserve_slots(dcreg_ctx *c, int64_t n_slots, dcreg_ctx::NormalIcpBufs::SlotsFor what) {
    using SlotsFor = dcreg_ctx::NormalIcpBufs::SlotsFor;
    if (n_slots < 0) { c->fail("negative slot count"); return DCREG_E_INVALID; }
    if (int rc = refuse_in_flight(c)) return rc;
    dcreg_ctx::NormalIcpBufs &B = c->nicp;
    B.n_slots = 0; B.slot_valid.clear(); B.slot_stride = 0;
    B.slots_for = what;
    const int64_t points = what == SlotsFor::pairs ? c->pair_src.max_points : what == SlotsFor::frames ? c->frames.max_points : c->n_src;
    if (n_slots == 0 || points <= 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t stride = ((size_t)points + 63) & ~(size_t)63;
    // nothing is cleared: a slot is "fresh" (host-side flag) until its first launch has filled it
    if (B.slots.ensure(c, stride * (size_t)n_slots)) return DCREG_E_NOMEM;
    B.slot_stride = stride;
    B.n_slots = n_slots;
    B.slot_valid.assign((size_t)n_slots, 0);
    return DCREG_OK;
}

}  // namespace dcreg

using namespace dcreg;

extern "C" {
int dcreg_linearize_normals(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out) {
    return nlin_run(c, R, t, p, out, nullptr);
}
int dcreg_linearize_normals_debug(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out,
                                  dcreg_nlin_debug *dbg) {
    if (c && !dbg) { c->fail("null dump"); return DCREG_E_INVALID; }
    return nlin_run(c, R, t, p, out, dbg);
}
int dcreg_normals_reserve_slots(dcreg_ctx *c, int64_t n_slots, int frames) {
    using SlotsFor = dcreg_ctx::NormalIcpBufs::SlotsFor;
    return c ? one_nn_reserve_slots(c, n_slots, frames ? SlotsFor::frames : SlotsFor::source) : DCREG_E_INVALID;
}
int dcreg_pairs_normals_reserve_slots(dcreg_ctx *c, int64_t n_slots) {
    return c ? one_nn_reserve_slots(c, n_slots, dcreg_ctx::NormalIcpBufs::SlotsFor::pairs) : DCREG_E_INVALID;
}
int dcreg_pairs_normals_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                                    const int32_t *source_ids, const int32_t *target_ids, const dcreg_lin_params *p) {
    if (c && (!source_ids || !target_ids)) { c->fail("null argument"); return DCREG_E_INVALID; }
    return one_nn_batch_begin(c, slot, n_poses, R9, t3, state_ids, c ? &c->pair_src : nullptr, source_ids, target_ids, p, nullptr, nlin_batch_launch,
                              "the k_nlin_batch launch");
}
int dcreg_normals_reset_slot(dcreg_ctx *c, int64_t slot_id) {
    if (!c) return DCREG_E_INVALID;
    if (slot_id < 0 || slot_id >= c->nicp.n_slots) { c->fail("warm slot %lld was not reserved", (long long)slot_id); return DCREG_E_INVALID; }
    c->nicp.slot_valid[(size_t)slot_id] = 0;
    return DCREG_OK;
}
int dcreg_normals_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                              const int32_t *frame_ids, const dcreg_lin_params *p) {
    return one_nn_batch_begin(c, slot, n_poses, R9, t3, state_ids, c ? &c->frames : nullptr, frame_ids, nullptr, p, nullptr, nlin_batch_launch,
                              "the k_nlin_batch launch");
}
int dcreg_normals_batch_end(dcreg_ctx *c, int slot, dcreg_lin_out *outs) { return rows_batch_end(c, slot, outs); }
}
