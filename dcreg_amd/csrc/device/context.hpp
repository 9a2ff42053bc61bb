// dcreg_ctx: device state behind the C-ABI.  Stands for ICPContext (DCReg/include/utils.hpp:340-425):
// the kd-tree becomes a cell-sorted target + cell table in HBM, the per-point scratch vectors become
// nothing at all (the row of every point lives in registers and is reduced on the fly).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/dcreg.h"
#include "kernels.hpp"
#include "align.hpp"

struct dcreg_lin_params;
struct dcreg_lin_out;
struct dcreg_lin_debug;

#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            (ctx)->fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return DCREG_E_DEVICE;                                                               \
        }                                                                                        \
    } while (0)

// A device buffer (hipMalloc) that owns its memory: move-only, freed by its destructor.  No conversion to T*: a kernel argument is
// written .data(), so a buffer object is never handed to a launch by value.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~DevBuf() { reset(); }
    T *data() const { return p_; }
    size_t cap() const { return cap_; }                 // elements
    explicit operator bool() const { return p_ != nullptr; }
    bool holds(size_t need) const { return p_ && need <= cap_; }
    void swap(DevBuf &o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    // frees what it holds, then allocates exactly n elements (the caller reports a failure)
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void **)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = n;
        return e;
    }
    // at least `need` elements, contents not kept: freed, then max(need, 1) allocated.  why != null: the failure's text names the caller
    int ensure(dcreg_ctx *c, size_t need, const char *why = nullptr);
    // at least `need` elements of which the first `keep` survive: allocated first (geometric capacity), the copy queued on c->stream and
    // waited for, then the old buffer freed
    int grow_keep(dcreg_ctx *c, size_t need, size_t keep);
private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// Pinned host memory (hipHostMalloc) that owns its block, as DevBuf; a block allocated hipHostMallocMapped also has its device address.
template <typename T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept { swap(o); }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~PinnedBuf() { reset(); }
    T *data() const { return p_; }
    T *dev() const { return d_; }                       // device address of a mapped block (null otherwise)
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    void swap(PinnedBuf &o) noexcept { std::swap(p_, o.p_); std::swap(d_, o.d_); std::swap(cap_, o.cap_); }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = d_ = nullptr; cap_ = 0; }
    // frees what it holds, then allocates n elements with these flags (capacity n once the block and its device address exist)
    hipError_t alloc(size_t n, unsigned flags) {
        reset();
        hipError_t e = hipHostMalloc((void **)&p_, n * sizeof(T), flags);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer((void **)&d_, p_, 0);
        if (e == hipSuccess) cap_ = n;
        return e;
    }
private:
    T *p_ = nullptr, *d_ = nullptr;
    size_t cap_ = 0;
};

namespace dcreg {
// one cloud of a deskew call on the device (deskew.hip k_pack_deskew): twist xi = Log(motion) (w then v), span, reference instant
struct DeskewCloud {
    double xi[6];
    double t_begin, t_end, ref;
    int from_data;                 // the span is the cloud's own minimum / maximum finite stamp (keys of k_deskew_span)
    int pad_;
};
// one cloud of a path deskew on the device (deskew.hip k_pack_deskew_path): its segment records segs[first_seg .. first_seg + n_seg), the
// first and last stamp of its knot window, and the extrinsic E = (R row-major, t)
struct PathCloud {
    int64_t first_seg;
    int n_seg;
    int pad_;
    double s_first, s_last;
    double E[12];
};
// one (cloud, segment) record: the segment's twist xi_k (w then v), G_k = E^-1 B(t_ref)^-1 P_k (R row-major, t), its first stamp and length
struct PathSeg {
    double xi[6];
    double G[12];
    double s0, len;
};
// one non-empty member of a keyframe gather on the device (keyframes.hip k_kf_gather): its first output point, its first point in the
// store, and its pose (R row-major, t) - 104 B
struct KfMember {
    uint32_t start, src;
    double pose[12];
};
// one non-empty member of a visibility batch on the device (visibility.hip k_vis_image, k_vis_vote): its first point among the batch's
// stored points, its first point in the store, its range image within the batch, and its pose (R row-major, t) - 112 B
struct VisMember {
    uint32_t start, src, img, pad_;
    double pose[12];
};
// the cloud of point i: the largest s with off[s] <= i (off[n_clouds] > i) - the segments of voxel.hip and deskew.hip
__device__ __forceinline__ uint32_t seg_of(const int64_t *__restrict__ off, int n_clouds, int64_t i) {
    int lo = 0, hi = n_clouds;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return (uint32_t)lo;
}
// blocks of bs threads that cover n items
inline unsigned blocks(int64_t n, int64_t bs) { return (unsigned)((n + bs - 1) / bs); }
// a packed point / three coordinates are finite: the rule of every pass over a caller's cloud (at most FLT_MAX in magnitude).  NOT
// kernels.hpp's finite3 of the map-insert path, whose bound is 3.4e38f: the two differ for values in (3.4e38, FLT_MAX]
__device__ __forceinline__ bool finite_xyz(float x, float y, float z) {
    return fabsf(x) <= 3.4028235e38f && fabsf(y) <= 3.4028235e38f && fabsf(z) <= 3.4028235e38f;
}
__device__ __forceinline__ bool finite_point(const float4 p) {
    return fabsf(p.x) <= 3.4028235e38f && fabsf(p.y) <= 3.4028235e38f && fabsf(p.z) <= 3.4028235e38f;
}
}  // namespace dcreg

namespace dcreg {
// the target of one scan pair as the batched 1-NN launches read it (normal_icp.hip k_nlin_batch<GRIDS>, gicp.hip k_glin_batch<GRIDS>): its
// grid, the rings that cover the 1-NN search bound in its cells, and where its kept normals start among the build batch's
struct OneNnGrid {
    GridDev g;
    int max_ring;
    uint32_t normals_first;
};
// the target of one scan pair as the fourth engine's pairs launch reads it (voxel_icp.hip k_vlin_pairs): the build batch's kept records,
// keys and lookup tables lie target after target (voxel.hip pairs_voxels_build); this target's records start at record `first`, its own
// table - mask + 1 slots, the values record numbers within the target - at slot `base`; mn / mx: the voxel box of all its points.
// n_kept == 0: no member, nothing else is read.  The leaf is the batch's
struct PairVoxMap {
    uint32_t first, base, mask, n_kept;
    long long mn[3], mx[3];
};
}  // namespace dcreg

// What a linearisation launch is and how it is carried out (context.hip linearize_begin: lin_check settles the kind, lin_plan the rest)
enum class LinKind : uint8_t { batch, frames, pairs, single, gated, dump, stamps };   // single .. stamps: one pose on the ctx's own source
enum class LinPass : uint8_t { none, advance, team };     // in front of k_lin: nothing, k_advance, k_advance_team (dcreg_launch_series_passes)
enum class LinBody : uint8_t { chunked, fused, one_wave, gated, dump, stamps };   // the k_lin instantiation (context.hip lin_kernel)
struct LinPlan {
    LinKind kind = LinKind::single; LinPass pass = LinPass::none; LinBody body = LinBody::fused;
    int n_poses = 0; uint32_t nbx = 0, n_chunks = 0;    // query blocks per pose, chunks of kChunk of them
    size_t n_rows = 0;                 // result rows the host waits for
    bool direct = false;               // the rows are block rows of one chunk (kernels.hpp FinArgs::direct)
    bool gate_inside = false;          // the gated launch waits for its pose in its first kernel (kernels.hpp gate_wait)
    bool pass_rows = false;            // the advance pass builds the rows and finishes the launch itself: no k_lin behind it (k_advance ROWS)
    bool ordered = false, use_cert = true;   // heavy query-block groups first (LinArgs::n_groups); certificates in use (LinArgs::use_cert)
    bool five = false;                 // a five-neighbour launch (kernels.hpp k_lin FIVE; context.hip lin_plan has the rule)
    bool fused() const { return body != LinBody::chunked; }     // the kernels sum and publish per pose (no k_finalize)
    bool one_wave() const { return body == LinBody::one_wave; }
    int passes() const { return (int)pass | (one_wave() ? 4 : 0); }   // dcreg_launch_series_passes: + 4 = k_lin ran in one-wave blocks
    int structure() const { return (pass_rows ? 2 : pass != LinPass::none ? 1 : 0) | (five ? 4 : 0); }   // dcreg_launch_series_structure
};

// buffers and in-flight state of one linearisation slot
struct LinSlot {
    DevBuf<double> d_partials;
    // batched poses: ONE pinned staging block [PoseArg x n | pose ids x n] and its device copy (one plain DMA per launch; a pageable
    // source is staged by the runtime, and beyond 16 KB that cost 14 us per launch)
    PinnedBuf<unsigned char> h_poses;
    DevBuf<unsigned char> d_poses;
    PinnedBuf<double> h_out;       // pinned, device-mapped result rows
    std::vector<double> h_rows;    // ... and the checked snapshot of them the sums are taken from
    DevBuf<unsigned int> d_tickets;
    bool tickets_dirty = false;    // a launch may have died half-way: clear the tickets before the next one
    std::vector<DevBuf<unsigned char>> tmp_dev;   // debug dump buffers of the launch in flight
    bool pending = false, timed = false, sync = false;
    LinPlan plan;                  // of the launch in flight
    std::vector<uint8_t> row_done; // wait_rows: rows taken so far
    std::vector<unsigned long long> row_chk;   // ... and the check word each row carried when it was last taken
    unsigned long long seq = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // "time_kernels": the events of this slot's launch (the two slots alternate in a pipelined run)
    bool coded = false;            // the launch in flight reports searched / refitted counts above its count slots (LinArgs::count_scale)
};

struct dcreg_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    char err[512] = {0};

    // a spatial index over a cloud (context.hip build_index): its points in original and in cell order, the cell table, the grid, and the
    // empty-space field, its owners and the row words of the grid (build_gap_field, build_row_words)
    struct IndexSet {
        DevBuf<float4> raw; int64_t n = 0;
        DevBuf<float4> sorted;
        DevBuf<uint32_t> cell_start;
        dcreg::GridDev grid{}; int64_t n_cells = 0; uint32_t occupied = 0;
        DevBuf<uint8_t> gap;
        DevBuf<uint32_t> owner, ymask;
    };
    // target: the ACTIVE index, the one every kernel launch uses (the whole map, or its window: see roi_store below)
    IndexSet map;
    // counts every event after which a pointer into some index's sorted points may show other points: a build of any index (context.hip
    // build_grid_at: the map, its window, the cloud scratch index, the source's grid), a change of the map (map_merge, map_changed) and a
    // change of the active index (swap_index).  The descriptor reports remember it beside their pointer (FeatureBufs::last_epoch)
    uint64_t index_epoch = 0;
    double radius_hint = 0.0;
    int last_max_ring = 0;
    // ---- updates of the map in place (context.hip map_insert / map_crop: dcreg_target_insert*, dcreg_target_crop).  The new sorted points
    // and cell table, and the raw points of a crop, are built beside the current arrays (map_alt: raw, sorted, cell_start, grid) and swapped
    // in at the end; tgt_box = bounds of the map's points
    IndexSet map_alt;
    DevBuf<float4> d_map_q, d_map_new;                   // the offered points in the map frame / the appended ones
    DevBuf<uint32_t> d_upd;                              // flags, scans, keys of an update
    DevBuf<uint8_t> d_fgap;                              // the fields over the box of a change (k_gap_init_box): plain and dense
    DevBuf<uint32_t> d_fown;
    double tgt_box[6] = {};
    double build_per_cell = 0.0;   // points per occupied cell when the grid was last derived (a merge that doubles it re-derives)
    int opt_map_update = 1;        // 1: merge into the current grid where possible, 0: always re-derive the grid
    int opt_normals_follow = 0;    // "normals_follow": 1 = an update refits the kept normals of dcreg_target_normals_keep instead of dropping them
    double opt_normals_follow_full_share = 0.25;   // "normals_follow_full_share": past this share of dirty points a followed update recomputes everything
    double opt_map_grow_margin = 20.0;   // metres added to each side of the box when an update re-derives the grid

    // ---- the WINDOW index of a large map (context.hip roi_ensure).  A prior map whose dense cell table would exceed "max_table_entries" gets
    // coarser cells the larger its extent - a local search then pays for the size of the map.  Single-pose linearisations of such a map
    // therefore search a second index built over the points of a BOX around the transformed source (its bounding box at the pose, the search
    // radius, "roi_margin" metres on top): the same points as the whole map holds there, in cells sized for their density alone.  Every
    // neighbour of every query lies inside the box, so the searches return what they would on the whole map (exact: the sums are bitwise the
    // same, tests/test_gpu_round6.py); a pose that leaves the box rebuilds the window around itself.  One of the two indices is ACTIVE (map:
    // what every kernel launch uses), the other is kept in roi_store; swapping them drops the neighbour states (their positions refer to
    // one index's sorted order).  Everything but the single-pose product launches (k-NN, metrics, batches, dumps, the kd-tree comparator)
    // runs on the whole map.
    IndexSet roi_store;            // the index that is NOT active
    bool roi_active = false;       // map holds the window, roi_store the whole map
    bool roi_built = false;        // a window exists for the box roi_lo .. roi_hi
    bool roi_empty = false;        // ... but the map has no point in it: the whole map serves inside this box
    int opt_roi_index = 1;         // 0 never, 1 when the whole map's build ran into the table budget, 2 always
    double opt_roi_margin = 20.0;  // metres of the box beyond what the first pose needs
    bool whole_capped = false;     // the whole map's build enlarged its cells or dropped x sub-cells for the table budget
    bool last_build_capped = false;
    double roi_lo[3] = {}, roi_hi[3] = {}, roi_pad = 0.0;
    double src_mn[3] = {}, src_mx[3] = {};      // bounding box of the source in the body frame (dcreg_set_source)
    int64_t roi_rebuilds = 0;

    // auxiliary grid over the body-frame source (backward pass of dcreg_p2p_error): sorted, cell_start, grid, n_cells (the raw points are d_src_raw)
    IndexSet aux;
    bool aux_valid = false;

    // source
    int64_t n_src = 0;
    DevBuf<float4> d_src_raw;
    DevBuf<float4> d_src;                                  // Hilbert-sorted
    // neighbour state of the ctx's own single-pose launches (search.hpp kStateRows): [kStateRows][state_stride]
    DevBuf<uint32_t> d_state;
    size_t state_stride = 0;
    bool state_valid = false;      // the state holds the results of a search of the current clouds
    // What the states hold was measured against the parameters of the launch that wrote it: certificates against the search / gate
    // radii, the stored gate bits against the plane thresholds, the stored plane by one of the two fits.  A launch with another key
    // finds the states empty (linearize_begin); the weights, the weight derivative and the parameterisation are not part of it
    // (they enter after the stored plane).  One key for the ctx's own state and one for the batch states.
    struct StateKey {
        double radius_sq = -1.0, max_thick_sq = 0.0, min_norm = 0.0;
        float radius_sq_f = 0.f, cert_r_out = 0.f, cert_r_in = 0.f;
        int fast_plane = -1;
        bool operator==(const StateKey &o) const {
            return radius_sq == o.radius_sq && max_thick_sq == o.max_thick_sq && min_norm == o.min_norm && radius_sq_f == o.radius_sq_f &&
                   cert_r_out == o.cert_r_out && cert_r_in == o.cert_r_in && fast_plane == o.fast_plane;
        }
    };
    StateKey state_key, batch_state_key;
    double src_radius = 0.0;       // largest distance of a source point from the body-frame origin (bounds a pose change's effect)
    // batched launches: n_batch_states states of the same layout, [state][kStateRows][state_batch_stride] (dcreg_reserve_warm_states),
    // and whether each holds anything yet
    DevBuf<uint32_t> d_state_batch;
    size_t state_batch_stride = 0;
    int64_t n_batch_states = 0;
    std::vector<uint8_t> batch_state_valid;
    // The frames of dcreg_register_frames (engine.cpp): many source clouds beside the ctx's own, registered against the same map.  Every
    // frame in the curve order dcreg_set_source would give it, starting on a query-block boundary; the launches of the call read each
    // pose's frame through its slice (kernels.hpp k_lin SLICE) and keep their neighbour states here - the ctx's own source, its own state
    // and its reserved batch states are not touched.
    struct FrameSet {
        DevBuf<float4> raw;                                    // upload order
        DevBuf<float4> src;                                    // curve order, frame f from point slice[f].x
        DevBuf<int64_t> d_off;                                 // frame f = points [off[f], off[f + 1]) of the upload
        DevBuf<uint32_t> d_dst;                                // ... and where it starts in src
        DevBuf<dcreg::FrameBox> d_box;
        std::vector<uint2> slice;                              // per frame: {first point in src, points}
        int64_t max_points = 0;
        DevBuf<uint32_t> state;                                // [state][kStateRows][state_stride]
        size_t state_stride = 0;
        int64_t n_states = 0;
        std::vector<uint8_t> state_valid;
        StateKey key;
        // the frames' own kept normals (normals.hip: dcreg_frames_normals_keep / _set; the third engine's many-frames form): float4 {nx,
        // ny, nz, curvature} at the positions of src - lane i of k_glin_batch reads it beside src[i]; dropped by every load of the set
        DevBuf<float4> normals; bool normals_kept = false;
    };
    FrameSet frames;
    // The scan pairs of dcreg_register_pairs (engine.cpp): pair p = source p (a frame of pair_src, loaded as dcreg_register_frames loads its
    // frames) against target p (a build batch of PairSet: every target indexed on its own, all of them at once - context.hip pairs_build).
    // The launches of the call read each pose's source slice and target grid (kernels.hpp k_lin SLICE + GRIDS); nothing of the ctx's own
    // target, source, states, frames or window index is touched.
    FrameSet pair_src;
    struct PairSet {
        DevBuf<float4> raw;                                    // the batch's targets in upload order (w = index within the own cloud)
        DevBuf<float4> sorted;                                 // cell-sorted, target after target, kPtsPad zero entries behind each
        DevBuf<uint32_t> table;                                // the cell tables, target after target
        DevBuf<uint32_t> ymask;                                // the row words, target after target
        DevBuf<int64_t> d_off;                                 // [3][n + 1]: a pass's point, table and row-word offsets (kernels.hpp k_pairs_*)
        DevBuf<dcreg::PairCells> d_cells;
        DevBuf<uint32_t> d_words;                              // bounds of the batch's targets, then occupied cells of a pass
        DevBuf<dcreg::PairGrid> d_grids;                       // per target of the batch: what k_lin<.., GRIDS> reads (empty target: n_pts 0)
        std::vector<uint8_t> built;                            // per target of the batch: it has an index
        int n = 0;                                             // targets of the batch
        float radius_sq_f = 0.f;                               // the search bound the grids' rings were counted for (LinArgs::radius_sq_f)
        // The 1-NN engines' pairs forms (dcreg_register_pairs_normals / _gicp; normals.hip pairs_normals_keep / _set): the kept normals of the
        // batch's targets - float4 {nx, ny, nz, curvature}, target after target, each in its own index order, target t from off[t] - and the
        // record k_nlin_batch<GRIDS> reads per target; both dropped by every build.  off / search_radius: what the batch was built with
        DevBuf<float4> normals; bool normals_kept = false;
        DevBuf<dcreg::OneNnGrid> d_nn_grids;
        std::vector<dcreg::GridDev> grids;                     // host copies of the built targets' grids (the normals pass reads them)
        std::vector<int64_t> off;
        double search_radius = 0.0;
    };
    PairSet pairs;
    // voxel-grid downsampling (voxel.hip voxel_pass: dcreg_voxel_downsample*, dcreg_set_*_voxel).  Per input point: the packed cloud, its
    // cloud (segment) and voxel key relative to the cloud's minimum voxel; per sorted position: head flags and their inclusive scan; per voxel:
    // its first sorted position, its point and keep flag (then their scan); per cloud: the counters of the call (voxel.hip VoxCounters)
    struct VoxelBufs {
        DevBuf<float4> pts;
        DevBuf<uint32_t> seg;
        DevBuf<uint64_t> rel;
        DevBuf<uint32_t> head, incl, start, keep, pos;
        DevBuf<float4> vout;
        DevBuf<float> out;                                   // 3 floats per output point (dcreg_voxel_downsample*)
        DevBuf<int64_t> d_off;
        DevBuf<int64_t> cnt;
    };
    VoxelBufs vox;
    // motion compensation (deskew.hip: dcreg_deskew*, dcreg_set_source_deskew*): per cloud its twist, span and reference instant, the
    // cloud offsets, and the call's keys - [0] finite points, [1] stamps outside their span, [2] minimum stamp key, [3] ~maximum key, then
    // per cloud s [4 + 2s] minimum and [5 + 2s] ~maximum key of its finite stamps (span_from_data)
    struct DeskewBufs {
        DevBuf<dcreg::DeskewCloud> clouds;
        DevBuf<int64_t> d_off;
        DevBuf<unsigned long long> keys;
        DevBuf<dcreg::PathCloud> pclouds;      // the path form (dcreg_deskew_path*): per cloud, and per (cloud, segment)
        DevBuf<dcreg::PathSeg> segs;
    };
    DeskewBufs dsk;
    // place recognition (places.hip: dcreg_place_descriptors*, dcreg_places_*).  The database: `count` descriptors of p.n_rings x p.n_sectors
    // floats (ring-major) and per column the inverse of its norm (0: a zero column); it lives until dcreg_places_reset or the context's end,
    // whatever happens to the target and the source.  The rest is scratch of one call: per (cloud, bin) the key of its maximum, the cloud
    // offsets, the call's counts; the query descriptors and their inverse norms; per (query, entry of the range) distance and shift; the
    // candidate lists of the selection (two sides, used in turn) and the shifts of the result
    struct PlaceBufs {
        bool ready = false;                                  // dcreg_places_reset has fixed p
        dcreg_place_params p{};
        int64_t count = 0;
        DevBuf<float> desc;
        DevBuf<double> inv;
        DevBuf<uint32_t> keys;
        DevBuf<int64_t> d_off;
        DevBuf<unsigned long long> cnt;
        DevBuf<float> qdesc;
        DevBuf<double> qinv;
        DevBuf<double> dist;
        DevBuf<int32_t> shift;
        DevBuf<double> sel_d[2];
        DevBuf<int32_t> sel_i[2];
        DevBuf<int32_t> sel_shift;
    };
    PlaceBufs places;
    // the packed-cloud scratch of every call over a caller's cloud (scratch.hip cloud_used_compact / cloud_index_used): the packed cloud,
    // the used (finite) flags and their scan (n + 1 entries each, the last flag 0), the used points compacted (w = input index) and their
    // index.  Scratch of one call, kept for the next.  The outlier filter packs, compacts and indexes its cloud here, and so do the cloud
    // forms of the normals (one cloud and many) and of both FPFH rules; the map form of the descriptors re-indexes the points with a
    // normal here.  One index for all of them: a descriptor call lets the normals search it and then rebuilds it for itself, and a
    // descriptor report behind any later build is refused (index_epoch)
    struct CloudScratch {
        DevBuf<float4> pts, cpts;
        DevBuf<uint32_t> used, upos;
        IndexSet idx;
    };
    CloudScratch cloud;
    // outlier removal (outliers.hip: dcreg_outlier_filter*, dcreg_set_*_outliers*, dcreg_target_remove_outliers).  Scratch of one call, beside
    // the packed-cloud scratch above: per input point the score, the keep flag and its scan (n + 1 entries each, the last flag 0); the
    // partial sums of the tree reductions (two sides, used in turn); the call's counts ([0] points in the statistics, [1] sparse points);
    // the outputs (3 floats per point, or packed as k_pack packs a cloud) and the byte mask
    struct OutlierBufs {
        DevBuf<float4> out4;
        DevBuf<uint32_t> keep, pos;
        DevBuf<float> score, out;
        DevBuf<uint8_t> mask;
        DevBuf<double> part[2];
        DevBuf<unsigned long long> cnt;
    };
    OutlierBufs outl;
    // keyframe store (keyframes.hip: dcreg_keyframes_*, dcreg_set_target_keyframes).  The store: the points of all keyframes back to back,
    // 3 floats each, in one growing array (capacity doubles), and on the host where each keyframe starts (count + 1 entries once `ready`); it
    // lives until dcreg_keyframes_reset or the context's end, whatever happens to the target and the source.  The rest is scratch of one
    // call: the member records of a gather, the raw output of a submap call to host memory, the non-finite flag of an add
    struct KeyframeBufs {
        bool ready = false;                                  // dcreg_keyframes_reset was called
        DevBuf<float> xyz;
        std::vector<int64_t> off;
        DevBuf<dcreg::KfMember> members;
        DevBuf<float> out;
        DevBuf<uint32_t> flag;
    };
    KeyframeBufs kf;
    // visibility votes (visibility.hip: dcreg_keyframes_range_images*, dcreg_visibility_filter*, dcreg_target_remove_dynamic).  Scratch of one
    // call: the range images of one batch of members and the batch's member records; per point the two counters; the packed cloud of the
    // filter form, its keep flags and their scan (n + 1 entries, the last flag 0), its outputs; the call's counts ([0] finite, [1] observed,
    // [2] flagged points)
    struct VisibilityBufs {
        DevBuf<float> images;
        DevBuf<dcreg::VisMember> members;
        DevBuf<int32_t> through, observed;
        DevBuf<float4> pts;
        DevBuf<uint32_t> keep, pos;
        DevBuf<float> out;
        DevBuf<uint8_t> mask;
        DevBuf<unsigned long long> cnt;
    };
    VisibilityBufs vis;
    // surface normals (normals.hip: dcreg_normals*, dcreg_target_normals*).  Scratch of one call: the outputs per input point (3 + 1 + 3
    // floats, those that are wanted) and the call's counts ([0] points with a normal, [1] sparse points); the cloud form packs, compacts and
    // indexes its cloud in the cloud scratch (CloudScratch: cloud.pts, cpts, used, upos, idx)
    // The many-clouds form (dcreg_normals_clouds*, dcreg_frames_normals_keep): every cloud's used points indexed on its own, all at once
    // (context.hip clouds_index_build into `clouds`: sorted points, tables, row words), cnt two words per cloud; d_off the cloud offsets,
    // d_words the clouds' bounds (6 n ordered floats) and the first compacted point of each (n + 1), d_launch the launch's records
    // [NrmCloud x indexed clouds | {cloud record, block within it} x blocks]
    struct NormalBufs {
        DevBuf<float> normal, curv, eig;
        DevBuf<unsigned long long> cnt;
        PairSet clouds;
        DevBuf<int64_t> d_off;
        DevBuf<uint32_t> d_words;
        DevBuf<unsigned char> d_launch;
    };
    NormalBufs nrm;
    // kept normals and the second engine (normals.hip: dcreg_target_normals_keep / _set / _drop; normal_icp.hip: dcreg_linearize_normals).
    // normals: float4 {nx, ny, nz, curvature} per map point in INDEX order (the kernel reaches it through the nearest point's original
    // index: the whole map's index and the window serve alike); dropped with every change of the map's points (context.hip target_commit,
    // map_changed).  warm: per source point (curve order) the sorted position of its last nearest neighbour - the start bound of its next
    // search, nothing more; valid for one pair of source and ACTIVE index (context.hip drop_warm).  partials / d_out: the block rows of a
    // launch and its result row; dbg: the dump buffers of the debug form
    // The batched form (normal_icp.hip k_nlin_batch: dcreg_normals_batch_begin / _end, the engine of dcreg_register_frames_normals): two launch
    // slots with their own block rows, pose block ([PoseArg x n | slices x n], pinned, and its device copy) and result rows (device, and
    // the pinned copy `done` is recorded behind), so that one group's kernel runs while the host steps the other.  slots: n_slots warm
    // arrays of slot_stride words, positions in the WHOLE map's sorted array (batched launches never search the window index), sized for
    // the largest loaded frame, the largest pair source or the own source (slots_for); slot_valid: the array holds the positions of an earlier launch
    // Following the map ("normals_follow", normals.hip normals_follow_*): reach = one float per map point beside its normal, the squared
    // distance within which a point that comes or goes can change it (the k-th neighbour's d2; the search bound for a sparse point);
    // from_keep / keep_params: the normals came from dcreg_target_normals_keep with these parameters - the rule an update refits with.
    // normals_alt / reach_alt: the survivors' entries of a removal, compacted beside the current arrays and swapped in once the update
    // stands.  f_bits: one bit per cell of the updated map's grid, set where a point came or went; f_list: the dirty points, compacted
    // in cell order (k_nrm's input).  follow: what the last update that changed the map did to the kept normals
    struct NormalIcpBufs {
        DevBuf<float4> normals; bool kept = false;
        DevBuf<float> reach; bool from_keep = false;
        dcreg_normal_params keep_params{};
        DevBuf<float4> normals_alt, f_list;
        DevBuf<float> reach_alt;
        DevBuf<uint32_t> f_bits, f_flag;
        dcreg_normals_follow_info follow{};
        DevBuf<uint32_t> warm; bool warm_valid = false;
        DevBuf<double> partials, d_out;
        DevBuf<unsigned char> dbg;
        struct BatchSlot {
            DevBuf<double> partials, d_out;
            PinnedBuf<unsigned char> h_poses;
            DevBuf<unsigned char> d_poses;
            PinnedBuf<double> h_out;
            hipEvent_t done = nullptr;
            int n_poses = 0;
            bool pending = false;
            std::vector<int32_t> ids;          // the warm slots the launch in flight writes
        };
        BatchSlot batch[2];
        DevBuf<uint32_t> slots;
        size_t slot_stride = 0;
        int64_t n_slots = 0;
        enum class SlotsFor : uint8_t { source, frames, pairs };   // the clouds the warm slots were sized for: the own source, the loaded frames, the pairs' sources
        SlotsFor slots_for = SlotsFor::source;
        std::vector<uint8_t> slot_valid;
        bool batch_pending() const { return batch[0].pending || batch[1].pending; }
        void drop_slots() { std::fill(slot_valid.begin(), slot_valid.end(), (uint8_t)0); }
    };
    NormalIcpBufs nicp;
    // the third engine (gicp.hip: dcreg_linearize_gicp; normals.hip: dcreg_source_normals_keep / _set / _get / _drop).  src_normals: float4
    // {nx, ny, nz, curvature} per SOURCE point in the context's curve order - lane i of k_glin reads it beside d_src[i]; dropped by every
    // call that replaces the source's points (context.hip source_commit), left alone by the batched calls.  The warm words are nicp.warm:
    // both 1-NN engines look for the same nearest point, and so are nicp's block rows, result row and dump block (normal_icp.hip rows_run: the
    // engines' single-pose launches never overlap).  tmp: the original-order form of a get.
    // The batched form (k_glin_batch: dcreg_gicp_batch_begin / _end) has no buffers of its own: it runs in nicp's launch slots and warm
    // slots (normal_icp.hip one_nn_batch_begin) and reads a frame's normals from FrameSet::normals
    struct GicpBufs {
        DevBuf<float4> src_normals; bool src_kept = false;
        DevBuf<float4> tmp;
    };
    GicpBufs gicp;
    // the kept voxel map and the fourth engine (voxel.hip: dcreg_target_voxels_keep / _get / _kept / _drop; voxel_icp.hip:
    // dcreg_linearize_voxels).  recs: 3 float4 per kept voxel in _get order (ascending z y x) - {mu, cxx} {cxy cxz cyy cyz} {czz, n as a
    // word, 0, 0}; vkeys: each one's key, (v - mn) per axis in 21 bits (what _get turns back into coordinates); t_keys / t_vals: the
    // open-addressing table a lookup probes (voxel_icp.hpp VoxMapDev), mask + 1 slots; mn / mx: the voxel box of all map points.  Dropped
    // with every change of the map's points (context.hip target_commit, map_changed) unless an update follows it ("voxels_follow").  tmp / cls: scratch of a keep - the records of all
    // voxels before compaction, and the counts [0] small [1] degenerate.  The engine's block rows, result row and dump block are nicp's
    // (the single-pose launches of the engines never overlap).
    // Following the map ("voxels_follow", voxel.hip voxels_follow_*): params = the block of the keep that made the member; *_alt: the
    // arrays a followed update builds the next member in (swapped in after its last launch); f_set: the touched voxels' keys, an
    // open-addressing set; f_cnt: its counters; f_sub: the points of the touched voxels, gathered in index order; f_flag: carry flags of
    // the old records and their scan; f_akeys / f_asrc, f_bkeys / f_bsrc: key and source record of the two sorted runs of the merge
    struct VoxelMapBufs {
        DevBuf<float4> recs, tmp;
        DevBuf<uint64_t> vkeys, t_keys;
        DevBuf<uint32_t> t_vals;
        DevBuf<unsigned long long> cls;
        bool kept = false;
        int64_t n_kept = 0;
        uint32_t mask = 0;
        long long mn[3] = {}, mx[3] = {};
        double leaf = 0.0;
        dcreg_voxel_map_params params{};
        dcreg_voxels_follow_info follow{};
        DevBuf<float4> recs_alt, f_sub;
        DevBuf<uint64_t> vkeys_alt, t_keys_alt, f_set, f_akeys, f_bkeys;
        DevBuf<uint32_t> t_vals_alt, f_flag, f_asrc, f_bsrc;
        DevBuf<long long> f_cnt;
    };
    VoxelMapBufs vmap;
    int opt_voxels_source_cov = 0;                             // "voxels_source_cov": 0 point-to-distribution, 1 distribution-to-distribution, read at every call
    int opt_voxels_follow = 0;                                 // "voxels_follow": 1 = an update refits the kept voxel map of dcreg_target_voxels_keep instead of dropping it
    double opt_voxels_follow_full_share = 0.25;                // "voxels_follow_full_share": past this share of the map's points in touched voxels a followed update runs the full keep
    int opt_voxels_neighbors = 1;                            // "voxels_neighbors": the voxels a point is matched to - its own (1), with the face neighbours (7), the whole 3^3 block (27), read at every call
    double opt_gicp_epsilon = 1.0e-3;                          // "gicp_epsilon": the small eigenvalue of both plane covariances, read at every call
    int opt_robust_kernel = 0;                                 // "robust_kernel" (DCREG_ROBUST_*): the second and third engine's rows, read at every call
    double opt_robust_scale = 0.1;                             // "robust_scale": its scale c for the second engine, metres
    double opt_gicp_robust_scale = 1.0;                        // "gicp_robust_scale": ... for the third engine, whitened units
    double opt_visibility_max_bytes = 268435456.0;             // "visibility_max_bytes": the images of one batch of members
    int opt_visibility_order = 1;                              // the map form votes in index order (0) or in cell order (1)
    int64_t opt_pair_max_table_entries = (int64_t)1 << 24;    // "max_table_entries" of every pair target
    double opt_pairs_max_bytes = 0.0;                          // device bytes of one build batch of pair targets (0: a quarter of the free memory)
    PinnedBuf<double> h_euler;                         // Euler engine: the 27 derivative entries of a launch (LinArgs::dR)
    DevBuf<double> d_euler;
    DevBuf<unsigned long long> d_search_count;         // option "count_searches": points searched since the last reset

    // build scratch
    DevBuf<float> d_stage;
    // small frames from host buffers (the registration path): the caller's floats are copied into this pinned block with a plain memcpy and
    // uploaded from there - the caller's buffer is consumed when dcreg_set_source returns whatever kind of memory it is, without a
    // stream synchronise; h_stage_ev = the upload behind the last use of the block
    PinnedBuf<float> h_stage; hipEvent_t h_stage_ev = nullptr; bool h_stage_busy = false;
    hipEvent_t null_ev = nullptr;          // caller_order: marks the work queued on the legacy default stream before a device input is read
    DevBuf<uint32_t> d_keys, d_keys2, d_vals, d_vals2;
    DevBuf<uint64_t> d_mkeys, d_mkeys2;
    DevBuf<uint32_t> d_scratch;
    DevBuf<char> sort_tmp;

    // linearisation: per-slot buffers (see linearize_begin / linearize_end)
    // gate of pipelined launches (kernels.hpp k_gate): pinned sequence number + pose, the device-resident pose it fills, abort word
    PinnedBuf<dcreg::GateHost> h_gate;     // (mapped: h_gate.dev() is the record's device address)
    DevBuf<dcreg::PoseArg> d_gate_pose;
    DevBuf<uint32_t> d_gate_abort;
    DevBuf<dcreg::GateDev> d_gate_dev;     // device copy of the gate record: launches gated in their first kernel (kernels.hpp gate_wait)
    bool opt_gate_in_kernel = true;
    int opt_one_wave = 1;                 // k_lin<.., ONE> (one-wave blocks): 0 never, 1 by the rule, 2 wherever possible
    bool opt_one_wave_batches = true;     // ... for batched launches of one-chunk poses with at least opt_one_wave_min_blocks blocks in all
    double opt_one_wave_min_frac = 0.5;
    double opt_one_wave_min_cells = 1.5;
    int opt_one_wave_min_blocks = 1024;
    unsigned long long gate_seq = 0;       // number of the gated launch last queued
    int gate_slot = -1;                    // slot of the gated launch that still waits for its pose (-1: none)
    bool gate_uses_state = false;          // what the queued launch was built with: it reads / writes the ctx's own state,
    bool gate_state_was_valid = false;     //   and what state_valid was before it was queued (restored if it is called off)
    bool gate_state_was_five = false;      //   ... and state_five
    static constexpr int kLinSlots = 2;
    LinSlot slots[kLinSlots];

    // k-NN / p2p
    DevBuf<float4> d_aligned;
    DevBuf<int32_t> d_nn_idx;
    DevBuf<float> d_nn_d2;
    DevBuf<double> d_p2p_part;

    // native exchange of point-sharded runs (exchange.hip): an ncclComm_t on this ctx's device + staging rows
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    DevBuf<double> d_xrow, d_xall;
    PinnedBuf<double> h_xrow, h_xall;

    // options / timing
    double opt_cell = 0.0, opt_cell_factor = 2.0;
    int opt_x_subdiv = 8;          // x sub-cells per grid cell (1, 2, 4, 8, 16)
    bool opt_use_cert = true;      // skip the search of every point whose certificate still holds (0: only bound the searches)
    bool opt_count_searches = false;
    double opt_cert_inflate = 0.005; // searches prune at (1 + inflate) x the 6th best distance: the 7th neighbour's lower bound (SET6 certificates)
    double opt_cert_margin = 0.05; // searches cover R (1 + margin): what "5th neighbour beyond R" certificates can spend
    int opt_time_kernels = 0;      // N > 0: bracket every N-th linearisation with HIP events
    uint64_t launch_counter = 0;
    double opt_wait_seconds = 30.0; // how long a result is awaited before the stream is drained to look for a device fault
    bool opt_spin = true;          // wait for results by spinning on pinned memory instead of hipStreamSynchronize
    bool need_set_device = true;
    unsigned long long seq = 0;
    bool opt_fast_plane = true;    // plane_fit_qr_fast (search.hpp) instead of the Eigen-shaped plane_fit_qr
    bool opt_gap_field = true;     // build the empty-space distance field of the target grid
    bool opt_far_bound = true;     // far queries with a loose bound start from the points around the nearest occupied cell (search.hpp lin_search6)
    bool opt_keep_source_order = false;   // experiments only
    // heavy groups first (kernels.hpp k_group_cost): the dispatch order of the query-block groups, estimated once per cloud pair
    bool opt_dispatch_order = true;
    uint8_t group_order[256] = {}; DevBuf<float> d_group_est;
    uint32_t group_blocks = 0, n_groups = 0;
    int n_cus = 256;                // compute units of the device
    void *kd = nullptr;             // kd-tree comparator (kdtree.hip), built on request
    bool order_valid = false;       // group_order is the estimate for est_R / est_t; order_uneven: its costs differ enough to matter
    bool order_uneven = false;
    double est_R[9] = {}, est_t[3] = {};
    int64_t est_launch = 0;         // the launch number (seq) at which the estimate was made
    double hint_misalign = 1e300;   // dcreg_hint_misalignment
    // "nothing known" (a negative hint: what the engines say at the start of a run) is resolved at the next launch whose pose is known up
    // front: a pose within half a cell of the last linearised one continues that trajectory - the last hint still describes it (a run
    // that is stepped through in several engine calls does not pay a cost estimate at the start of each)
    bool hint_unknown = false;
    double hint_last = 1e300, last_R[9] = {}, last_t[3] = {};
    bool last_pose_valid = false;
    double opt_curve_x_scale = 1.0;  // kernels.hpp k_curve_keys: < 1 stretches the patches of the source's curve order along x
    int64_t opt_max_table_entries = (int64_t)1 << 30;   // entries of the dense cell table (x sub-cells of the bounding box) before the cell edge grows
    // the advance pass (kernels.hpp k_advance) and its small-frame form (k_advance_team): 0 never, 1 by the rules of context.hip lin_plan,
    // 2 whenever a launch can take it (tests)
    int opt_advance = 1;
    int opt_advance_fused = 1;           // the advance pass carries its launch out alone (kernels.hpp k_advance ROWS); 0: k_advance + k_lin
    int opt_advance_min_blocks = 2048;   // k_advance by the rule: the cloud has at least this many query blocks (twice what the device holds)
    int opt_team_pass = 1;
    bool opt_team_stamps = false;
    DevBuf<unsigned long long> d_team_stamps; uint32_t team_stamps_n = 0;
    DevBuf<uint32_t> d_adv_counts; bool adv_counts_dirty = true;
    int64_t n_advance_launches = 0;
    // Five-neighbour launches (kernels.hpp k_lin FIVE): 0 never, 1 by the rule of context.hip lin_plan, 2 wherever a launch can be one
    // (tests).  state_five: the last launch queued on the ctx's own state was one - every certificate in it has radius zero, the next
    // five-neighbour launch does not load them.  last_step: how far the pose of the last launch of an engine's trajectory lies from the
    // pose before it (pose_jump; 1e300 = a run starts, nothing known; 0 = no trajectory: launches nobody announced)
    int opt_search_five = 1;
    double opt_search_five_step = 0.04;  // the rule: the last known step exceeds this many cell edges
    double opt_search_five_frac = 0.95;  // ... and the last completed launch searched at least this share of its points
    bool state_five = false;
    int five_tail = 0;                   // launches still to come whose searched share the last completed launch does not predict (lin_plan)
    double last_step = 0.0;
    int opt_team_max = 7;          // search.hpp team_search6: waves with at most this many lanes to search serve them cooperatively
    bool opt_warm = true;          // bound each search by the previous neighbour set (same exact result, fewer cells)
    int64_t n_launches = 0, n_poses_launched = 0, n_points_launched = 0;    // dcreg_launch_stats
    double kernel_ms_total = 0.0;
    int64_t kernel_launches = 0;
    // what the last completed launch did (decoded from the count slots of its result rows, search.hpp LinArgs::count_scale): points
    // searched / refitted, -1 = not reported.  Scheduling input of the next launches; "record_launches": every launch is also logged
    int64_t last_searched = -1, last_refitted = -1, last_points = 0;
    struct LaunchRec { double ms; int64_t searched, refitted, points; int advanced, structure; };
    bool opt_record_launches = false;
    std::vector<LaunchRec> launch_series;

    // The pairs' voxel maps (voxel.hip pairs_voxels_build: dcreg_pairs_voxels_build, the build batch of dcreg_register_pairs_voxels): one
    // kept voxel map per target of the batch, all of them built at once.  recs / vkeys: the kept records and keys of all targets, target
    // after target, each target's in dcreg_target_voxels_get order; t_keys / t_vals: the targets' lookup tables one behind the other, each
    // the power of two at or above twice its kept voxels; maps / d_maps: per target where its records and table start, its mask and its
    // voxel box (host and device copies).  tmp, d_cnt (per target: voxels, small, degenerate, kept) and d_words (the pack's bounds) are
    // scratch of a build; the packed points and the sort run in the voxel pass's scratch (vox).  Every build replaces the batch; the
    // pairs' index batch (pairs) is another member and is not touched.  (Last in the struct: no option field above moves.)
    struct PairVoxBufs {
        DevBuf<float4> recs, tmp;
        DevBuf<uint64_t> vkeys, t_keys;
        DevBuf<uint32_t> t_vals, d_words;
        DevBuf<unsigned long long> d_cnt;
        DevBuf<dcreg::PairVoxMap> d_maps;
        std::vector<dcreg::PairVoxMap> maps;
        int n = 0;                                             // targets of the batch (0: none built)
        double leaf = 0.0;
    };
    PairVoxBufs pvox;

    // FPFH descriptors and feature-space matching (features.hip: dcreg_fpfh*, dcreg_target_fpfh*, dcreg_feature_match*).  Scratch of one
    // call, kept for the next.  Descriptors: the caller's normals as uploaded (the host form), per used point in cell order the neighbour
    // list ([slot][point]: position in the sorted array and d2, k slots) and the SPFH record (12 words: 33 byte counts, then m and the
    // "has an SPFH" flag), the 33 floats per input point, the call's counts ([0] descriptors, [1] empty points, [2] non-finite kept
    // normals of the map form).  Matching: both descriptor sets (the host form), per row of either set its valid flag, per (split, query)
    // the partial winners {D1, D2, {j1, j2}}, the results of both directions and the counts ([0] valid a, [1] valid b, [2] mutual).
    // The cloud form packs, compacts and indexes its cloud in the cloud scratch (CloudScratch), as the normals do.
    struct FeatureBufs {
        DevBuf<float> nrm_in, out;
        DevBuf<uint32_t> nb_pos;
        DevBuf<float> nb_d2;
        DevBuf<uint4> spfh;
        DevBuf<unsigned long long> cnt;
        DevBuf<float> a, b;
        DevBuf<uint8_t> va, vb, mutual;
        DevBuf<double> part_d;
        DevBuf<int32_t> part_i;
        DevBuf<int32_t> idx, idx2, idx_b;
        DevBuf<double> d1, d2;
        // dcreg_fpfh_debug_counts: the sorted points, their number and the input's size of the last descriptor call, and the export
        const float4 *last_q = nullptr; int64_t last_nq = 0, last_n = 0;
        uint64_t last_epoch = 0;       // dcreg_ctx::index_epoch when last_q / rlast_q was taken: a report behind a later epoch is refused
        DevBuf<uint32_t> dbg;
        // the radius rule (dcreg_fpfh_radius*): per used point its record (q[33], m, has, 0) and its 33 counts, in the index's cell order;
        // what dcreg_fpfh_radius_debug_counts reports.  A call of either rule ends the other's report
        DevBuf<uint4> rrec;
        DevBuf<uint32_t> rcounts;
        const float4 *rlast_q = nullptr; int64_t rlast_nq = 0, rlast_n = 0;
    };
    FeatureBufs feat;
    int64_t opt_feature_match_split = 0;                      // "feature_match_split": rows of b per block column of k_match (0: from the sizes; tests)

    // A pose from correspondences (align.hip: dcreg_align_correspondences*).  Scratch of one call, kept for the next: both clouds and both
    // index arrays as uploaded (the host form), per correspondence its used flag and the flags' exclusive scan (n_pairs + 1 entries: the
    // last one is the number of used pairs), the used pairs compacted ([u] -> p, q: six floats) with their correspondence numbers, the
    // survivors' keys {count, h, cost} as k_align_hypotheses appends them and in rank order, the counts ([0] survivors, [1] degenerate,
    // [2] rejected hypotheses).
    struct AlignBufs {
        DevBuf<float> a, b, P;
        DevBuf<int32_t> ca, cb, m_of_u;
        DevBuf<uint32_t> flag, pos;
        DevBuf<dcreg::AlignKey> keys, sorted;
        DevBuf<unsigned long long> cnt;
    };
    AlignBufs algn;
    int64_t opt_align_score_split = 0;                        // "align_score_split": used pairs per block column of k_align_score (0: from the sizes; tests)

    // The consensus pose (consensus.hip: dcreg_consensus_correspondences*), behind the used pairs of AlignBufs.  The compatibility graph as
    // a bit matrix, word-major (adj[word * M_u + u]: bits 64 word .. 64 word + 63 of row u), deg and w per used pair, the seeds' sort keys
    // ((~w) << 32 | u) unsorted and sorted, per seed its row of second-order counts (uint16, M_u each), its members (64 used-pair numbers)
    // and their number, the scored sets' poses (12 doubles) and keys {count, place, cost}, and the host form's degree / weight outputs.
    struct ConsensusBufs {
        DevBuf<unsigned long long> adj, key, key_sorted;
        DevBuf<uint32_t> deg, w, mem, n_mem, out_deg, out_w;
        DevBuf<uint16_t> s_row;
        DevBuf<double> pose;
        DevBuf<dcreg::AlignKey> score;
    };
    ConsensusBufs cons;

    // Verification of candidate poses (verify.hip: dcreg_verify_poses*).  Scratch of one call, kept for the next, and nothing any other
    // call reads: the cloud form's rows as uploaded, the selection flags and their exclusive scan (n + 1 entries, the last flag 0), the
    // selected points compacted (w = the original index), the pose table (12 doubles per pose), the sums {count, cost} per pose, and the
    // detail pose's mask and nn by original index.
    struct VerifyBufs {
        DevBuf<float> rows;
        DevBuf<uint32_t> flag, pos;
        DevBuf<float4> sel;
        DevBuf<double> poses;
        DevBuf<unsigned long long> acc;
        DevBuf<uint8_t> mask;
        DevBuf<int32_t> nn;
    };
    VerifyBufs verify;
    int64_t opt_verify_poses_per_launch = 0;                  // "verify_poses_per_launch": poses per launch of k_verify (0: all of them; tests)

    void fail(const char *fmt, ...);
};

template <typename T>
int DevBuf<T>::ensure(dcreg_ctx *c, size_t need, const char *why) {
    if (holds(need)) return DCREG_OK;
    const size_t n = std::max<size_t>(need, 1);
    const hipError_t e = alloc(n);
    if (e != hipSuccess) {
        (void)hipGetLastError();      // (the failed allocation must not surface as the "launch error" of whatever is queued next)
        if (why) c->fail("hipMalloc(%zu B) failed %s", n * sizeof(T), why);
        else c->fail("hipMalloc(%zu B) failed: %s", n * sizeof(T), hipGetErrorString(e));
        return DCREG_E_NOMEM;
    }
    return DCREG_OK;
}

template <typename T>
int DevBuf<T>::grow_keep(dcreg_ctx *c, size_t need, size_t keep) {
    if (holds(need)) return DCREG_OK;
    DevBuf fresh;
    const size_t n = std::max(need, cap_ + cap_ / 2);
    if (fresh.alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        c->fail("hipMalloc(%zu B) failed while growing the map", n * sizeof(T));
        return DCREG_E_NOMEM;
    }
    if (p_ && keep) HIP_TRY(c, hipMemcpyAsync(fresh.p_, p_, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    swap(fresh);                      // (the old buffer goes with `fresh`)
    return DCREG_OK;
}

namespace dcreg {

int launch_linearize(dcreg_ctx *c, int n_poses, const double *R9, const double *t3, const dcreg_lin_params *p,
                     dcreg_lin_out *outs, dcreg_lin_debug *dbg_host);
void kdtree_free(void *kd);      // kdtree.hip (the comparator index of dcreg_debug.h)
int roi_ensure(dcreg_ctx *c, const double *R, const double *t, double search_radius);   // context.hip: the index a single-pose linearisation at this pose searches becomes the active one
// ---- normal_icp.hip: the host seam of the engines that leave block rows for k_finalize (the second, third and fourth: dcreg_linearize_normals,
// _gicp and _voxels and their batched forms).  The rows_* functions serve all three; the one_nn_* functions are about the 1-NN search and
// serve the second and third only - the fourth searches nothing.
// n finite numbers (a pose's R and t, many poses' R9 and t3, ...)
inline bool finite_n(const double *v, int64_t n) {
    for (int64_t k = 0; k < n; ++k) if (!std::isfinite(v[k])) return false;
    return true;
}
// rows_run: the back half of a single-pose call, plain or debug, behind the engine's refusals (all three engines) - nicp's block rows and
// result row sized for the context's source, the dump block cut into its arrays, `launch` (it queues the engine's kernel: nb blocks that
// leave their rows at partials), the copies of the dump arrays that were asked for, k_finalize, the row copy, the wait and the result.
// fields: the debug form's arrays in the order they are cut from the dump block (8-byte ones first): the caller's array (null: not asked
// for), its bytes per point, and the kernel argument's pointer that receives the device array; n_fields == 0: the plain form
struct DumpField { void *host; size_t bytes; void *dev; };
int rows_run(dcreg_ctx *c, dcreg_lin_out *out, const DumpField *fields, int n_fields, const std::function<void(double *partials, uint32_t nb)> &launch);
// What the single-pose 1-NN linearisations (dcreg_linearize_normals, dcreg_linearize_gicp) share in front of it.  one_nn_check: every refusal
// of both, in the header's order, up to "no kept normals" (`what` names the linearisation in the messages).  one_nn_bound: the gate R^2, the
// cold search bound (the smallest float >= R^2) and the rings that cover it.  The warm words (NormalIcpBufs::warm): _reserve sizes them for
// the source (a new array holds nothing), _take returns what a plain launch starts from (null: cold) and marks them invalid until _done
// says that the launch has run; a debug launch calls neither
struct OneNnBound { double radius_sq; float bound_f; int max_ring; };
int one_nn_check(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, const dcreg_lin_out *out, const char *what);
OneNnBound one_nn_bound(const GridDev &g, double search_radius);
int one_nn_warm_reserve(dcreg_ctx *c);
// one_nn_run: the single-pose call of either 1-NN engine, plain or debug - what belongs to a search against the index: one_nn_check, the
// engine's own refusal (`extra`, with fs == null), roi_ensure, the warm words and the search bound; then rows_run, with `launch` queueing
// the engine's kernel for the filled record, and the warm bookkeeping.  fields / n_fields: rows_run's (read with dump only)
struct OneNnLaunch {
    PoseArg P; OneNnBound bound;                // the pose, the search bound on the active index
    bool dump;                                  // the debug form: the kernel's dump instantiation, no warm words
    const uint32_t *warm_in; uint32_t *warm_out;
    double *partials; uint32_t nb;
};
int one_nn_run(dcreg_ctx *c, const double *R, const double *t, const dcreg_lin_params *p, dcreg_lin_out *out, const char *what,
               int (*extra)(dcreg_ctx *, const dcreg_ctx::FrameSet *fs), const std::function<void(const OneNnLaunch &)> &launch, bool dump,
               const DumpField *fields, int n_fields);
// ... and the batched forms: the two launch slots of NormalIcpBufs, which all three engines share (a pending slot of one refuses the others).
// rows_batch_check: the front of every batched begin's refusal ladder (include/dcreg_debug.h), in this order - null context, bad slot, null
// arguments (ids_given: the ids a launch cannot do without are there) or n_poses < 1, more than 65535 poses, a waiting gate, a pending
// slot of the first engine, this slot pending, the parameterization (`what` names the linearisation in the message), with `search` the
// search radius, a non-finite pose.  The engine's state refusals follow it.
int rows_batch_check(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const dcreg_lin_params *p, bool ids_given, const char *what,
                     bool search);
// rows_batch_clouds: the clouds of a launch and n_max, the points of the largest.  fs == null: the context's own source ("no source").
// Else pose i's cloud is ids[i] of fs (c->frames or c->pair_src): "no frames" / "no pair sources" for an empty set, then pose by pose an
// id outside the set or naming an empty cloud ("<noun> %d is not loaded or empty") and whatever pose_check(i) refuses (may be empty: the
// voxel pairs launch checks pose i's target there, after its source and before pose i + 1's)
int rows_batch_clouds(dcreg_ctx *c, const dcreg_ctx::FrameSet *fs, int n_poses, const int32_t *ids, const char *noun,
                      const std::function<int(int)> &pose_check, int64_t &n_max);
// one_nn_batch_begin (dcreg_normals_batch_begin, dcreg_gicp_batch_begin and their pairs forms) makes every refusal of the header before
// anything is queued - rows_batch_check, the state refusals, rows_batch_clouds, `extra` (the engine's own state refusals, after "no kept
// normals"), the warm slots - and queues through rows_batch_queue with the index, the kept normals, the bound and the warm slots filled in.
// fs: the source set frame_ids index (c->frames, or c->pair_src; null with frame_ids == null: the own source).
// target_ids (with fs == &c->pair_src only): pose i searches target target_ids[i] of the pairs' build batch and reads that target's kept
// normals (OneNnGrid) instead of the map and its kept normals; the state refusals are then "no pair batch built" and "no kept pair normals"
struct OneNnBatch {
    const float4 *src; uint32_t n_src;          // the set's points (slices != null) or the own source
    const float4 *src_normals;                  // ... and its kept normals at the same positions (the third and fourth engine)
    GridDev g;                                  // the whole map's index (grids == null)
    const float4 *normals;                      // the map's kept normals, or the pair batch's
    const OneNnGrid *grids; const uint32_t *grid_ids;   // device; pairs: the batch's target records and every pose's target
    const PoseArg *poses; const uint2 *slices;  // device
    OneNnBound bound;
    uint32_t *warm; uint32_t warm_stride;
    double *partials; uint32_t nbx; int n_poses;
    const dcreg_lin_params *p;
};
int one_nn_batch_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids, dcreg_ctx::FrameSet *fs,
                       const int32_t *frame_ids, const int32_t *target_ids, const dcreg_lin_params *p,
                       int (*extra)(dcreg_ctx *, const dcreg_ctx::FrameSet *fs), void (*launch)(dcreg_ctx *, const OneNnBatch &), const char *kernel_name);
// rows_batch_queue: the slot plumbing behind the refusals, for all three engines (the fourth: voxel_icp.hip vlin_batch_begin,
// vlin_pairs_batch_begin) - the slot's buffers sized for the largest cloud (n_max: the launch's largest), the pinned pose
// and slice block and its upload, `launch` (it completes the record - the fields of the engine's own target stay zero until then - and
// queues the engine's kernel), k_finalize, the result copy, the slot's event and the `failed` path.  state_ids == null: no warm slot is
// read or written.  The caller has made every refusal, the slot's `pending` included.  rows_batch_end waits for the slot's event and
// turns its rows into results (dcreg_normals_batch_end, dcreg_gicp_batch_end, dcreg_voxels_batch_end)
int rows_batch_queue(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids, dcreg_ctx::FrameSet *fs,
                     const int32_t *frame_ids, const int32_t *target_ids, int64_t n_max, const std::function<void(OneNnBatch &)> &launch,
                     const char *kernel_name);
int rows_batch_end(dcreg_ctx *c, int slot, dcreg_lin_out *outs);
// the warm slots of the batched 1-NN forms, sized for the own source, the loaded frames or the pairs' sources (dcreg_normals_reserve_slots,
// dcreg_pairs_normals_reserve_slots)
int one_nn_reserve_slots(dcreg_ctx *c, int64_t n_slots, dcreg_ctx::NormalIcpBufs::SlotsFor what);
const uint32_t *one_nn_warm_take(dcreg_ctx *c);
void one_nn_warm_done(dcreg_ctx *c);
// a result row of kSlots doubles (block_slot_sum's slots, summed) as the C-ABI's record
inline void lin_out_of_row(const double *row, dcreg_lin_out &o) {
    std::memcpy(o.H_upper, row, 21 * sizeof(double));
    std::memcpy(o.g, row + 21, 6 * sizeof(double));
    o.sum_r2 = row[27]; o.sum_b2 = row[28];
    o.n_eff = (int64_t)std::llround(row[29]); o.n_pt = (int64_t)std::llround(row[30]);
}
int roi_deactivate(dcreg_ctx *c);      // context.hip: make the whole map's index the active one (entry points that are not single-pose linearisations)
// the rule of the deskew calls (deskew.hip is_rotation) on the rotation block of a row-major 4x4: what dcreg_p2p_error and
// dcreg_verify_poses* refuse a pose by
inline bool rigid_rotation(const double T[16]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = T[i] * T[j] + T[4 + i] * T[4 + j] + T[8 + i] * T[8 + j] - (i == j ? 1.0 : 0.0);   // (R^T R - I)_ij
            if (!(std::fabs(g) <= 1e-6)) return false;
        }
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) + T[2] * (T[4] * T[9] - T[5] * T[8]);
    return det > 0.0;
}
// align.hip: step 1 of the alignment rule for both correspondence calls - both clouds and both index arrays through caller_rows (the host
// form's staged in c->algn.a / b / ca / cb, the device form's ordered once), k_align_valid, the scan and k_align_gather into c->algn.P /
// m_of_u - and the number of used pairs, read back behind a stream synchronisation.  n_pairs > 0
int align_used_pairs(dcreg_ctx *c, const float *a, int64_t n_a, int64_t stride_a, const float *b, int64_t n_b, int64_t stride_b, const int32_t *ca,
                     const int32_t *cb, int64_t n_pairs, bool on_device, uint32_t *m_u);
int refuse_in_flight(dcreg_ctx *c);    // context.hip: DCREG_E_STATE while a linearisation is queued or in flight (entry points that queue work)
// deskew.hip: one call's motion compensation, checked and prepared on the host by deskew_prepare (every refusal of include/dcreg.h before
// anything is queued).  upload_cloud given one packs the records with k_pack_deskew instead of k_pack (into its float4 buffer, or 3 floats
// per point to out3 when set); deskew_readback queues the copy of the call's counts into `head` (the caller synchronises: it rides on the
// readback the call has anyway), deskew_info decodes them.  deskew_path_prepare fills the path form (dcreg_deskew_path*) instead: the pack
// is then k_pack_deskew_path, everything else goes the same way.
struct DeskewRun {
    int n_clouds = 0;
    const int64_t *off = nullptr;          // host, n_clouds + 1
    int column = 0, type = 0;
    double scale = 1.0;
    std::vector<DeskewCloud> clouds;
    bool any_from_data = false;
    bool path = false;                     // the path form: pclouds and segs instead of clouds
    std::vector<PathCloud> pclouds;
    std::vector<PathSeg> segs;
    float *out3 = nullptr;
    bool queued = false;                   // the pack was queued (not for an empty call)
    bool read = false;                     // the counts were queued for readback
    unsigned long long head[4] = {0, 0, ~0ull, ~0ull};
};
int deskew_prepare(dcreg_ctx *c, int n_clouds, const int64_t *off, int64_t stride, const dcreg_time_field *f, const dcreg_sweep_motion *m,
                   DeskewRun &d);
struct PathTable {                         // the knot table and path blocks of a dcreg_deskew_path* call (host memory, borrowed)
    int64_t n_knots;
    const double *stamps, *poses;
    const dcreg_sweep_path *paths;
};
int deskew_path_prepare(dcreg_ctx *c, int n_clouds, const int64_t *off, int64_t stride, const dcreg_time_field *f, const PathTable &t,
                        DeskewRun &d);
int deskew_reserve(dcreg_ctx *c, const DeskewRun &d);       // the call's device buffers grow here, before upload_cloud queues anything
int deskew_queue(dcreg_ctx *c, const float *src, int64_t n, int64_t stride, DeskewRun &d, float4 *out4);
int deskew_readback(dcreg_ctx *c, DeskewRun &d);
void deskew_info(const DeskewRun &d, int64_t n_in, dcreg_deskew_info *info);
// keyframes.hip: one call's gather of keyframe members (checked on the host by the caller: ids, poses, sizes).  upload_cloud given one has
// the n packed records written by k_kf_gather from the store instead of k_pack from a cloud (xyz is not read); gather_queue with out3 set
// writes 3 floats per point there instead.  Empty members are left out of `members`.
struct GatherRun {
    std::vector<KfMember> members;
    int64_t n = 0;                         // points of the call
};
int gather_queue(dcreg_ctx *c, const GatherRun &g, float4 *out4, float *out3);
// context.hip: a caller's cloud packed into `raw` - host records staged in c->d_stage (a small frame through the pinned block first), a
// device cloud ordered by caller_order: the seam call of every entry point that takes a cloud
int upload_cloud(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, DevBuf<float4> &raw,
                 DeskewRun *dsk = nullptr, const GatherRun *gat = nullptr);
// voxel.hip: the voxel-grid pass of n_clouds clouds (offsets off[n_clouds + 1], host memory) - checks everything before it writes; the output
// points go to c->vox.out (3 floats each) or, packed, to c->d_aligned as k_pack packs a cloud (one cloud only).  Ends with ONE readback of
// the per-cloud counts and the bounds of the output.  dsk: the clouds are deskewed while they are packed (its counts come back with the
// pass's first readback).
struct VoxelResult {
    std::vector<int64_t> voxels, kept;     // per cloud
    int64_t n_in = 0, n_finite = 0, n_voxels = 0, n_out = 0;
    double mn[3] = {}, mx[3] = {};         // bounds of the output points (as k_bounds takes them)
};
int voxel_pass(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device, const dcreg_voxel_params *p,
               bool packed, VoxelResult &r, DeskewRun *dsk = nullptr, const GatherRun *gat = nullptr);
// voxel.hip: the kept voxel map of the whole map's points (dcreg_target_voxels_keep): every refusal of include/dcreg.h, then the pass's
// keying and sort, one lane per voxel for the records, the compaction and the lookup table; info may be null
int voxel_map_keep(dcreg_ctx *c, const dcreg_voxel_map_params *p, dcreg_voxel_map_info *info);
// voxel.hip: dcreg_voxel_downsample* (and dcreg_deskew* with a voxel block): the pass, then the copy of the output to the caller
int voxel_downsample_to(dcreg_ctx *c, int n_clouds, const float *xyz, const int64_t *off, int64_t stride, bool on_device, const dcreg_voxel_params *p,
                        float *out, int64_t capacity, int64_t *out_off, dcreg_voxel_info *info, DeskewRun *dsk = nullptr);
int launch_knn(dcreg_ctx *c, const GridDev &grid, const float4 *d_q, int64_t n, int k, double max_radius, const PoseArg *pose,
               int32_t *d_idx, float *d_d2, bool sweep = false);
// context.hip: the index of the n points at raw built into d, and the empty-space field of its grid
int build_index(dcreg_ctx *c, const float4 *raw, int64_t n, dcreg_ctx::IndexSet &d, double radius_hint, uint32_t *occupied_out, const double *box = nullptr);
int build_gap_field(dcreg_ctx *c, dcreg_ctx::IndexSet &d, double radius_hint);
// context.hip: the indices of n_t clouds at once, as pairs_build builds its targets' (one sort per pass over all of them; synchronises and
// launches do not grow with n_t).  Cloud t = the count[t] packed points from raw[first[t]] (count 0: none, no index), bounds in `words` (3 n_t
// minima, then 3 n_t maxima, ordered floats, all finite); radius_hint 0: cells from the density alone; max_cells: table budget per cloud.
// Fills grids[t] / built[t]; the arrays live in ps.  The grids carry no gap field and no owners: knn_search reads neither when they are null
int clouds_index_build(dcreg_ctx *c, dcreg_ctx::PairSet &ps, const float4 *raw, int n_t, const std::vector<int64_t> &count,
                       const std::vector<int64_t> &first, const std::vector<uint32_t> &words, double radius_hint, double max_cells,
                       std::vector<GridDev> &grids, std::vector<uint8_t> &built);
// ---- scratch.hip: what the passes over a cloud share (the outlier filter, the normals, the descriptors, the visibility filter, the 1-NN
// engines, the map updates).
// cloud_used_compact: used flags of the n packed points at `in` and their scan (n + 1 entries in c->cloud.used / upos) and ALL used points
// compacted into c->cloud.cpts (w = the input index); nothing is waited for.  cloud_index_used: that, then - when there are at least
// min_used used points - their index in c->cloud.idx (hint: the cell size follows it, 0 = from the density); waits for the stream for
// *n_used.  The build's last_build_capped word belongs to the target's builds: saved and restored here
int cloud_used_compact(dcreg_ctx *c, const float4 *in, int64_t n);
int cloud_index_used(dcreg_ctx *c, const float4 *in, int64_t n, double hint, int64_t min_used, int64_t *n_used);
// the compaction of the n packed points at `in` by keep flags and their exclusive scan: 3 floats per kept point to out3 and / or a packed
// point (w = the new index, as k_pack packs a cloud) to out4, the byte mask where wanted
int cloud_write_kept(dcreg_ctx *c, const float4 *in, int64_t n, const uint32_t *keep, const uint32_t *pos, float *out3, float4 *out4, uint8_t *mask);
// the tail of a filter call (dcreg_outlier_filter*, dcreg_visibility_filter*) behind its keep flags: the capacity refusal, the output and
// mask buffers sized, the flags' scan where the caller has not made it (scan), cloud_write_kept and the copies of points and mask to the
// caller, queued.  The caller adds its own copies and waits for the stream; n == 0: nothing but the refusal
int cloud_filter_finish(dcreg_ctx *c, const float4 *pts, int64_t n, const uint32_t *keep, uint32_t *pos, bool scan, int64_t n_out, int64_t capacity,
                        DevBuf<float> &out_buf, DevBuf<uint8_t> &mask_buf, float *out, uint8_t *mask, bool on_device);
// flag_s[p] = the flag of the point at sorted position p of an index, flag_r by original index (n + 1 entries, the last 0)
int flags_to_sorted(dcreg_ctx *c, const float4 *sorted, int64_t n, const uint32_t *flag_r, uint32_t *flag_s);
// the plus-scan of n uint32 on c->stream, exclusive (from 0) or inclusive; its temporary storage is c->sort_tmp
int scan_u32(dcreg_ctx *c, const uint32_t *in, uint32_t *out, size_t n, bool inclusive);
// the rings a walk of g needs to cover the ball of squared radius `bound`; -1: sweep the grid
int rings_for_bound(const GridDev &g, float bound);
// a[0 .. n) = v, queued
void fill_f32(dcreg_ctx *c, float *a, int64_t n, float v);
// the squared bound of a search radius as a float (0: unbounded, 3.0e38) and, given the grid, the rings its walk needs (-1: sweep)
struct SearchBound { float bound = 3.0e38f; int max_ring = -1; };
SearchBound search_bound(double search_radius, const GridDev *g);
// f(std::integral_constant<int, K>) for the neighbour-heap size K the kernels are instantiated for: the smallest of 8, 16, 32 that holds k
template <class F>
void with_heap_k(int k, F &&f) {
    if (k <= 8) f(std::integral_constant<int, 8>{});
    else if (k <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 32>{});
}
// ---- scratch.hip: the seam for caller memory.  Every input that arrives as host memory or as a device pointer
// and every output that goes back to either passes through these three.
// caller_order: a device-pointer input is read behind the legacy default stream (the rule and its reason stand at the definition).
// caller_rows: n rows of `width` used elements at `stride` become readable on c->stream at *dev - host rows are copied into `stage`
// ((n - 1) * stride + width elements; width == stride: whole records), device rows are ordered by caller_order and read in place.
// ordered: an earlier input of the same call has already made the stream wait (a call orders itself once).  n == 0 copies nothing.
// caller_out: `bytes` of a result to the caller's host or device buffer, queued on c->stream; the caller waits
int caller_order(dcreg_ctx *c);
int caller_in(dcreg_ctx *c, void *stage, const void *src, size_t bytes, bool on_device, bool ordered);
int caller_out(dcreg_ctx *c, void *dst, const void *src, size_t bytes, bool on_device);
template <typename T>
int caller_rows(dcreg_ctx *c, const T *rows, int64_t n, int64_t stride, int64_t width, bool on_device, DevBuf<T> &stage, const T **dev,
                bool ordered = false) {
    const size_t len = n > 0 ? (size_t)(n - 1) * (size_t)stride + (size_t)width : 0;     // (the last row's padding is not the caller's to give)
    if (!on_device && stage.ensure(c, len)) return DCREG_E_NOMEM;
    *dev = on_device ? rows : stage.data();
    return caller_in(c, stage.data(), rows, sizeof(T) * len, on_device, ordered);
}
// ---- outliers.hip: one call's filter over the n packed points at `in` (input order, w = the index).  map == null: the used points are
// compacted and indexed (cloud_index_used); otherwise the points ARE the map behind that index (all finite) and its grid is searched.  Leaves
// the scores in c->outl.score, the keep flags and their exclusive scan in c->outl.keep / pos (n + 1 entries) and the counts in r; waits for
// the stream.
struct OutlierResult {
    int64_t n_in = 0, n_finite = 0, n_sparse = 0, n_out = 0;
    double mean = 0.0, stddev = 0.0, threshold = 0.0;
};
int outlier_check(dcreg_ctx *c, const dcreg_outlier_params *p);      // the parameter refusals of include/dcreg.h
int outlier_pass(dcreg_ctx *c, const float4 *in, int64_t n, const dcreg_outlier_params *p, const dcreg_ctx::IndexSet *map, OutlierResult &r);
void outlier_info(dcreg_outlier_info *info, const OutlierResult &r);
// the kept points of the pass packed into c->outl.out4 as k_pack packs a cloud (w = the new index)
int outlier_write_packed(dcreg_ctx *c, const float4 *in, int64_t n, int64_t n_out);
// normals.hip: the parameter refusals of dcreg_normals (engine.cpp reaches it through dcreg_normal_params_check)
int normals_check(dcreg_ctx *c, const dcreg_normal_params *p);
// normals.hip, for features.hip: dcreg_normals of a cloud that is already indexed (q: its nq used points in cell order behind the grid g,
// w = the input index; nq = 0: no index, every used point sparse) - normals and curvature of the n input points into c->nrm.normal /
// curv, NaN where a point has none; waits for the stream
int normals_to_scratch(dcreg_ctx *c, const float4 *q, int64_t nq, const GridDev &g, int64_t n, int64_t n_used, const dcreg_normal_params *p,
                       dcreg_normal_info *info);
// normals.hip: the kept normals follow an update of the map ("normals_follow", include/dcreg.h).  normals_follow_wanted: asked BEFORE the
// update drops them (option on, normals kept, and kept by dcreg_target_normals_keep).  normals_follow_carry (a removal, beside k_crop_raw,
// before anything is swapped): the survivors' normals and reaches compacted by flag_r / pos_r into the alt arrays; false: out of memory,
// the normals will not follow.  normals_follow_update (after the update stands and the whole map's index is the active one): the carried
// entries are swapped in or the arrays grown, the cells of the points that came (added: n_added packed points) and went (old_raw: the n_old
// points of the map as it was, flag_r their keep flags) are marked, the dirty points found, compacted and refitted - or, past the
// threshold, everything recomputed.  On any failure the normals stay dropped.  carried: normals_follow_carry ran
struct FollowChange {
    const float4 *added = nullptr; int64_t n_added = 0;
    const float4 *old_raw = nullptr; const uint32_t *flag_r = nullptr; int64_t n_old = 0;
    bool carried = false;
};
bool normals_follow_wanted(const dcreg_ctx *c);
bool normals_follow_carry(dcreg_ctx *c, int64_t n_old, const uint32_t *flag_r, const uint32_t *pos_r, int64_t kept);
void normals_follow_update(dcreg_ctx *c, const FollowChange &ch);
// voxel.hip: the kept voxel map follows an update of the map ("voxels_follow", include/dcreg.h).  voxels_follow_wanted: asked BEFORE the
// update drops the member (option on, a member kept).  voxels_follow_update (after the update stands and the whole map's index is the
// active one; wanted = what voxels_follow_wanted answered): the voxels of the points that came or went are marked, the updated map's
// points in them gathered and reduced again, the other records carried and both runs merged into the alternate arrays - or, past the
// threshold, the full keep; the member is restored on success.  On any failure it stays dropped, as map_changed left it; !wanted: the
// info says so and nothing else happens
bool voxels_follow_wanted(const dcreg_ctx *c);
void voxels_follow_update(dcreg_ctx *c, const FollowChange &ch, bool wanted);
// visibility.hip: one call's votes.  visibility_prepare checks parameters and members on the host (every refusal of include/dcreg.h before
// anything is queued; poses == null: range images only) and cuts the members into batches; visibility_votes leaves through / observed of
// the n packed points at `pts` in c->vis (by_w: point i counts at index w_i - a map in cell order); visibility_flags writes the keep flags
// of the decision (n + 1 entries, the last 0) and reads the counts back: it waits for the stream
struct VisRun {
    dcreg_visibility_params p{};
    std::vector<VisMember> members;        // the non-empty members, batch after batch
    std::vector<int64_t> batch;            // batch b = members [batch[b], batch[b + 1]); its images: n_img[b], its stored points: n_pts[b]
    std::vector<int64_t> n_img, n_pts;
    int64_t n_members = 0;                 // members of the call, the empty ones among them
};
struct VisResult {
    int64_t n_in = 0, n_finite = 0, n_observed = 0, n_flagged = 0, n_out = 0, n_members = 0;
};
int visibility_prepare(dcreg_ctx *c, int64_t n_members, const int64_t *ids, const double *poses, const dcreg_visibility_params *p, VisRun &v);
int visibility_votes(dcreg_ctx *c, const float4 *pts, int64_t n, bool by_w, const VisRun &v);
int visibility_flags(dcreg_ctx *c, const float4 *pts, int64_t n, const VisRun &v, uint32_t *keep, VisResult &r);
void visibility_info(dcreg_visibility_info *info, const VisResult &r);
// context.hip: the gathered points become the target as dcreg_set_target (p == null: a non-finite point refuses) or dcreg_set_target_voxel
// takes a cloud - packed into c->d_aligned by the gather or by the voxel pass behind it, then the commit of the plain calls
int set_target_gathered(dcreg_ctx *c, const GatherRun &g, const dcreg_voxel_params *p, double radius_hint, dcreg_voxel_info *info);
}  // namespace dcreg
