// Device seam of the C-ABI (include/dcreg.h): owns HBM buffers, the spatial index and the launches.
// Replaces ICPContext::setTargetCloud (DCReg/include/utils.hpp:393-424) and the per-iteration body of
// Point2PlaneICP_SO3_OpenMP up to AtA/Atb (DCReg/src/icp_test_runner.cpp:1704-1919).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "../../../include/dcreg_debug.h"
#include "context.hpp"
#include "kernels.hpp"

namespace dcreg {

constexpr double kCountScale = 67108864.0;      // 2^26 (search.hpp LinArgs::count_scale)
constexpr size_t kSearchCountBytes = 64 * kCounterStride * sizeof(uint32_t);     // 64 counters, one per 128-byte line
static void drop_warm(dcreg_ctx *c);

// ------------------------------------------------------------------------------------------ index build
static int sort_pairs_u32(dcreg_ctx *c, uint32_t *keys_in, uint32_t *keys_out, uint32_t *vals_in, uint32_t *vals_out, size_t n, int bits) {
    size_t tmp = 0;
    HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, n, 0, bits, c->stream));
    if (c->sort_tmp.ensure(c, tmp) != DCREG_OK) return DCREG_E_NOMEM;
    HIP_TRY(c, rocprim::radix_sort_pairs(c->sort_tmp.data(), tmp, keys_in, keys_out, vals_in, vals_out, n, 0, bits, c->stream));
    return DCREG_OK;
}
// sorts by the bits [lo_bit, hi_bit) of the keys only (stable: equal prefixes keep their order)
static int sort_pairs_u64(dcreg_ctx *c, uint64_t *keys_in, uint64_t *keys_out, uint32_t *vals_in, uint32_t *vals_out, size_t n, int lo_bit = 0, int hi_bit = 63) {
    size_t tmp = 0;
    HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, n, lo_bit, hi_bit, c->stream));
    if (c->sort_tmp.ensure(c, tmp) != DCREG_OK) return DCREG_E_NOMEM;
    HIP_TRY(c, rocprim::radix_sort_pairs(c->sort_tmp.data(), tmp, keys_in, keys_out, vals_in, vals_out, n, lo_bit, hi_bit, c->stream));
    return DCREG_OK;
}

// bounding box of a cloud the caller handed over in HOST memory, for clouds small enough that a loop over them costs less than the
// kernel + copy + stream synchronise of device_bounds (a frame of a few thousand points: the per-registration path)
static void host_bounds(const float *xyz, int64_t n, int64_t stride, double mn[3], double mx[3]) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n; ++i) {
        const float *p = xyz + i * stride;
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]);
            if (!(std::fabs(p[a]) <= 3.4e38f)) hi[0] = INFINITY;       // (a NaN compares false everywhere: make it visible, as k_bounds does)
        }
    }
    for (int a = 0; a < 3; ++a) { mn[a] = lo[a]; mx[a] = hi[a]; }
}

// (dsk: the counts of a deskew that packed the cloud come back with the bounds)
static int device_bounds(dcreg_ctx *c, const float4 *pts, int64_t n, double mn[3], double mx[3], DeskewRun *dsk = nullptr) {
    uint32_t init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    HIP_TRY(c, hipMemcpyAsync(c->d_scratch.data(), init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    const unsigned nb = std::min<unsigned>(blocks(n, 256), 256);      // grid-stride: one block per CU is plenty
    hipLaunchKernelGGL(k_bounds, dim3(nb), dim3(256), 0, c->stream, pts, n, c->d_scratch.data());
    uint32_t out[6];
    HIP_TRY(c, hipMemcpyAsync(out, c->d_scratch.data(), sizeof(out), hipMemcpyDeviceToHost, c->stream));
    if (dsk) if (int rc = deskew_readback(c, *dsk)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int a = 0; a < 3; ++a) { mn[a] = ord2f(out[a]); mx[a] = ord2f(out[3 + a]); }
    return DCREG_OK;
}

using IndexSet = dcreg_ctx::IndexSet;

// builds keys/sort/cell_start of the n points at raw into d (sorted, cell_start, grid, n_cells) for the given cell edge; returns number
// of occupied cells (sx = x sub-cells per cell, GridDev::sx; *occupied then counts sub-cells)
static int build_grid_at(dcreg_ctx *c, const float4 *raw, int64_t n, IndexSet &d, double h, const double mn[3], const double mx[3], uint32_t *occupied,
                         int sx = 1) {
    GridDev g{};
    g.h = h; g.inv_h = 1.0 / h;
    g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
    g.nx = (int)std::floor((mx[0] - mn[0]) * g.inv_h) + 1;
    g.ny = (int)std::floor((mx[1] - mn[1]) * g.inv_h) + 1;
    g.nz = (int)std::floor((mx[2] - mn[2]) * g.inv_h) + 1;
    g.sx = sx;
    const int64_t n_cells = (int64_t)g.nx * sx * g.ny * g.nz;       // table entries
    g.n_pts = (uint32_t)n;
    c->index_epoch += 1;           // d.sorted is about to be reallocated or rewritten
    if (c->d_keys.ensure(c, (size_t)n) || c->d_keys2.ensure(c, (size_t)n) || c->d_vals.ensure(c, (size_t)n) || c->d_vals2.ensure(c, (size_t)n) ||
        d.cell_start.ensure(c, (size_t)n_cells + 1) || d.sorted.ensure(c, (size_t)n + kPtsPad))
        return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_cell_keys, dim3(blocks(n, 256)), dim3(256), 0, c->stream, raw, n, g, c->d_keys.data(), c->d_vals.data());
    int bits = 1;
    while (((int64_t)1 << bits) < n_cells && bits < 32) ++bits;
    int rc = sort_pairs_u32(c, c->d_keys.data(), c->d_keys2.data(), c->d_vals.data(), c->d_vals2.data(), (size_t)n, bits);
    if (rc) return rc;
    hipLaunchKernelGGL(k_gather4, dim3(blocks(n, 256)), dim3(256), 0, c->stream, raw, c->d_vals2.data(), n, d.sorted.data());
    HIP_TRY(c, hipMemsetAsync(d.sorted.data() + n, 0, kPtsPad * sizeof(float4), c->stream));   // tail padding
    HIP_TRY(c, hipMemsetAsync(c->d_scratch.data(), 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_cell_start, dim3(blocks(n_cells + 1, 256)), dim3(256), 0, c->stream, c->d_keys2.data(), n, n_cells, d.cell_start.data(),
                       c->d_scratch.data());
    HIP_TRY(c, hipMemcpyAsync(occupied, c->d_scratch.data(), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    g.cell_start = d.cell_start.data();
    g.pts = d.sorted.data();
    d.grid = g;
    d.n_cells = n_cells / sx;
    return DCREG_OK;
}

static double cap_cell_for_budget(double h, const double mn[3], const double mx[3], double max_cells) {
    // enlarge h until the dense grid fits the cell budget
    for (int it = 0; it < 64; ++it) {
        const double nx = std::floor((mx[0] - mn[0]) / h) + 1, ny = std::floor((mx[1] - mn[1]) / h) + 1, nz = std::floor((mx[2] - mn[2]) / h) + 1;
        if (nx * ny * nz <= max_cells && nx < 2e9 && ny < 2e9 && nz < 2e9) return h;
        h *= 1.26;
    }
    return h;
}

// the index of the n points at raw, built into d (build_grid_at); box = the cloud's bounds min xyz, max xyz when the caller has them
// already, else NULL
int build_index(dcreg_ctx *c, const float4 *raw, int64_t n, IndexSet &d, double radius_hint, uint32_t *occupied_out, const double *box) {
    if (n <= 0) { c->fail("cloud is empty"); return DCREG_E_INVALID; }
    double mn[3], mx[3];
    int rc = DCREG_OK;
    if (box) for (int a = 0; a < 3; ++a) { mn[a] = box[a]; mx[a] = box[3 + a]; }
    else rc = device_bounds(c, raw, n, mn, mx);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a) if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) { c->fail("target cloud has non-finite coordinates"); return DCREG_E_INVALID; }
    const double ext = std::max({mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2], 1e-6});
    // The cell table is DENSE (one uint32 per x sub-cell of the bounding box): on a device with 288 GB of HBM a table of 2^30 entries (4 GB:
    // a 700 m x 700 m x 12 m prior map at 0.25 m cells, two x sub-cells each) is cheaper than any indirection on the search's critical path.
    // Rounds 1-5 capped it at 2^27 entries and enlarged the cell edge beyond that - a 50 M-point map then got 0.4 m cells without x
    // sub-cells and three times the candidates per query.  The cap is an option ("max_table_entries", at most 2^31: table indices are
    // 32-bit in the kernels); beyond it the cell edge still grows.
    const double max_cells = (double)c->opt_max_table_entries;
    // the radius caps the cell edge (slightly above R so that one ring already covers the radius)
    const double h_cap = radius_hint > 0.0 ? radius_hint * 1.00001 : ext / std::cbrt((double)n) * 4.0;
    uint32_t occ = 0;
    double h = c->opt_cell > 0.0 ? c->opt_cell : h_cap;
    // (how far the table budget pushed the cell edge beyond what radius and density ask for, and whether it took the x sub-cells: dcreg_ctx::whole_capped)
    c->last_build_capped = false;
    double cap_ratio = 1.0;
    {
        const double h0 = h;
        h = cap_cell_for_budget(h, mn, mx, max_cells);
        cap_ratio = h / h0;
    }
    rc = build_grid_at(c, raw, n, d, h, mn, mx, &occ);
    if (rc) return rc;
    if (c->opt_cell <= 0.0) {
        // density-adaptive cell: aim at `target_occ` points per occupied cell (surface data: occupancy ~ h^2)
        const double target_occ = 1.59 * c->opt_cell_factor * c->opt_cell_factor;   // = rho*h^2 at h = factor * r5
        double m1 = (double)n / std::max<uint32_t>(occ, 1);
        double h1 = h, expo = 2.0;
        for (int pass = 0; pass < 2 && m1 > target_occ * 1.3; ++pass) {
            double h2 = h1 * std::pow(target_occ / m1, 1.0 / expo);
            h2 = std::max(h2, h_cap / 64.0);
            {
                const double h20 = h2;
                h2 = cap_cell_for_budget(h2, mn, mx, max_cells);
                cap_ratio = h2 / h20;                              // (the last pass decides the cell edge)
            }
            if (h2 >= h1 * 0.95) break;
            rc = build_grid_at(c, raw, n, d, h2, mn, mx, &occ);
            if (rc) return rc;
            const double m2 = (double)n / std::max<uint32_t>(occ, 1);
            if (m2 < m1 && h2 < h1) expo = std::min(3.0, std::max(1.0, std::log(m1 / m2) / std::log(h1 / h2)));
            h1 = h2; m1 = m2;
        }
    }
    if (occupied_out) *occupied_out = occ;
    // the cell edge is settled: cut x into sub-cells (same rows, same table loads, tighter candidate runs), as far as the
    // table budget allows
    int sx = c->opt_x_subdiv;
    while (sx > 1 && (double)d.grid.nx * sx * d.grid.ny * d.grid.nz > max_cells) sx >>= 1;
    // one step of the budget (x 1.26) with sub-cells left is what a 50 M-point, 700 m map gets: a window of its own has nothing to add there
    // (measured, window forced: 0.79 against 0.73 ms per registration); two steps, or no sub-cells at all, is where the window pays (100 M points: 0.93 -> 0.76 ms)
    c->last_build_capped = cap_ratio > 1.5 || (sx == 1 && c->opt_x_subdiv > 1 && cap_ratio > 1.0);
    if (sx > 1) {
        uint32_t occ_sub = 0;
        rc = build_grid_at(c, raw, n, d, d.grid.h, mn, mx, &occ_sub, sx);
        if (rc) return rc;
    }
    return DCREG_OK;
}

// empty-space distance field of the grid of d (queries far from any point skip the rings they know are empty)
int build_gap_field(dcreg_ctx *c, IndexSet &d, double radius_hint) {
    GridDev &g = d.grid;
    g.gap = nullptr; g.gap_cap = 0; g.owner = nullptr;
    if (!c->opt_gap_field) return DCREG_OK;
    const int64_t n_cells = d.n_cells;
    int rings = 1;                                            // rings that a search up to the radius can need
    while (rings < 12 && (double)rings * g.h < (radius_hint > 0.0 ? radius_hint : 4.0 * g.h)) ++rings;
    if (rings < 2) return DCREG_OK;                           // one ring covers the radius: nothing to skip
    if (d.gap.ensure(c, (size_t)n_cells) || d.owner.ensure(c, (size_t)n_cells)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_gap_init, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, d.cell_start.data(), n_cells, g.sx, d.gap.data(), d.owner.data());
    for (int r = 1; r <= rings; ++r)
        hipLaunchKernelGGL(k_gap_dilate, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, d.gap.data(), d.owner.data(), g.nx, g.ny, g.nz, r);
    if (c->opt_far_bound) {      // the probe's owners: nearest DENSE cell (kernels.hpp k_gap_init_dense); scratch of this block only
        DevBuf<uint8_t> gap2;
        DevBuf<uint32_t> own2;
        if (gap2.alloc((size_t)n_cells) == hipSuccess && own2.alloc((size_t)n_cells) == hipSuccess) {
            hipLaunchKernelGGL(k_gap_init_dense, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, d.cell_start.data(), g.nx, n_cells, g.sx, 6u,
                               gap2.data(), own2.data());
            for (int r = 1; r <= rings; ++r)
                hipLaunchKernelGGL(k_gap_dilate, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, gap2.data(), own2.data(), g.nx, g.ny, g.nz, r);
            hipLaunchKernelGGL(k_owner_merge, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, d.owner.data(), own2.data(), n_cells);
        } else {
            (void)hipGetLastError();     // (no memory for the scratch: the plain owners serve)
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    g.gap = d.gap.data(); g.gap_cap = rings;
    g.owner = c->opt_far_bound ? d.owner.data() : nullptr;
    return DCREG_OK;
}

// row occupancy words of the grid of d (GridDev::ymask): what the searches of the linearisation sweep instead of walking rings
static int build_row_words(dcreg_ctx *c, IndexSet &d) {
    GridDev &g = d.grid;
    g.ymask = nullptr;
    g.nxb = (g.nx + 15) >> 4; g.nyw = (g.ny + 31) >> 5;
    const int64_t n_words = (int64_t)g.nz * g.nxb * g.nyw;
    if (d.ymask.ensure(c, (size_t)n_words)) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_ymask, dim3(blocks(n_words, 256)), dim3(256), 0, c->stream, d.cell_start.data(), g.nx, g.ny, g.nz, g.sx, g.nxb, g.nyw,
                       d.ymask.data());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    g.ymask = d.ymask.data();
    return DCREG_OK;
}

// ------------------------------------------------------------------------------------------ the window index of a large map (context.hpp)
static void swap_index(dcreg_ctx *c) {
    std::swap(c->map, c->roi_store);
    c->roi_active = !c->roi_active;
    c->index_epoch += 1;
    drop_warm(c);                 // the states' positions are positions in the other index's order
    c->order_valid = false;
    c->last_pose_valid = false;
}

int roi_deactivate(dcreg_ctx *c) {
    if (c && c->roi_active) swap_index(c);
    return DCREG_OK;
}

// bounding box of the source at a pose: the box of the eight corners of its body-frame box
static void source_box_at(const dcreg_ctx *c, const double *R, const double *t, double lo[3], double hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = 1e300; hi[a] = -1e300; }
    for (int k = 0; k < 8; ++k) {
        const double p[3] = {(k & 1) ? c->src_mx[0] : c->src_mn[0], (k & 2) ? c->src_mx[1] : c->src_mn[1], (k & 4) ? c->src_mx[2] : c->src_mn[2]};
        for (int a = 0; a < 3; ++a) {
            const double w = R[a * 3] * p[0] + R[a * 3 + 1] * p[1] + R[a * 3 + 2] * p[2] + t[a];
            lo[a] = std::min(lo[a], w); hi[a] = std::max(hi[a], w);
        }
    }
}
// every query of a linearisation at this pose, and the ball of the search radius around it, lies inside the window's box
static bool roi_covers(const dcreg_ctx *c, const double *R, const double *t, double pad) {
    double lo[3], hi[3];
    source_box_at(c, R, t, lo, hi);
    for (int a = 0; a < 3; ++a) {
        if (!(lo[a] - pad >= c->roi_lo[a] && hi[a] + pad <= c->roi_hi[a])) return false;      // (also false for a NaN pose)
    }
    return true;
}
static bool roi_wanted(const dcreg_ctx *c) { return c->opt_roi_index == 2 || (c->opt_roi_index == 1 && c->whole_capped); }
// what a linearisation at this search radius needs of the window beyond its transformed source's box
static double roi_pad_for(const dcreg_ctx *c, double search_radius) {
    return std::max(search_radius, c->radius_hint) * (1.0 + c->opt_cert_margin) * 1.001 + 1e-3;
}
// R (9) and t (3) of n poses are all finite numbers
static bool poses_finite(int n, const double *R9, const double *t3) { return finite_n(R9, 9 * (int64_t)n) && finite_n(t3, 3 * (int64_t)n); }

// A single-pose linearisation at (R, t) with this search radius is about to be queued: make the index it should search the active one -
// the window if the map wants one (building it around the pose when there is none that covers it), the whole map otherwise.
int roi_ensure(dcreg_ctx *c, const double *R, const double *t, double search_radius) {
    if (!roi_wanted(c)) return roi_deactivate(c);
    const double pad = roi_pad_for(c, search_radius);
    if (c->roi_built && pad <= c->roi_pad && roi_covers(c, R, t, pad)) {
        if (c->roi_empty) return roi_deactivate(c);
        if (!c->roi_active) swap_index(c);
        return DCREG_OK;
    }
    // ---- a new window around this pose
    (void)roi_deactivate(c);                                        // map is the whole map
    c->roi_built = false;                                           // (from here on no box describes the window: a failed build leaves none)
    HIP_TRY(c, hipStreamSynchronize(c->stream));                    // (nothing in flight reads the buffers that are about to be replaced)
    double lo[3], hi[3], blo[3], bhi[3];
    source_box_at(c, R, t, lo, hi);
    for (int a = 0; a < 3; ++a) {
        blo[a] = lo[a] - pad - c->opt_roi_margin; bhi[a] = hi[a] + pad + c->opt_roi_margin;
        // a pose that is not a pose (linearize_begin refuses those; a NaN pose leaves the inverted +-1e300 box): the whole map, no window
        if (!(std::isfinite(blo[a]) && std::isfinite(bhi[a]) && blo[a] <= bhi[a] && std::fabs(lo[a]) < 1e300 && std::fabs(hi[a]) < 1e300)) return DCREG_OK;
    }
    for (int a = 0; a < 3; ++a) { c->roi_lo[a] = blo[a]; c->roi_hi[a] = bhi[a]; }
    c->roi_pad = pad;
    c->roi_empty = false;
    // the map's points in the box: the x-runs of the whole map's (y,z) rows that cross it - contiguous ranges of its cell-sorted points (every cell
    // the box touches is taken whole: a few points more than the box holds, all of them the map's), read through the whole map's OWN index,
    // i.e. a pass over the window and not over the map
    const int64_t n = c->map.n;
    const GridDev &g = c->map.grid;
    int c0[3], c1[3];                                   // cell ranges [c0, c1) of the box in the whole map's grid
    const double org[3] = {g.ox, g.oy, g.oz};
    const int dims[3] = {g.nx, g.ny, g.nz};
    for (int a = 0; a < 3; ++a) {
        const double f0 = std::floor((c->roi_lo[a] - org[a]) * g.inv_h) - 1.0, f1 = std::floor((c->roi_hi[a] - org[a]) * g.inv_h) + 2.0;    // (one cell of slack: float cell keys)
        c0[a] = (int)std::min(std::max(f0, 0.0), (double)dims[a]); c1[a] = (int)std::min(std::max(f1, 0.0), (double)dims[a]);
    }
    const int ny_box = c1[1] - c0[1], nz_box = c1[2] - c0[2];
    const int64_t n_rows64 = (int64_t)ny_box * nz_box;
    uint32_t count = 0;
    c->roi_rebuilds += 1;
    if (c1[0] > c0[0] && n_rows64 > 0 && n_rows64 < ((int64_t)1 << 30)) {
        const int n_rows = (int)n_rows64, nxs = g.nx * g.sx, x0s = c0[0] * g.sx, x1s = c1[0] * g.sx;
        if (c->d_vals.ensure(c, (size_t)n_rows) || c->d_vals2.ensure(c, (size_t)n_rows)) return DCREG_E_NOMEM;
        uint32_t *vals = c->d_vals.data(), *vals2 = c->d_vals2.data();
        hipLaunchKernelGGL(k_roi_rows, dim3(blocks(n_rows, 256)), dim3(256), 0, c->stream, g.cell_start, nxs, g.ny, x0s, x1s, c0[1], ny_box, c0[2], n_rows, vals);
        if (int rc = scan_u32(c, vals, vals2, (size_t)n_rows, false)) return rc;
        uint32_t last[2] = {0u, 0u};
        HIP_TRY(c, hipMemcpyAsync(&last[0], vals + (n_rows - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&last[1], vals2 + (n_rows - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        count = last[0] + last[1];
        if (count != 0u && (int64_t)count < n) {
            if (c->roi_store.raw.ensure(c, (size_t)count)) return DCREG_E_NOMEM;
            hipLaunchKernelGGL(k_roi_copy, dim3((unsigned)n_rows), dim3(256), 0, c->stream, g.pts, g.cell_start, nxs, g.ny, x0s, x1s, c0[1], ny_box, c0[2], vals2,
                               c->roi_store.raw.data());
            HIP_TRY(c, hipGetLastError());
        }
    }
    if (count == 0u || (int64_t)count >= n) {        // nothing of the map in the box / all of it: the whole map's index serves inside this box
        c->roi_built = true; c->roi_empty = true;
        return DCREG_OK;
    }
    c->roi_store.n = (int64_t)count;
    swap_index(c);                                                  // map is the window's now (its buffers of the last build are reused)
    IndexSet &m = c->map;
    int rc = build_index(c, m.raw.data(), m.n, m, c->radius_hint * (1.0 + c->opt_cert_margin), &m.occupied);
    if (rc == DCREG_OK) rc = build_gap_field(c, m, c->radius_hint * (1.0 + c->opt_cert_margin));
    if (rc == DCREG_OK) rc = build_row_words(c, m);
    if (rc != DCREG_OK) { swap_index(c); return rc; }               // (the whole map stays usable)
    c->roi_built = true;
    return DCREG_OK;
}

// grid over the body-frame source cloud (backward pass of dcreg_p2p_error); built lazily, once per source
int build_aux_index(dcreg_ctx *c) {
    if (c->aux_valid) return DCREG_OK;
    int rc = build_index(c, c->d_src_raw.data(), c->n_src, c->aux, c->radius_hint, nullptr);
    if (rc) return rc;
    c->aux_valid = true;
    return DCREG_OK;
}

// Entry points that queue work on the stream, wait for it, or free / replace buffers refuse while a linearisation is queued or in flight:
// behind a gated launch they would wait for a gate nobody can open meanwhile, and a pending launch still reads the clouds and states.
int refuse_in_flight(dcreg_ctx *c) {
    if (c->gate_slot >= 0) { c->fail("a gated linearisation still waits for its pose (dcreg_linearize_gate_open / _gate_abort first)"); return DCREG_E_STATE; }
    for (const LinSlot &S : c->slots) if (S.pending) { c->fail("a linearisation is still in flight"); return DCREG_E_STATE; }
    if (c->nicp.batch_pending()) { c->fail("a batched normal linearisation is still in flight (dcreg_normals_batch_end first)"); return DCREG_E_STATE; }
    return DCREG_OK;
}

// a frame from a host buffer small enough for the registration path (icp_test_runner.cpp:442-461): staged through pinned memory, bounds on the
// host, no stream synchronise in dcreg_set_source
static bool small_host_frame(int64_t n, int64_t stride) { return n <= 65536 && n * stride <= (int64_t)1 << 20; }

int upload_cloud(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, DevBuf<float4> &raw, DeskewRun *dsk,
                 const GatherRun *gat) {
    if (gat) {                 // the records are gathered from the keyframe store (keyframes.hip: k_kf_gather packs)
        if (n != gat->n || n < 0 || n >= ((int64_t)1 << 31)) { c->fail("invalid gather arguments"); return DCREG_E_INVALID; }
        if (raw.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
        return n == 0 ? DCREG_OK : gather_queue(c, *gat, raw.data(), nullptr);
    }
    if (!xyz || n < 0 || stride < 3) { c->fail("invalid cloud arguments"); return DCREG_E_INVALID; }
    if (n >= ((int64_t)1 << 31)) { c->fail("cloud too large (%lld points)", (long long)n); return DCREG_E_INVALID; }
    if (!(dsk && dsk->out3) && raw.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
    if (n == 0) return DCREG_OK;
    if (dsk) if (int rc = deskew_reserve(c, *dsk)) return rc;
    const float *src = xyz;
    if (!on_device) {
        if (c->d_stage.ensure(c, (size_t)(n * stride))) return DCREG_E_NOMEM;
        const float *from = xyz;
        const size_t words = (size_t)(n * stride);
        if (small_host_frame(n, stride)) {
            // through the context's own pinned block: safe for pageable, pinned and registered buffers alike, and the
            // copy engine reads pinned memory without the runtime's staging pass
            if (words > c->h_stage.cap()) {
                if (c->h_stage) { HIP_TRY(c, hipStreamSynchronize(c->stream)); c->h_stage.reset(); c->h_stage_busy = false; }
                HIP_TRY(c, c->h_stage.alloc(words, hipHostMallocDefault));
            }
            if (!c->h_stage_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->h_stage_ev, hipEventDisableTiming));
            if (c->h_stage_busy) { HIP_TRY(c, hipEventSynchronize(c->h_stage_ev)); c->h_stage_busy = false; }   // (the previous frame's upload: long done)
            std::memcpy(c->h_stage.data(), xyz, sizeof(float) * words);
            from = c->h_stage.data();
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_stage.data(), from, sizeof(float) * words, hipMemcpyHostToDevice, c->stream));
        if (from == c->h_stage.data()) { HIP_TRY(c, hipEventRecord(c->h_stage_ev, c->stream)); c->h_stage_busy = true; }
        src = c->d_stage.data();
    } else if (int rc = caller_order(c)) return rc;
    if (dsk) return deskew_queue(c, src, n, stride, *dsk, dsk->out3 ? nullptr : raw.data());     // (deskew.hip: k_pack_deskew packs)
    hipLaunchKernelGGL(k_pack, dim3(blocks(n, 256)), dim3(256), 0, c->stream, src, n, stride, raw.data());
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

static int target_commit(dcreg_ctx *c, int64_t n, const double box[6], double radius_hint);
static int set_target(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, double radius_hint, bool on_device) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (n <= 0) { c->fail("target cloud is null or empty"); return DCREG_E_INVALID; }   // icp_test_runner.cpp:1643
    HIP_TRY(c, hipSetDevice(c->device));
    // packed and checked beside the current map (in the k-NN query buffer): a refused cloud leaves the map as it was
    int rc = upload_cloud(c, xyz, n, stride, on_device, c->d_aligned);
    if (rc) return rc;
    double box[6];
    rc = device_bounds(c, c->d_aligned.data(), n, box, box + 3);
    if (rc) return rc;
    for (int a = 0; a < 6; ++a) if (!std::isfinite(box[a])) { c->fail("target cloud has non-finite coordinates"); return DCREG_E_INVALID; }
    return target_commit(c, n, box, radius_hint);
}

// the checked cloud of n points in c->d_aligned.data() (packed as k_pack packs it), with bounds box = {min xyz, max xyz}, becomes the target
static int target_commit(dcreg_ctx *c, int64_t n, const double box[6], double radius_hint) {
    int rc;
    (void)roi_deactivate(c);             // the new map goes into the whole map's buffers; a window of the old one means nothing
    c->roi_built = false; c->whole_capped = false;
    IndexSet &m = c->map;
    m.raw.swap(c->d_aligned);
    m.n = n;
    c->radius_hint = radius_hint;
    // the cells are sized for the SEARCH radius (make_lin_args): one ring must cover it
    rc = build_index(c, m.raw.data(), n, m, radius_hint * (1.0 + c->opt_cert_margin), &m.occupied, box);
    if (rc) { m.n = 0; return rc; }
    c->whole_capped = c->last_build_capped;
    for (int a = 0; a < 6; ++a) c->tgt_box[a] = box[a];
    c->build_per_cell = (double)n / (double)std::max<uint32_t>(m.occupied, 1u);
    rc = build_gap_field(c, m, radius_hint * (1.0 + c->opt_cert_margin));
    if (rc) { m.n = 0; return rc; }
    rc = build_row_words(c, m);
    if (rc) { m.n = 0; return rc; }
    drop_warm(c);            // positions and certificates refer to the old target
    c->nicp.kept = false;    // ... and the kept normals to the old map's points
    c->vmap.kept = false;    // ... and the kept voxel map
    c->vmap.follow = dcreg_voxels_follow_info{};
    c->nicp.follow = dcreg_normals_follow_info{};      // (a new map: no update of it yet)
    c->order_valid = false;  // ... and the cost estimate of the query groups to the old map
    c->last_pose_valid = false;
    c->n_batch_states = 0;
    return DCREG_OK;
}

// ------------------------------------------------------------------------------------------ updates of the resident map (dcreg_target_insert*, _crop)
// Points are appended to the map, or cut from it by a box, and the index follows in place: the grid is kept where it can serve (the merged
// path), and re-derived from the device-resident raw points where it cannot (rebuilt).  Every search is exact in any grid, so either way
// the map answers bitwise as dcreg_set_target of the updated cloud would.  A refused call changes nothing: everything is checked in scratch
// buffers first, and the arrays that replace the map's are allocated before the first of them is written.

static void update_info(dcreg_map_update *info, int64_t offered, int64_t added, int64_t removed, int64_t n_target, int rebuilt) {
    if (!info) return;
    info->n_offered = offered; info->n_added = added; info->n_removed = removed; info->n_target = n_target; info->rebuilt = rebuilt; info->reserved_ = 0;
}

// everything derived from the map as it was goes, as dcreg_set_target drops it
static void map_changed(dcreg_ctx *c) {
    c->index_epoch += 1;
    c->roi_built = false;
    drop_warm(c);
    c->nicp.kept = false;                              // (an update that follows them puts them back: normals.hip normals_follow_update)
    c->vmap.kept = false;                              // (an update that follows it puts it back: voxel.hip voxels_follow_update)
    c->nicp.follow = dcreg_normals_follow_info{c->map.n, 0, 0, 0, 0};
    c->order_valid = false;
    c->last_pose_valid = false;
    c->n_batch_states = 0;
    std::fill(c->frames.state_valid.begin(), c->frames.state_valid.end(), (uint8_t)0);
    kdtree_free(c->kd); c->kd = nullptr;
}

static void words_init(uint32_t w[kMwWords]) {
    for (int k = 0; k < kMwWords; ++k) w[k] = 0u;
    for (int a = 0; a < 3; ++a) { w[kMwMin + a] = 0xFFFFFFFFu; w[kMwCellMin + a] = 0xFFFFFFFFu; }
    w[kMwKeyMin] = 0xFFFFFFFFu;
}

static int64_t box_cells(const MapBox &b) { return (int64_t)(b.x1 - b.x0) * (b.y1 - b.y0) * (b.z1 - b.z0); }
static MapBox box_grow(const MapBox &b, int r, const GridDev &g) {
    return MapBox{std::max(b.x0 - r, 0), std::max(b.y0 - r, 0), std::max(b.z0 - r, 0), std::min(b.x1 + r, g.nx), std::min(b.y1 + r, g.ny), std::min(b.z1 + r, g.nz)};
}
// the cells of a change (words kMwCellMin .. : cell + 1) and one more in x (the dense seeds look at their x neighbours' points)
static MapBox change_box(const uint32_t w[kMwWords], const GridDev &g) {
    MapBox S{(int)w[kMwCellMin] - 1, (int)w[kMwCellMin + 1] - 1, (int)w[kMwCellMin + 2] - 1, (int)w[kMwCellMax], (int)w[kMwCellMax + 1], (int)w[kMwCellMax + 2]};
    S.x0 = std::max(S.x0 - 1, 0); S.x1 = std::min(S.x1 + 1, g.nx);
    return S;
}
// scratch the fields of a change need (before the first write of an update)
static int fields_reserve(dcreg_ctx *c, const MapBox &S) {
    const GridDev &g = c->map.grid;
    if (!g.gap) return DCREG_OK;
    const MapBox E = box_grow(S, 2 * g.gap_cap, g);
    const size_t ne = (size_t)box_cells(E);
    if (c->d_fgap.ensure(c, 2 * ne) || c->d_fown.ensure(c, 2 * ne)) return DCREG_E_NOMEM;
    return DCREG_OK;
}
// row words and fields of the cells a change can reach, recomputed from the updated table (k_ymask_box, k_gap_*_box)
static void fields_local(dcreg_ctx *c, const MapBox &S) {
    const GridDev &g = c->map.grid;
    if (g.ymask) {
        const int xb0 = S.x0 >> 4, xb1 = (S.x1 + 15) >> 4, yw0 = S.y0 >> 5, yw1 = (S.y1 + 31) >> 5;
        const int64_t nw = (int64_t)(xb1 - xb0) * (yw1 - yw0) * (S.z1 - S.z0);
        hipLaunchKernelGGL(k_ymask_box, dim3(blocks(nw, 256)), dim3(256), 0, c->stream, g.cell_start, g.nx, g.ny, g.sx, g.nxb, g.nyw,
                           xb0, xb1 - xb0, yw0, yw1 - yw0, S.z0, S.z1 - S.z0, c->map.ymask.data());
    }
    if (!g.gap) return;
    const int rings = g.gap_cap;
    const MapBox B = box_grow(S, rings, g), E = box_grow(B, rings, g);
    const int64_t ne = box_cells(E), nb = box_cells(B);
    uint8_t *gap_p = c->d_fgap.data(), *gap_d = gap_p + ne;
    uint32_t *own_p = c->d_fown.data(), *own_d = own_p + ne;
    hipLaunchKernelGGL(k_gap_init_box, dim3(blocks(ne, 256)), dim3(256), 0, c->stream, g.cell_start, g.nx, g.ny, g.sx, E, 0, 0u, gap_p, own_p);
    for (int r = 1; r <= rings; ++r)
        hipLaunchKernelGGL(k_gap_dilate_box, dim3(blocks(ne, 256)), dim3(256), 0, c->stream, gap_p, own_p, g.nx, g.ny, E, r);
    if (g.owner) {
        hipLaunchKernelGGL(k_gap_init_box, dim3(blocks(ne, 256)), dim3(256), 0, c->stream, g.cell_start, g.nx, g.ny, g.sx, E, 1, 6u, gap_d, own_d);
        for (int r = 1; r <= rings; ++r)
            hipLaunchKernelGGL(k_gap_dilate_box, dim3(blocks(ne, 256)), dim3(256), 0, c->stream, gap_d, own_d, g.nx, g.ny, E, r);
    }
    hipLaunchKernelGGL(k_gap_store_box, dim3(blocks(nb, 256)), dim3(256), 0, c->stream, gap_p, own_p, g.owner ? own_d : (const uint32_t *)nullptr,
                       g.nx, g.ny, E, B, c->map.gap.data(), c->map.owner.data());
}

static int count_occupied(dcreg_ctx *c, const GridDev &g, int64_t n_cells, uint32_t *out) {
    HIP_TRY(c, hipMemsetAsync(c->d_scratch.data(), 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_count_occupied, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, g.cell_start, n_cells, g.sx, c->d_scratch.data());
    HIP_TRY(c, hipMemcpyAsync(out, c->d_scratch.data(), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

// The map's raw points (c->map.n of them, index order) are final and bounded by c->tgt_box: derive the grid anew, over that box enlarged by
// "map_grow_margin" on each side in x and y - not in z: a ground vehicle's map is flat, and z slack would multiply the dense table of a
// wide, flat map (12 m of height grown by 20 m on each side is 4.3 x the entries) and push it past its budget into coarser cells.  A point
// that leaves the box in z re-derives the grid again.  keep_edge: the current cell edge and x sub-cells where the table budget allows
// them (one key sort); otherwise - or when it does not - build_index's rules.  Built beside the current index (c->map_alt, and fields
// allocated beside the current ones where these are too small) and swapped in at the end; *swapped tells whether that happened (a
// failure before it leaves the current index standing).
static int map_rebuild(dcreg_ctx *c, bool keep_edge, bool *swapped) {
    *swapped = false;
    const double m[3] = {c->opt_map_grow_margin, c->opt_map_grow_margin, 0.0};
    double box[6];
    for (int a = 0; a < 3; ++a) { box[a] = c->tgt_box[a] - m[a]; box[3 + a] = c->tgt_box[3 + a] + m[a]; }
    uint32_t occ = 0;
    IndexSet &cur = c->map, &alt = c->map_alt;
    const GridDev &g = cur.grid;
    bool capped = c->whole_capped, built = false;
    if (keep_edge) {
        double dims[3], entries = (double)g.sx;
        for (int a = 0; a < 3; ++a) { dims[a] = std::floor((box[3 + a] - box[a]) * g.inv_h) + 1.0; entries *= dims[a]; }
        if (entries <= (double)c->opt_max_table_entries && dims[0] < 2e9 && dims[1] < 2e9 && dims[2] < 2e9) {
            int rc = build_grid_at(c, cur.raw.data(), cur.n, alt, g.h, box, box + 3, &occ, g.sx);
            if (rc) return rc;
            rc = count_occupied(c, alt.grid, alt.n_cells, &occ);
            if (rc) return rc;
            built = true;
        }
    }
    if (!built) {
        int rc = build_index(c, cur.raw.data(), cur.n, alt, c->radius_hint * (1.0 + c->opt_cert_margin), &occ, box);
        if (rc) return rc;
        capped = c->last_build_capped;
    }
    // the fields of the new grid (the current index keeps reading the current ones until the swap)
    const GridDev &g2 = alt.grid;
    const size_t n_words = (size_t)g2.nz * (size_t)((g2.nx + 15) >> 4) * (size_t)((g2.ny + 31) >> 5), n_cells2 = (size_t)alt.n_cells;
    const char *why = "while re-deriving the map's grid";
    DevBuf<uint8_t> gap;
    DevBuf<uint32_t> owner, ymask;
    if ((!cur.ymask.holds(n_words) && ymask.ensure(c, n_words, why)) ||
        (c->opt_gap_field && !cur.gap.holds(n_cells2) && gap.ensure(c, n_cells2, why)) ||
        (c->opt_gap_field && !cur.owner.holds(n_cells2) && owner.ensure(c, n_cells2, why)))
        return DCREG_E_NOMEM;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ymask) cur.ymask = std::move(ymask);
    if (gap) cur.gap = std::move(gap);
    if (owner) cur.owner = std::move(owner);
    cur.sorted.swap(alt.sorted);
    cur.cell_start.swap(alt.cell_start);
    *swapped = true;
    cur.grid = alt.grid; cur.n_cells = alt.n_cells;
    cur.occupied = occ;
    c->whole_capped = capped;
    c->build_per_cell = (double)cur.n / (double)std::max<uint32_t>(occ, 1u);
    int rc = build_gap_field(c, cur, c->radius_hint * (1.0 + c->opt_cert_margin));
    if (rc == DCREG_OK) rc = build_row_words(c, cur);
    return rc;
}

// The appended points (c->d_map_new[0, n_add), w = their map indices; their keys and input ranks at keys / vals) go into the current grid.
static int map_merge(dcreg_ctx *c, uint32_t n_add, uint32_t *keys, uint32_t *vals, uint32_t *keys2, uint32_t *vals2, uint32_t *b, const uint32_t w[kMwWords]) {
    IndexSet &m = c->map;
    DevBuf<float4> &alt = c->map_alt.sorted;
    GridDev &g = m.grid;
    const int64_t n_old = m.n, n_new = n_old + n_add;
    const int64_t n_entries = (int64_t)g.nx * g.sx * g.ny * g.nz;
    const MapBox S = change_box(w, g);
    // ---- every allocation first
    if (m.raw.grow_keep(c, (size_t)n_new, (size_t)n_old) || alt.ensure(c, (size_t)n_new + kPtsPad) || fields_reserve(c, S))
        return DCREG_E_NOMEM;
    int bits = 1;
    while (((int64_t)1 << bits) < n_entries && bits < 32) ++bits;
    int rc = sort_pairs_u32(c, keys, keys2, vals, vals2, (size_t)n_add, bits);
    if (rc) return rc;
    // ---- from here on the map is rewritten
    c->index_epoch += 1;
    uint32_t *scratch = c->d_scratch.data();
    HIP_TRY(c, hipMemcpyAsync(m.raw.data() + n_old, c->d_map_new.data(), sizeof(float4) * n_add, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(scratch + kMwOccupied, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_map_bpos, dim3(blocks(n_add, 256)), dim3(256), 0, c->stream, keys2, n_add, g.cell_start, g.sx, b, scratch);
    hipLaunchKernelGGL(k_map_merge_old, dim3(blocks(n_old, 256)), dim3(256), 0, c->stream, m.sorted.data(), (uint32_t)n_old, b, n_add, alt.data());
    hipLaunchKernelGGL(k_map_merge_new, dim3(blocks(n_add, 256)), dim3(256), 0, c->stream, c->d_map_new.data(), vals2, b, n_add, alt.data());
    HIP_TRY(c, hipMemsetAsync(alt.data() + n_new, 0, kPtsPad * sizeof(float4), c->stream));
    const int64_t first = (int64_t)w[kMwKeyMin] + 1;       // entries up to the smallest new key keep their value
    if (first <= n_entries)
        hipLaunchKernelGGL(k_map_table_insert, dim3(blocks(n_entries - first + 1, 256)), dim3(256), 0, c->stream, m.cell_start.data(), first, n_entries,
                           keys2, n_add);
    m.sorted.swap(alt);
    m.n = n_new;
    g.pts = m.sorted.data(); g.n_pts = (uint32_t)n_new;
    fields_local(c, S);
    uint32_t occ_new = 0;
    HIP_TRY(c, hipMemcpyAsync(&occ_new, scratch + kMwOccupied, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    m.occupied += occ_new;
    return DCREG_OK;
}

// the whole map's index, whichever index is active (a refused or empty update must not swap them: that drops the states)
static const IndexSet &whole_map(const dcreg_ctx *c) { return c->roi_active ? c->roi_store : c->map; }

static int map_insert(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, bool from_source, const double *R, const double *t,
                      double min_spacing, dcreg_map_update *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (!R || !t || (!from_source && (!xyz || n < 0 || stride < 3)) || !std::isfinite(min_spacing)) { c->fail("invalid insert arguments"); return DCREG_E_INVALID; }
    if (!poses_finite(1, R, t)) { c->fail("the pose of an insert has non-finite entries"); return DCREG_E_INVALID; }
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    if (from_source && c->n_src <= 0) { c->fail("no source: dcreg_set_source first"); return DCREG_E_STATE; }
    const int64_t m = from_source ? c->n_src : n;
    if (m >= ((int64_t)1 << 31)) { c->fail("too many points (%lld)", (long long)m); return DCREG_E_INVALID; }
    const int64_t n_old = whole_map(c).n;
    if (m == 0) { update_info(info, 0, 0, 0, n_old, 0); return DCREG_OK; }
    HIP_TRY(c, hipSetDevice(c->device));
    const float4 *in = c->d_src_raw.data();
    if (!from_source) {
        int rc = upload_cloud(c, xyz, n, stride, on_device, c->d_aligned);
        if (rc) return rc;
        in = c->d_aligned.data();
    }
    const size_t m1 = (size_t)m + 1;
    if (c->d_map_q.ensure(c, (size_t)m) || c->d_map_new.ensure(c, (size_t)m) || c->d_upd.ensure(c, 6 * m1)) return DCREG_E_NOMEM;
    uint32_t *flag = c->d_upd.data(), *pos = flag + m1, *keys = pos + m1, *vals = keys + m1, *keys2 = vals + m1, *vals2 = keys2 + m1;
    uint32_t w[kMwWords];
    words_init(w);
    HIP_TRY(c, hipMemcpyAsync(c->d_scratch.data(), w, sizeof(w), hipMemcpyHostToDevice, c->stream));
    PoseArg P{};
    for (int k = 0; k < 9; ++k) P.R[k] = R[k];
    for (int k = 0; k < 3; ++k) P.t[k] = t[k];
    hipLaunchKernelGGL(k_map_transform, dim3(blocks(m, 256)), dim3(256), 0, c->stream, in, m, P, c->d_map_q.data(), c->d_scratch.data());
    const GridDev wg = whole_map(c).grid;
    const float *d2 = nullptr;
    float spacing_sq = 0.f;
    if (min_spacing > 0.0) {      // the map as it stood: dcreg_knn with k = 1 (the bound only has to reach the spacing)
        if (c->d_nn_idx.ensure(c, (size_t)m) || c->d_nn_d2.ensure(c, (size_t)m)) return DCREG_E_NOMEM;
        int rc = launch_knn(c, wg, c->d_map_q.data(), m, 1, min_spacing, nullptr, c->d_nn_idx.data(), c->d_nn_d2.data());
        if (rc) return rc;
        d2 = c->d_nn_d2.data();
        spacing_sq = (float)(min_spacing * min_spacing);
    }
    hipLaunchKernelGGL(k_map_keep, dim3(blocks((int64_t)m1, 256)), dim3(256), 0, c->stream, m, d2, spacing_sq, flag);
    if (int rc = scan_u32(c, flag, pos, m1, false)) return rc;
    hipLaunchKernelGGL(k_map_append, dim3(blocks(m, 256)), dim3(256), 0, c->stream, c->d_map_q.data(), m, flag, pos, (uint32_t)n_old, wg, c->d_map_new.data(),
                       keys, vals, c->d_scratch.data());
    uint32_t n_add = 0;
    HIP_TRY(c, hipMemcpyAsync(w, c->d_scratch.data(), sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&n_add, pos + m, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (w[kMwBad]) { c->fail("inserted points have non-finite coordinates"); return DCREG_E_INVALID; }
    if (n_old + (int64_t)n_add > (int64_t)INT32_MAX) { c->fail("the map would hold more than 2^31 - 1 points"); return DCREG_E_INVALID; }
    if (n_add == 0) { update_info(info, m, 0, 0, n_old, 0); return DCREG_OK; }     // everything thinned: nothing changes
    // ---- the map changes
    const bool follow = normals_follow_wanted(c), vfollow = voxels_follow_wanted(c);      // (asked before map_changed drops them)
    (void)roi_deactivate(c);
    double box[6];
    for (int a = 0; a < 3; ++a) {
        box[a] = std::min(c->tgt_box[a], (double)ord2f(w[kMwMin + a]));
        box[3 + a] = std::max(c->tgt_box[3 + a], (double)ord2f(w[kMwMax + a]));
    }
    int rebuilt = 0, rc = DCREG_OK;
    bool swapped = false;
    if (c->opt_map_update && !w[kMwOutside]) {
        rc = map_merge(c, n_add, keys, vals, keys2, vals2, flag, w);
        if (rc) return rc;
        for (int a = 0; a < 6; ++a) c->tgt_box[a] = box[a];
        map_changed(c);
        // the density the cell edge was sized for has doubled: derive the grid again (build_index's rules)
        if ((double)c->map.n / (double)std::max<uint32_t>(c->map.occupied, 1u) > 2.0 * c->build_per_cell) {
            rc = map_rebuild(c, false, &swapped);
            rebuilt = swapped ? 1 : 0;
            if (rc != DCREG_OK && !swapped) {
                // nothing was swapped in: the merged map stands, complete and exact, in the grid it had.  Short of memory that is the
                // result (the re-derivation only restores speed; the next update tries again); any other failure is reported
                if (rc != DCREG_E_NOMEM) return rc;
                (void)hipGetLastError();
                rc = DCREG_OK;
            }
        }
    } else {
        if (c->map.raw.grow_keep(c, (size_t)(n_old + n_add), (size_t)n_old)) return DCREG_E_NOMEM;
        HIP_TRY(c, hipMemcpyAsync(c->map.raw.data() + n_old, c->d_map_new.data(), sizeof(float4) * n_add, hipMemcpyDeviceToDevice, c->stream));
        const double old_box[6] = {c->tgt_box[0], c->tgt_box[1], c->tgt_box[2], c->tgt_box[3], c->tgt_box[4], c->tgt_box[5]};
        c->map.n = n_old + n_add;               // (the points beyond n_old are not read by the index as it was)
        for (int a = 0; a < 6; ++a) c->tgt_box[a] = box[a];
        rebuilt = 1;
        rc = map_rebuild(c, true, &swapped);
        if (rc != DCREG_OK && !swapped) {                               // nothing was swapped in: the old map stands
            c->map.n = n_old;
            for (int a = 0; a < 6; ++a) c->tgt_box[a] = old_box[a];
            return rc;
        }
        map_changed(c);
    }
    if (rc) { c->map.n = 0; c->vmap.follow = dcreg_voxels_follow_info{}; return rc; }         // (a failure after a rebuild swapped its grid in: the map is gone, as after a failed dcreg_set_target)
    FollowChange ch;
    ch.added = c->d_map_new.data(); ch.n_added = (int64_t)n_add;
    if (follow) normals_follow_update(c, ch);
    voxels_follow_update(c, ch, vfollow);
    update_info(info, m, n_add, 0, c->map.n, rebuilt);
    return DCREG_OK;
}

static int map_keep_flagged(dcreg_ctx *c, const char *none_kept, dcreg_map_update *info);
static int map_crop(dcreg_ctx *c, const double *lo, const double *hi, dcreg_map_update *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (!lo || !hi) { c->fail("invalid crop arguments"); return DCREG_E_INVALID; }
    for (int a = 0; a < 3; ++a) if (std::isnan(lo[a]) || std::isnan(hi[a])) { c->fail("the crop box has NaN bounds"); return DCREG_E_INVALID; }
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    const IndexSet &wm = whole_map(c);
    const int64_t n = wm.n;
    const size_t n1 = (size_t)n + 1;
    if (c->d_upd.ensure(c, 4 * n1)) return DCREG_E_NOMEM;
    uint32_t *flag_r = c->d_upd.data(), *flag_s = flag_r + 2 * n1;
    CropBox bx;
    for (int a = 0; a < 3; ++a) { bx.lo[a] = lo[a]; bx.hi[a] = hi[a]; }
    hipLaunchKernelGGL(k_crop_flags, dim3(blocks((int64_t)n1, 256)), dim3(256), 0, c->stream, wm.raw.data(), n, bx, flag_r);
    hipLaunchKernelGGL(k_crop_flags, dim3(blocks((int64_t)n1, 256)), dim3(256), 0, c->stream, wm.sorted.data(), n, bx, flag_s);
    return map_keep_flagged(c, "the crop box keeps no point of the map", info);
}

// The keep flags of the whole map's points are in c->d_upd (n + 1 entries each, the last 0): [0] in index order, [2 (n + 1)] in sorted
// order.  The kept points, renumbered in their old order, become the map (dcreg_target_crop, dcreg_target_remove_outliers); none_kept: the
// refusal's text when no flag is set
static int map_keep_flagged(dcreg_ctx *c, const char *none_kept, dcreg_map_update *info) {
    const IndexSet &wm = whole_map(c);
    const int64_t n = wm.n;
    const size_t n1 = (size_t)n + 1;
    uint32_t *flag_r = c->d_upd.data(), *pos_r = flag_r + n1, *flag_s = pos_r + n1, *pos_s = flag_s + n1;
    uint32_t w[kMwWords];
    words_init(w);
    HIP_TRY(c, hipMemcpyAsync(c->d_scratch.data(), w, sizeof(w), hipMemcpyHostToDevice, c->stream));
    if (int rc = scan_u32(c, flag_r, pos_r, n1, false)) return rc;
    if (int rc = scan_u32(c, flag_s, pos_s, n1, false)) return rc;
    hipLaunchKernelGGL(k_crop_scan_box, dim3(blocks(n, 256)), dim3(256), 0, c->stream, wm.sorted.data(), n, flag_s, wm.grid, c->d_scratch.data());
    uint32_t kept = 0;
    HIP_TRY(c, hipMemcpyAsync(w, c->d_scratch.data(), sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&kept, pos_r + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (kept == 0) { c->fail("%s", none_kept); return DCREG_E_INVALID; }
    if ((int64_t)kept == n) { update_info(info, n, 0, 0, n, 0); return DCREG_OK; }      // nothing outside the box: nothing changes
    // ---- the map changes
    (void)roi_deactivate(c);
    IndexSet &m = c->map, &alt = c->map_alt;
    GridDev &g = m.grid;
    double kbox[6];
    for (int a = 0; a < 3; ++a) { kbox[a] = ord2f(w[kMwMin + a]); kbox[3 + a] = ord2f(w[kMwMax + a]); }
    const int64_t n_entries = (int64_t)g.nx * g.sx * g.ny * g.nz;
    double kept_entries = (double)g.sx;
    for (int a = 0; a < 3; ++a) kept_entries *= std::floor((kbox[3 + a] - kbox[a] + (a < 2 ? 2.0 * c->opt_map_grow_margin : 0.0)) * g.inv_h) + 1.0;
    const bool rederive = !c->opt_map_update || kept_entries < 0.25 * (double)n_entries;
    const MapBox S = change_box(w, g);
    if (alt.raw.ensure(c, (size_t)kept) || (!rederive && (alt.sorted.ensure(c, (size_t)kept + kPtsPad) || fields_reserve(c, S))))
        return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_crop_raw, dim3(blocks(n, 256)), dim3(256), 0, c->stream, m.raw.data(), n, flag_r, pos_r, alt.raw.data());
    // the survivors' kept normals go the same way, beside the current ones (short of memory they will not follow: dropped as without the option)
    const bool follow = normals_follow_wanted(c) && normals_follow_carry(c, n, flag_r, pos_r, (int64_t)kept);
    const bool vfollow = voxels_follow_wanted(c);
    int rebuilt = 0, rc = DCREG_OK;
    bool swapped = false;
    if (rederive) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        m.raw.swap(alt.raw);
        const double old_box[6] = {c->tgt_box[0], c->tgt_box[1], c->tgt_box[2], c->tgt_box[3], c->tgt_box[4], c->tgt_box[5]};
        m.n = kept;
        for (int a = 0; a < 6; ++a) c->tgt_box[a] = kbox[a];
        rebuilt = 1;
        rc = map_rebuild(c, true, &swapped);
        if (rc != DCREG_OK && !swapped) {                               // nothing was swapped in: the old map stands
            m.raw.swap(alt.raw);
            m.n = n;
            for (int a = 0; a < 6; ++a) c->tgt_box[a] = old_box[a];
            return rc;
        }
    } else {
        hipLaunchKernelGGL(k_crop_sorted, dim3(blocks(n, 256)), dim3(256), 0, c->stream, m.sorted.data(), n, flag_s, pos_s, pos_r, alt.sorted.data());
        HIP_TRY(c, hipMemsetAsync(alt.sorted.data() + kept, 0, kPtsPad * sizeof(float4), c->stream));
        hipLaunchKernelGGL(k_crop_table, dim3(blocks(n_entries + 1, 256)), dim3(256), 0, c->stream, m.cell_start.data(), n_entries, pos_s);
        m.raw.swap(alt.raw);
        m.sorted.swap(alt.sorted);
        m.n = kept;
        g.pts = m.sorted.data(); g.n_pts = kept;
        for (int a = 0; a < 6; ++a) c->tgt_box[a] = kbox[a];
        fields_local(c, S);
        rc = count_occupied(c, g, m.n_cells, &m.occupied);
        if (rc == DCREG_OK) { const hipError_t e = hipGetLastError(); if (e != hipSuccess) { c->fail("crop: %s", hipGetErrorString(e)); rc = DCREG_E_DEVICE; } }
    }
    map_changed(c);
    if (rc) { m.n = 0; c->vmap.follow = dcreg_voxels_follow_info{}; return rc; }
    FollowChange ch;                                   // (the map as it was is in alt.raw since the swap, its keep flags still in c->d_upd)
    ch.old_raw = alt.raw.data(); ch.flag_r = flag_r; ch.n_old = n; ch.carried = true;
    if (follow) normals_follow_update(c, ch);
    voxels_follow_update(c, ch, vfollow);
    update_info(info, n, 0, n - kept, m.n, rebuilt);
    return DCREG_OK;
}

// dcreg_target_remove_outliers: the filter over the whole map's points through the map's own index (outliers.hip), the survivors through the
// update path of the crop.  Nothing of the context changes before the flags are known and some point goes.
static int map_remove_outliers(dcreg_ctx *c, const dcreg_outlier_params *p, dcreg_outlier_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = outlier_check(c, p)) return rc;
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    const IndexSet &wm = whole_map(c);
    const int64_t n = wm.n;
    const size_t n1 = (size_t)n + 1;
    OutlierResult r;
    int rc = outlier_pass(c, wm.raw.data(), n, p, &wm, r);
    if (rc) return rc;
    if (r.n_out == 0) { c->fail("the filter would remove every point of the map"); return DCREG_E_INVALID; }
    outlier_info(info, r);
    if (r.n_out == n) return DCREG_OK;               // nothing to remove: nothing changes
    if (c->d_upd.ensure(c, 4 * n1)) return DCREG_E_NOMEM;
    uint32_t *flag_r = c->d_upd.data(), *flag_s = flag_r + 2 * n1;
    HIP_TRY(c, hipMemcpyAsync(flag_r, c->outl.keep.data(), sizeof(uint32_t) * n1, hipMemcpyDeviceToDevice, c->stream));
    rc = flags_to_sorted(c, wm.sorted.data(), n, flag_r, flag_s);
    if (rc) return rc;
    return map_keep_flagged(c, "the filter would remove every point of the map", nullptr);
}

// dcreg_target_remove_dynamic: the visibility votes of the members over the whole map's points (visibility.hip), the survivors through the
// update path of the crop.  Nothing of the context changes before the flags are known and some point goes.
static int map_remove_dynamic(dcreg_ctx *c, int64_t n_members, const int64_t *ids, const double *poses, const dcreg_visibility_params *p,
                              dcreg_visibility_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    VisRun v;
    if (int rc = visibility_prepare(c, n_members, ids, poses, p, v)) return rc;
    if (!poses && n_members > 0) { c->fail("null member poses"); return DCREG_E_INVALID; }
    if (c->map.n <= 0) { c->fail("no target: dcreg_set_target first"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    const IndexSet &wm = whole_map(c);
    const int64_t n = wm.n;
    const size_t n1 = (size_t)n + 1;
    if (c->d_upd.ensure(c, 4 * n1)) return DCREG_E_NOMEM;
    uint32_t *flag_r = c->d_upd.data(), *flag_s = flag_r + 2 * n1;
    const bool cell_order = c->opt_visibility_order != 0;
    int rc = visibility_votes(c, cell_order ? wm.sorted.data() : wm.raw.data(), n, cell_order, v);
    if (rc) return rc;
    VisResult r;
    rc = visibility_flags(c, wm.raw.data(), n, v, flag_r, r);
    if (rc) return rc;
    if (r.n_out == 0) { c->fail("the votes would remove every point of the map"); return DCREG_E_INVALID; }
    visibility_info(info, r);
    if (r.n_out == n) return DCREG_OK;               // nothing to remove: nothing changes
    rc = flags_to_sorted(c, wm.sorted.data(), n, flag_r, flag_s);
    if (rc) return rc;
    return map_keep_flagged(c, "the votes would remove every point of the map", nullptr);
}

// dcreg_debug_index_check: the whole map's grid built from scratch (same origin, edge, dims, sub-cells) from its raw points, compared entry by entry
static int index_check(dcreg_ctx *c, int64_t mm[5]) {
    const IndexSet &wm = whole_map(c);
    const GridDev &g = wm.grid;
    const int64_t n = wm.n, n_cells = (int64_t)g.nx * g.ny * g.nz, n_entries = n_cells * g.sx;
    const int64_t n_words = (int64_t)g.nz * g.nxb * g.nyw;
    if (c->d_keys.ensure(c, (size_t)n) || c->d_keys2.ensure(c, (size_t)n) || c->d_vals.ensure(c, (size_t)n) || c->d_vals2.ensure(c, (size_t)n))
        return DCREG_E_NOMEM;
    // scratch of this check only
    DevBuf<float4> pts_b;
    DevBuf<uint32_t> tab_b, ym_b, own_b, own2_b;
    DevBuf<uint8_t> gap_b, gap2_b;
    DevBuf<unsigned long long> cnt_b;
    if (pts_b.alloc((size_t)(n + kPtsPad)) != hipSuccess || tab_b.alloc((size_t)(n_entries + 1)) != hipSuccess ||
        ym_b.alloc((size_t)std::max<int64_t>(n_words, 1)) != hipSuccess || own_b.alloc((size_t)n_cells) != hipSuccess ||
        own2_b.alloc((size_t)n_cells) != hipSuccess || gap_b.alloc((size_t)n_cells) != hipSuccess || gap2_b.alloc((size_t)n_cells) != hipSuccess ||
        cnt_b.alloc(5) != hipSuccess) {
        (void)hipGetLastError(); c->fail("no memory for the index check"); return DCREG_E_NOMEM;
    }
    float4 *pts = pts_b.data();
    uint32_t *tab = tab_b.data(), *ym = ym_b.data(), *own = own_b.data(), *own2 = own2_b.data();
    uint8_t *gap = gap_b.data(), *gap2 = gap2_b.data();
    unsigned long long *cnt = cnt_b.data();
    HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * 5, c->stream));
    hipLaunchKernelGGL(k_cell_keys, dim3(blocks(n, 256)), dim3(256), 0, c->stream, wm.raw.data(), n, g, c->d_keys.data(), c->d_vals.data());
    int bits = 1;
    while (((int64_t)1 << bits) < n_entries && bits < 32) ++bits;
    int rc = sort_pairs_u32(c, c->d_keys.data(), c->d_keys2.data(), c->d_vals.data(), c->d_vals2.data(), (size_t)n, bits);
    if (rc) return rc;
    hipLaunchKernelGGL(k_gather4, dim3(blocks(n, 256)), dim3(256), 0, c->stream, wm.raw.data(), c->d_vals2.data(), n, pts);
    HIP_TRY(c, hipMemsetAsync(pts + n, 0, kPtsPad * sizeof(float4), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_scratch.data(), 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_cell_start, dim3(blocks(n_entries + 1, 256)), dim3(256), 0, c->stream, c->d_keys2.data(), n, n_entries, tab, c->d_scratch.data());
    hipLaunchKernelGGL(k_count_diff<float4>, dim3(blocks(n + kPtsPad, 256)), dim3(256), 0, c->stream, (const float4 *)g.pts, (const float4 *)pts, n + kPtsPad, cnt);
    hipLaunchKernelGGL(k_count_diff<uint32_t>, dim3(blocks(n_entries + 1, 256)), dim3(256), 0, c->stream, g.cell_start, (const uint32_t *)tab, n_entries + 1, cnt + 1);
    if (g.ymask) {
        hipLaunchKernelGGL(k_ymask, dim3(blocks(n_words, 256)), dim3(256), 0, c->stream, tab, g.nx, g.ny, g.nz, g.sx, g.nxb, g.nyw, ym);
        hipLaunchKernelGGL(k_count_diff<uint32_t>, dim3(blocks(n_words, 256)), dim3(256), 0, c->stream, g.ymask, (const uint32_t *)ym, n_words, cnt + 2);
    }
    if (g.gap) {
        hipLaunchKernelGGL(k_gap_init, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, tab, n_cells, g.sx, gap, own);
        for (int r = 1; r <= g.gap_cap; ++r)
            hipLaunchKernelGGL(k_gap_dilate, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, gap, own, g.nx, g.ny, g.nz, r);
        if (g.owner) {
            hipLaunchKernelGGL(k_gap_init_dense, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, tab, g.nx, n_cells, g.sx, 6u, gap2, own2);
            for (int r = 1; r <= g.gap_cap; ++r)
                hipLaunchKernelGGL(k_gap_dilate, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, gap2, own2, g.nx, g.ny, g.nz, r);
            hipLaunchKernelGGL(k_owner_merge, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, own, own2, n_cells);
            hipLaunchKernelGGL(k_count_diff<uint32_t>, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, g.owner, (const uint32_t *)own, n_cells, cnt + 4);
        }
        hipLaunchKernelGGL(k_count_diff<uint8_t>, dim3(blocks(n_cells, 256)), dim3(256), 0, c->stream, g.gap, (const uint8_t *)gap, n_cells, cnt + 3);
    }
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    const hipError_t e0 = hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    const hipError_t e1 = hipStreamSynchronize(c->stream);
    HIP_TRY(c, e0); HIP_TRY(c, e1);
    HIP_TRY(c, hipGetLastError());
    for (int k = 0; k < 5; ++k) mm[k] = (int64_t)h[k];
    return DCREG_OK;
}

static int target_get(const dcreg_ctx *cc, float *out, int64_t capacity) {
    dcreg_ctx *c = const_cast<dcreg_ctx *>(cc);
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    const IndexSet &wm = whole_map(c);
    if (wm.n <= 0) { c->fail("no target"); return DCREG_E_STATE; }
    if (!out || capacity < wm.n) { c->fail("the output holds %lld points, the map %lld", (long long)capacity, (long long)wm.n); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->d_stage.ensure(c, (size_t)(3 * wm.n))) return DCREG_E_NOMEM;
    hipLaunchKernelGGL(k_unpack3, dim3(blocks(wm.n, 256)), dim3(256), 0, c->stream, wm.raw.data(), wm.n, c->d_stage.data());
    HIP_TRY(c, hipMemcpyAsync(out, c->d_stage.data(), sizeof(float) * (size_t)(3 * wm.n), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

// the curve frame of a source cloud (dcreg_set_source; the frames of dcreg_register_frames get exactly the same): key scale of its bounding
// box, and levels of the curve resolved - log8(n) levels + 4 (a 4096-fold finer grid than one point per cell): 27 key bits for an 8 k-point
// frame instead of 63, i.e. half the radix passes; points that share the prefix keep their input order (the sort is stable)
static void curve_frame(int64_t n, const double mn[3], const double mx[3], double &inv_q, int &levels) {
    const double ext = std::max({mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2], 1e-6});
    inv_q = 2097151.0 / ext * 0.999999;
    levels = 4;
    while (levels < 21 && ((int64_t)1 << (3 * (levels - 4))) < n) ++levels;
}

static int source_commit(dcreg_ctx *c, int64_t n, const double mn[3], const double mx[3], bool must_wait);
static int set_source(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (n <= 0) { c->fail("measure cloud is null or empty"); return DCREG_E_INVALID; }  // icp_test_runner.cpp:1635
    HIP_TRY(c, hipSetDevice(c->device));
    // packed and checked beside the current source (in the k-NN query buffer): a refused cloud leaves it as it was (dcreg_p2p_error reads it)
    int rc = upload_cloud(c, xyz, n, stride, on_device, c->d_aligned);
    if (rc) return rc;
    // Hilbert-curve order in the body frame (pose independent: a rigid motion keeps neighbours neighbours)
    double mn[3], mx[3];
    const bool small_host = !on_device && small_host_frame(n, stride);   // a frame from a host buffer: the registration path (icp_test_runner.cpp:442-461)
    if (small_host) {
        host_bounds(xyz, n, stride, mn, mx);
    } else {
        rc = device_bounds(c, c->d_aligned.data(), n, mn, mx);
        if (rc) return rc;
    }
    for (int a = 0; a < 3; ++a) if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) { c->fail("source cloud has non-finite coordinates"); return DCREG_E_INVALID; }
    return source_commit(c, n, mn, mx, !small_host);
}

// the checked cloud of n points in c->d_aligned.data() (packed as k_pack packs it), with bounds mn .. mx, becomes the source
static int source_commit(dcreg_ctx *c, int64_t n, const double mn[3], const double mx[3], bool must_wait) {
    int rc;
    c->gicp.src_kept = false;          // (the kept source normals belong to the points that go)
    c->d_src_raw.swap(c->d_aligned);
    for (int a = 0; a < 3; ++a) { c->src_mn[a] = mn[a]; c->src_mx[a] = mx[a]; }
    double inv_q;
    int levels;
    curve_frame(n, mn, mx, inv_q, levels);
    {   // farthest corner of the bounding box: no point is farther from the body-frame origin
        double r2 = 0.0;
        for (int k = 0; k < 3; ++k) { const double m = std::max(std::fabs(mn[k]), std::fabs(mx[k])); r2 += m * m; }
        c->src_radius = std::sqrt(r2);
    }
    if (c->d_mkeys.ensure(c, (size_t)n) || c->d_mkeys2.ensure(c, (size_t)n) ||
        c->d_vals.ensure(c, (size_t)n) || c->d_vals2.ensure(c, (size_t)n) ||
        c->d_src.ensure(c, (size_t)n))
        return DCREG_E_NOMEM;
    if (c->opt_keep_source_order) {      // experiments: the caller supplies the processing order
        HIP_TRY(c, hipMemcpyAsync(c->d_src.data(), c->d_src_raw.data(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    } else {
        // the curve is resolved as far as the cloud can tell cells apart (curve_frame)
        // (round 6: ONE workgroup ordering a frame of <= 8192 points in LDS - keys, bitonic sort, gather, a single launch - was built and
        //  measured: 35 us of host time instead of 39, and 120 us of DEVICE time in front of the first linearisation instead of 15; removed)
        hipLaunchKernelGGL(k_curve_keys, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->d_src_raw.data(), n, mn[0], mn[1], mn[2], inv_q, c->opt_curve_x_scale, c->d_mkeys.data(), c->d_vals.data());
        rc = sort_pairs_u64(c, c->d_mkeys.data(), c->d_mkeys2.data(), c->d_vals.data(), c->d_vals2.data(), (size_t)n, 63 - 3 * levels);
        if (rc) return rc;
        hipLaunchKernelGGL(k_gather4, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->d_src_raw.data(), c->d_vals2.data(), n, c->d_src.data());
    }
    // A small frame from a host buffer went through the context's pinned block (upload_cloud): the caller's buffer is consumed, whatever
    // kind of memory it is, and nothing has to be waited for - the first linearisation queues behind the sort, and a device fault surfaces
    // at that linearisation (include/dcreg.h says so).  Everything else is waited for here.
    if (must_wait) HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    c->n_src = n;
    {   // dispatch groups of the single-pose launches (kernels.hpp k_group_cost): multiples of 16 query blocks, at most kMaxGroups of them
        const uint32_t nb = blocks(n, kLinBlock);
        const uint32_t gq = 16u;                  // one XCD's run of query blocks (kXcdChunk)
        c->group_blocks = gq * std::max<uint32_t>(1u, (nb + gq * kMaxGroups - 1) / (gq * kMaxGroups));
        c->n_groups = std::min<uint32_t>(nb / c->group_blocks, (uint32_t)kMaxGroups);
        c->order_valid = false;                   // estimated at the pose of the next single-pose linearisation
    }
    c->aux_valid = false;
    drop_warm(c);
    c->n_batch_states = 0;
    c->last_pose_valid = false;
    return DCREG_OK;
}

// The frames of one dcreg_register_frames call (context.hpp FrameSet): checked (offsets, finite coordinates) before anything is queued,
// uploaded in ONE copy, each frame in its own curve frame (curve_frame of its bounding box, computed on the host as dcreg_set_source does for
// a frame from a host buffer) - one stable sort over (frame, key prefix) - and gathered so that every frame starts on a query-block boundary.
// Waits for the stream: the caller's buffer is consumed when this returns.
// (fs: the ctx's frames, or the sources of dcreg_register_pairs)
static int frames_load(dcreg_ctx *c, dcreg_ctx::FrameSet &fs, int n_frames, const float *xyz, const int64_t *off, int64_t stride) {
    if (!c) return DCREG_E_INVALID;
    if (n_frames < 0 || (n_frames > 0 && !off) || stride < 3) { c->fail("invalid frame arguments"); return DCREG_E_INVALID; }
    if (n_frames > 0 && off[0] != 0) { c->fail("frame offsets must start at 0"); return DCREG_E_INVALID; }
    for (int f = 0; f < n_frames; ++f)
        if (off[f + 1] < off[f]) { c->fail("frame offsets decrease at frame %d", f); return DCREG_E_INVALID; }
    const int64_t n = n_frames > 0 ? off[n_frames] : 0;
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    std::vector<FrameBox> box((size_t)std::max(n_frames, 1));
    std::vector<uint2> slice((size_t)n_frames);
    std::vector<uint32_t> dst((size_t)std::max(n_frames, 1));
    int64_t padded = 0, max_points = 0;
    int max_bits = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int64_t m = off[f + 1] - off[f];
        if (m >= ((int64_t)1 << 31)) { c->fail("frame %d too large (%lld points)", f, (long long)m); return DCREG_E_INVALID; }
        dst[(size_t)f] = (uint32_t)padded;
        slice[(size_t)f] = make_uint2((uint32_t)padded, (uint32_t)m);
        box[(size_t)f] = FrameBox{0.0, 0.0, 0.0, 1.0, 0ull};
        if (m > 0) {
            double mn[3], mx[3];
            host_bounds(xyz + off[f] * stride, m, stride, mn, mx);
            for (int a = 0; a < 3; ++a)
                if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) { c->fail("frame %d has non-finite coordinates", f); return DCREG_E_INVALID; }
            double inv_q;
            int levels;
            curve_frame(m, mn, mx, inv_q, levels);
            box[(size_t)f] = FrameBox{mn[0], mn[1], mn[2], inv_q, 0ull};
            if (!c->opt_keep_source_order) { box[(size_t)f].mask = (uint64_t)3 * levels; max_bits = std::max(max_bits, 3 * levels); }    // (bits; made a mask below)
        }
        padded += (m + kLinBlock - 1) / kLinBlock * kLinBlock;
        max_points = std::max(max_points, m);
        if (padded >= ((int64_t)1 << 31)) { c->fail("the frames of one call hold too many points (%lld)", (long long)padded); return DCREG_E_INVALID; }
    }
    int fbits = 0;
    while (((int64_t)1 << fbits) < (int64_t)n_frames) ++fbits;
    if (fbits + max_bits > 63) { c->fail("too many frames for one call at these frame sizes (%d key bits); split the call", fbits + max_bits); return DCREG_E_INVALID; }
    for (int f = 0; f < n_frames; ++f) {        // the frame's prefix bits, below the frame id
        const int bits = (int)box[(size_t)f].mask;
        box[(size_t)f].mask = bits > 0 ? (((uint64_t)1 << bits) - 1) << (63 - fbits - bits) : 0ull;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    fs.slice.clear(); fs.max_points = 0; fs.n_states = 0; fs.state_valid.clear();
    if (n > 0) {
        if (fs.raw.ensure(c, (size_t)n) || fs.src.ensure(c, (size_t)padded) || fs.d_off.ensure(c, (size_t)n_frames + 1) ||
            fs.d_dst.ensure(c, (size_t)n_frames) || fs.d_box.ensure(c, (size_t)n_frames) ||
            c->d_mkeys.ensure(c, (size_t)n) || c->d_mkeys2.ensure(c, (size_t)n) ||
            c->d_vals.ensure(c, (size_t)n) || c->d_vals2.ensure(c, (size_t)n))
            return DCREG_E_NOMEM;
        const float *staged = nullptr;                 // (whole records: the deskew fields live in them)
        if (int rc = caller_rows(c, xyz, n, stride, stride, false, c->d_stage, &staged)) return rc;
        HIP_TRY(c, hipMemcpyAsync(fs.d_off.data(), off, sizeof(int64_t) * ((size_t)n_frames + 1), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(fs.d_dst.data(), dst.data(), sizeof(uint32_t) * (size_t)n_frames, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(fs.d_box.data(), box.data(), sizeof(FrameBox) * (size_t)n_frames, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_pack, dim3(blocks(n, 256)), dim3(256), 0, c->stream, staged, n, stride, fs.raw.data());
        const uint32_t *order = nullptr;
        if (fbits + max_bits > 0) {
            hipLaunchKernelGGL(k_frame_keys, dim3(blocks(n, 256)), dim3(256), 0, c->stream, fs.raw.data(), n, fs.d_off.data(), n_frames, fs.d_box.data(), fbits,
                               c->opt_curve_x_scale, c->d_mkeys.data(), c->d_vals.data());
            const int rc = sort_pairs_u64(c, c->d_mkeys.data(), c->d_mkeys2.data(), c->d_vals.data(), c->d_vals2.data(), (size_t)n, 63 - fbits - max_bits);
            if (rc) return rc;
            order = c->d_vals2.data();
        }
        hipLaunchKernelGGL(k_frame_gather, dim3(blocks(n, 256)), dim3(256), 0, c->stream, fs.raw.data(), order, n, fs.d_off.data(), n_frames, fs.d_dst.data(), fs.src.data());
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    fs.slice = std::move(slice);
    fs.max_points = max_points;
    return DCREG_OK;
}

// the search bound of a launch: searches cover a little more than the gate radius (certificates of "5th neighbour beyond R" spend the
// difference); candidates with d2 < this are kept
static float search_bound_sq(const dcreg_ctx *c, double search_radius) {
    const double rs = search_radius * (1.0 + c->opt_cert_margin), r2 = rs * rs;
    float rf = (float)r2;
    if ((double)rf < r2) rf = std::nextafterf(rf, INFINITY);
    return std::nextafterf(rf, INFINITY);
}
// rings of cells of edge h that cover the search bound
static int rings_for(double h, float radius_sq_f) {
    int k = 1;
    while (k < 100000) {
        const double safe = (double)k * h * (1.0 - 1e-9);
        if (safe * safe * (1.0 - 1e-6) >= (double)radius_sq_f) break;
        ++k;
    }
    return k;
}

// ------------------------------------------------------------------------------------------ the targets of dcreg_register_pairs
// Device bytes a build batch of pair targets may take ("pairs_max_bytes"; 0 = a quarter of the device's free memory), and what a target of
// m points is counted at: the upload (stride floats a point), raw and sorted points, two key and two value arrays of the sort, and its cell
// table at the table budget ("pair_max_table_entries": the table is not known before the bounds are)
static double pairs_budget(dcreg_ctx *c) {
    if (c->opt_pairs_max_bytes > 0.0) return c->opt_pairs_max_bytes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 4.0e9; }
    return 0.25 * (double)free_b;
}
// (extra: further bytes per point - the 1-NN engines keep a float4 normal per target point and estimate it through 3 + 1 floats of scratch)
static double pair_target_bytes(const dcreg_ctx *c, int64_t m, int64_t stride, double extra = 0.0) {
    return m > 0 ? (double)m * (4.0 * (double)stride + 16.0 + 16.0 + 16.0 + 8.0 + extra) + 4.0 * (double)c->opt_pair_max_table_entries + 16.0 * kPtsPad : 0.0;
}
// ... and what a target of m points is counted at in a build batch of dcreg_register_pairs_voxels (voxel.hip pairs_voxels_build), which
// allocates no cell table.  Per point: the upload (stride floats), the packed point (16), its cloud and relative key (4 + 8), the head
// flags, their scan, the voxel starts, the keep flags and their scan (5 x 4), the sort's two key and two value arrays (2 x 8 + 2 x 4)
// and its own temporary storage, bounded by a further copy of keys and values and its digit counters (16).  Per voxel - a target has at
// most m of them: the records before compaction (48).  Per kept voxel - each holds at least min_points >= 2 points, so at most m / 2:
// its record (48), its key (8) and fewer than 4 table slots of 8 + 4 bytes (48), together at most 52 a point.  Per target, points or
// not: offsets, counters, bounds and its record (256 covers them).  This is the peak of a build; the packed points, the sort's arrays and
// the per-voxel scratch are scratch of the voxel pass (dcreg_ctx::vox) and are not read while the batch's pairs run, so what a batch
// holds then is below what it was planned with
static double pair_voxel_target_bytes(int64_t m, int64_t stride) {
    return 256.0 + (double)m * (4.0 * (double)stride + 16.0 + 12.0 + 20.0 + 24.0 + 16.0 + 48.0 + 52.0);
}

// One pass over some targets of the batch (J: batch targets, cells[j]: the geometry of J[j] in this pass): cell keys of all their points
// in one kernel, ONE sort over (pass target, cell).  occ != null: the occupied cells of every pass target (one readback).  Otherwise the
// final index: points gathered target after target (kPtsPad zero entries behind each), every cell table and every target's row words.
// (ps / raw: the set whose buffers the pass fills and the packed points it indexes - the pair targets, or the clouds of dcreg_normals_clouds)
static int pairs_pass(dcreg_ctx *c, dcreg_ctx::PairSet &ps, const float4 *raw, const std::vector<int> &J, std::vector<PairCells> &cells,
                      const std::vector<int64_t> &count, std::vector<uint32_t> *occ, std::vector<int64_t> *tab_first, std::vector<int64_t> *yw_first) {
    const int n_j = (int)J.size();
    std::vector<int64_t> offs((size_t)3 * (n_j + 1), 0);       // [pass points | table entries | row words] offsets
    int64_t *po = offs.data(), *to = po + (n_j + 1), *yo = to + (n_j + 1);
    int64_t max_entries = 1, pts = 0;
    for (int j = 0; j < n_j; ++j) {
        const PairCells &g = cells[(size_t)j];
        const int64_t entries = (int64_t)g.nx * g.sx * g.ny * g.nz;
        max_entries = std::max(max_entries, entries + 1);
        po[j + 1] = po[j] + count[(size_t)J[(size_t)j]];
        to[j + 1] = to[j] + entries + 1;
        yo[j + 1] = yo[j] + (int64_t)g.nz * g.nxb * g.nyw;
        cells[(size_t)j].pts_first = pts;
        pts += count[(size_t)J[(size_t)j]] + kPtsPad;
    }
    const int64_t n = po[n_j];
    int cbits = 1, jbits = 0;
    while (((int64_t)1 << cbits) < max_entries) ++cbits;
    while (((int64_t)1 << jbits) < (int64_t)n_j) ++jbits;
    if (ps.d_off.ensure(c, offs.size()) || ps.d_cells.ensure(c, (size_t)n_j) || ps.d_words.ensure(c, (size_t)n_j) ||
        c->d_mkeys.ensure(c, (size_t)n) || c->d_mkeys2.ensure(c, (size_t)n) ||
        c->d_vals.ensure(c, (size_t)n) || c->d_vals2.ensure(c, (size_t)n))
        return DCREG_E_NOMEM;
    if (!occ && (ps.sorted.ensure(c, (size_t)pts) || ps.table.ensure(c, (size_t)to[n_j]) ||
                 ps.ymask.ensure(c, (size_t)std::max<int64_t>(yo[n_j], 1))))
        return DCREG_E_NOMEM;
    int64_t *d_po = ps.d_off.data(), *d_to = d_po + (n_j + 1), *d_yo = d_to + (n_j + 1);
    HIP_TRY(c, hipMemcpyAsync(ps.d_off.data(), offs.data(), sizeof(int64_t) * offs.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ps.d_cells.data(), cells.data(), sizeof(PairCells) * (size_t)n_j, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pairs_keys, dim3(blocks(n, 256)), dim3(256), 0, c->stream, raw, n, d_po, n_j, ps.d_cells.data(), cbits, c->d_mkeys.data(), c->d_vals.data());
    int rc = sort_pairs_u64(c, c->d_mkeys.data(), c->d_mkeys2.data(), c->d_vals.data(), c->d_vals2.data(), (size_t)n, 0, cbits + jbits);
    if (rc) return rc;
    if (occ) {
        HIP_TRY(c, hipMemsetAsync(ps.d_words.data(), 0, sizeof(uint32_t) * (size_t)n_j, c->stream));
        hipLaunchKernelGGL(k_pairs_occupancy, dim3(blocks(n, 256)), dim3(256), 0, c->stream, c->d_mkeys2.data(), n, cbits, ps.d_words.data());
        occ->assign((size_t)n_j, 0u);
        HIP_TRY(c, hipMemcpyAsync(occ->data(), ps.d_words.data(), sizeof(uint32_t) * (size_t)n_j, hipMemcpyDeviceToHost, c->stream));
    } else {
        hipLaunchKernelGGL(k_pairs_gather, dim3(blocks(n, 256)), dim3(256), 0, c->stream, raw, c->d_vals2.data(), n, d_po, n_j, ps.d_cells.data(), ps.sorted.data());
        hipLaunchKernelGGL(k_pairs_pad, dim3((unsigned)n_j), dim3(64), 0, c->stream, d_po, ps.d_cells.data(), ps.sorted.data());
        hipLaunchKernelGGL(k_pairs_table, dim3(blocks(to[n_j], 256)), dim3(256), 0, c->stream, c->d_mkeys2.data(), d_po, d_to, n_j, cbits, ps.table.data());
        if (yo[n_j] > 0)
            hipLaunchKernelGGL(k_pairs_ymask, dim3(blocks(yo[n_j], 256)), dim3(256), 0, c->stream, ps.table.data(), d_to, d_yo, n_j, ps.d_cells.data(), ps.ymask.data());
        tab_first->assign(to, to + n_j);
        yw_first->assign(yo, yo + n_j);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the host arrays above are the sources of the copies)
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

// The indices of n_t clouds at once (pairs_build below; normals.hip: the clouds of dcreg_normals_clouds).  Cloud t = the count[t] packed
// points from raw[first[t]] (count 0: no index), its bounds in `words` as k_pairs_pack leaves them (3 n_t minima, then 3 n_t maxima, ordered
// floats; all finite).  radius_hint > 0 caps the cell edge as build_index does, 0 starts from the density; max_cells = the table budget per
// cloud.  Fills grids[t] and built[t] for every indexed cloud; the arrays live in ps (sorted, table, ymask).  No gap field and no owners.
int clouds_index_build(dcreg_ctx *c, dcreg_ctx::PairSet &ps, const float4 *raw, int n_t, const std::vector<int64_t> &count,
                       const std::vector<int64_t> &first, const std::vector<uint32_t> &words, double radius_hint, double max_cells,
                       std::vector<GridDev> &grids, std::vector<uint8_t> &built) {
    grids.assign((size_t)n_t, GridDev{});
    built.assign((size_t)n_t, 0);
    // ---- every target's cell edge, as build_index chooses it
    struct Plan { double mn[3], mx[3], h_cap, h1, m1, expo; bool adapt; int nx, ny, nz; };
    std::vector<Plan> plan((size_t)n_t);
    auto geom = [](Plan &P, double h) {
        const double inv_h = 1.0 / h;
        P.nx = (int)std::floor((P.mx[0] - P.mn[0]) * inv_h) + 1;
        P.ny = (int)std::floor((P.mx[1] - P.mn[1]) * inv_h) + 1;
        P.nz = (int)std::floor((P.mx[2] - P.mn[2]) * inv_h) + 1;
    };
    auto cells_of = [&](int t, double h, int sx) {
        Plan &P = plan[(size_t)t];
        geom(P, h);
        PairCells g{};
        g.ox = P.mn[0]; g.oy = P.mn[1]; g.oz = P.mn[2]; g.inv_h = 1.0 / h;
        g.nx = P.nx; g.ny = P.ny; g.nz = P.nz; g.sx = sx;
        g.raw_first = first[(size_t)t];
        g.nxb = (g.nx + 15) >> 4; g.nyw = (g.ny + 31) >> 5;
        return g;
    };
    std::vector<int> J;
    std::vector<PairCells> cells;
    for (int t = 0; t < n_t; ++t) {
        const int64_t m = count[(size_t)t];
        if (m <= 0) continue;
        Plan &P = plan[(size_t)t];
        for (int a = 0; a < 3; ++a) { P.mn[a] = ord2f(words[(size_t)3 * t + a]); P.mx[a] = ord2f(words[(size_t)3 * n_t + 3 * t + a]); }
        const double ext = std::max({P.mx[0] - P.mn[0], P.mx[1] - P.mn[1], P.mx[2] - P.mn[2], 1e-6});
        P.h_cap = radius_hint > 0.0 ? radius_hint * 1.00001 : ext / std::cbrt((double)m) * 4.0;
        P.h1 = cap_cell_for_budget(c->opt_cell > 0.0 ? c->opt_cell : P.h_cap, P.mn, P.mx, max_cells);
        P.expo = 2.0; P.adapt = c->opt_cell <= 0.0;
        J.push_back(t);
        cells.push_back(cells_of(t, P.h1, 1));
    }
    std::vector<uint32_t> occ;
    int rc = DCREG_OK;
    if (!J.empty() && c->opt_cell <= 0.0) {
        // density-adaptive cells (build_index): the occupancy at the first edge, then up to two passes over the targets that ask for one
        rc = pairs_pass(c, ps, raw, J, cells, count, &occ, nullptr, nullptr);
        if (rc) return rc;
        const double target_occ = 1.59 * c->opt_cell_factor * c->opt_cell_factor;
        std::vector<double> h2s;
        for (size_t j = 0; j < J.size(); ++j) { Plan &P = plan[(size_t)J[j]]; P.m1 = (double)count[(size_t)J[j]] / std::max<uint32_t>(occ[j], 1u); }
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<int> K;
            cells.clear(); h2s.clear();
            for (int t : J) {
                Plan &P = plan[(size_t)t];
                if (!P.adapt || !(P.m1 > target_occ * 1.3)) { P.adapt = false; continue; }
                double h2 = P.h1 * std::pow(target_occ / P.m1, 1.0 / P.expo);
                h2 = std::max(h2, P.h_cap / 64.0);
                h2 = cap_cell_for_budget(h2, P.mn, P.mx, max_cells);
                if (h2 >= P.h1 * 0.95) { P.adapt = false; continue; }
                K.push_back(t); h2s.push_back(h2);
                cells.push_back(cells_of(t, h2, 1));
            }
            if (K.empty()) break;
            rc = pairs_pass(c, ps, raw, K, cells, count, &occ, nullptr, nullptr);
            if (rc) return rc;
            for (size_t k = 0; k < K.size(); ++k) {
                Plan &P = plan[(size_t)K[k]];
                const double h2 = h2s[k], m2 = (double)count[(size_t)K[k]] / std::max<uint32_t>(occ[k], 1u);
                if (m2 < P.m1 && h2 < P.h1) P.expo = std::min(3.0, std::max(1.0, std::log(P.m1 / m2) / std::log(P.h1 / h2)));
                P.h1 = h2; P.m1 = m2;
            }
        }
    }
    // ---- the final index: the settled edge, x cut into sub-cells as far as the table budget allows
    cells.clear();
    for (int t : J) {
        Plan &P = plan[(size_t)t];
        geom(P, P.h1);
        int sx = c->opt_x_subdiv;
        while (sx > 1 && (double)P.nx * sx * P.ny * P.nz > max_cells) sx >>= 1;
        cells.push_back(cells_of(t, P.h1, sx));
    }
    if (!J.empty()) {
        std::vector<int64_t> tab_first, yw_first;
        rc = pairs_pass(c, ps, raw, J, cells, count, nullptr, &tab_first, &yw_first);
        if (rc) return rc;
        for (size_t j = 0; j < J.size(); ++j) {
            const int t = J[j];
            const PairCells &q = cells[j];
            const double h = plan[(size_t)t].h1;
            GridDev &g = grids[(size_t)t];
            g.h = h; g.inv_h = q.inv_h;
            g.ox = q.ox; g.oy = q.oy; g.oz = q.oz;
            g.nx = q.nx; g.ny = q.ny; g.nz = q.nz; g.sx = q.sx;
            g.n_pts = (uint32_t)count[(size_t)t];
            g.cell_start = ps.table.data() + tab_first[j];
            g.pts = ps.sorted.data() + q.pts_first;
            g.gap = nullptr; g.gap_cap = 0; g.owner = nullptr;
            g.ymask = ps.ymask.data() + yw_first[j]; g.nxb = q.nxb; g.nyw = q.nyw;
            built[(size_t)t] = 1;
        }
    }
    return DCREG_OK;
}

// The targets of one build batch (xyz: HOST memory, target t = points [off[t], off[t + 1]), off[0] = 0), each indexed as dcreg_set_target
// with radius hint `search_radius` would index it alone - build_index's rules: the radius caps the cell edge, the table budget
// ("pair_max_table_entries", per target) enlarges it, the density adaptation shrinks it, x sub-cells as far as the budget allows - all of
// them at once: ONE upload, ONE segmented pack / finiteness / bounds pass and ONE readback, then passes over all targets (ONE sort each):
// the occupancy at the first cell edge, at most two adaptation passes over the targets that ask for one, the final index.  No gap field and
// no owners (GridDev::gap = owner = null).  The searches are exact in any cells, so the sums are those of the target's
// own index.  The synchronises and launches do not grow with the number of targets.  DCREG_E_INVALID: a non-finite coordinate.
static int pairs_build(dcreg_ctx *c, int n_t, const float *xyz, const int64_t *off, int64_t stride, double search_radius) {
    dcreg_ctx::PairSet &ps = c->pairs;
    if (n_t < 0 || !off || stride < 3 || off[0] != 0 || !(search_radius > 0.0)) { c->fail("invalid pair target arguments"); return DCREG_E_INVALID; }
    ps.n = 0;
    ps.built.assign((size_t)n_t, 0);
    ps.normals_kept = false;                     // (the kept normals of the 1-NN engines belong to the batch that was built)
    ps.grids.clear(); ps.off.clear();
    const int64_t n = n_t > 0 ? off[n_t] : 0;
    if (n > 0 && !xyz) { c->fail("null point buffer"); return DCREG_E_INVALID; }
    if (n >= ((int64_t)1 << 31)) { c->fail("the pair targets of one build batch hold too many points (%lld)", (long long)n); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (ps.d_grids.ensure(c, (size_t)std::max(n_t, 1)) || ps.d_words.ensure(c, (size_t)6 * std::max(n_t, 1)) ||
        ps.d_off.ensure(c, (size_t)3 * (n_t + 1)))
        return DCREG_E_NOMEM;
    std::vector<PairGrid> grids((size_t)n_t);
    std::memset(grids.data(), 0, sizeof(PairGrid) * (size_t)n_t);
    std::vector<int64_t> count((size_t)n_t);
    for (int t = 0; t < n_t; ++t) count[(size_t)t] = off[t + 1] - off[t];
    std::vector<uint32_t> words((size_t)6 * n_t);
    if (n > 0) {
        const float *staged = nullptr;
        if (ps.raw.ensure(c, (size_t)n)) return DCREG_E_NOMEM;
        if (int rc = caller_rows(c, xyz, n, stride, stride, false, c->d_stage, &staged)) return rc;
        HIP_TRY(c, hipMemcpyAsync(ps.d_off.data(), off, sizeof(int64_t) * (size_t)(n_t + 1), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(ps.d_words.data(), 0xFF, sizeof(uint32_t) * 3 * (size_t)n_t, c->stream));
        HIP_TRY(c, hipMemsetAsync(ps.d_words.data() + 3 * (size_t)n_t, 0, sizeof(uint32_t) * 3 * (size_t)n_t, c->stream));
        hipLaunchKernelGGL(k_pairs_pack, dim3(blocks(n, 256)), dim3(256), 0, c->stream, staged, n, stride, ps.d_off.data(), n_t, ps.raw.data(), ps.d_words.data());
        HIP_TRY(c, hipMemcpyAsync(words.data(), ps.d_words.data(), sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    }
    for (int t = 0; t < n_t; ++t) {
        if (count[(size_t)t] <= 0) continue;
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(ord2f(words[(size_t)3 * t + a])) || !std::isfinite(ord2f(words[(size_t)3 * n_t + 3 * t + a]))) { c->fail("pair target %d has non-finite coordinates", t); return DCREG_E_INVALID; }
    }
    // ---- every target's index, its cell edge chosen as build_index chooses it
    std::vector<int64_t> first(off, off + n_t);
    std::vector<GridDev> gs;
    int rc = clouds_index_build(c, ps, ps.raw.data(), n_t, count, first, words, search_radius * (1.0 + c->opt_cert_margin),
                                (double)c->opt_pair_max_table_entries, gs, ps.built);
    if (rc) return rc;
    const float bound = search_bound_sq(c, search_radius);
    for (int t = 0; t < n_t; ++t) {
        if (!ps.built[(size_t)t]) continue;
        grids[(size_t)t].g = gs[(size_t)t];
        grids[(size_t)t].max_ring = rings_for(gs[(size_t)t].h, bound);
        grids[(size_t)t].infl_max_d2 = (float)(4.0 * gs[(size_t)t].h * gs[(size_t)t].h);
    }
    if (n_t > 0) {
        HIP_TRY(c, hipMemcpyAsync(ps.d_grids.data(), grids.data(), sizeof(PairGrid) * (size_t)n_t, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    }
    ps.n = n_t;
    ps.radius_sq_f = bound;
    ps.grids = std::move(gs);
    ps.off.assign(off, off + n_t + 1);
    ps.search_radius = search_radius;
    return DCREG_OK;
}

// ------------------------------------------------------------------------------------------ linearise
// settled rules, once options (dcreg_debug.h "Settled and no longer options")
constexpr uint32_t kXcdChunk = 16;    // query-block -> XCD mapping (kernels.hpp xcd_remap): runs of 16 blocks round-robin (measured: C4 -13 %)
constexpr double kFarLoose = 1.5;     // search.hpp lin_search6: when a start bound is loose enough to be worth a probe (cells)

// the kernel arguments of checked parameters (lin_check) for a source of n points per pose (the Euler coefficients: stage_euler);
// own_grid = false: the launch searches grids of its own (dcreg_register_pairs: LinArgs::max_ring and infl_max_d2 come with every pose's grid)
static LinArgs make_lin_args(dcreg_ctx *c, const dcreg_lin_params *p, bool own_grid, int64_t n) {
    LinArgs a{};
    a.radius_sq = p->search_radius * p->search_radius;
    a.radius_sq_f = search_bound_sq(c, p->search_radius);
    float ro = (float)(p->search_radius * (1.0 + 1e-5));
    if ((double)ro < p->search_radius * (1.0 + 1e-5)) ro = std::nextafterf(ro, INFINITY);
    a.cert_r_out = ro;
    float ri = (float)(p->search_radius * (1.0 - 1e-5));
    if ((double)ri > p->search_radius * (1.0 - 1e-5)) ri = std::nextafterf(ri, 0.0f);
    a.cert_r_in = ri;
    a.max_thick_sq = p->max_plane_thickness_sq; a.min_norm = p->min_normal_norm;
    a.w_slope = p->weight_slope; a.w_min = p->weight_min; a.use_wd = p->use_weight_derivative;
    a.warm = c->opt_warm ? 1 : 0;
    a.team_max = std::min(std::max(c->opt_team_max, 0), kTeamMax);
    a.far_loose = (float)kFarLoose; a.xcd_chunk = kXcdChunk;
    a.prune_infl = (float)((1.0 + c->opt_cert_inflate) * (1.0 + c->opt_cert_inflate));
    a.infl_max_d2 = own_grid ? (float)(4.0 * c->map.grid.h * c->map.grid.h) : 0.f;
    a.max_ring = own_grid ? rings_for(c->map.grid.h, a.radius_sq_f) : 0;
    if (own_grid) c->last_max_ring = a.max_ring;
    a.count_scale = n < ((int64_t)1 << 26) ? kCountScale : 0.0;      // (strictly below: a count of 2^26 would read as one more of the number riding above it)
    a.euler = p->parameterization != DCREG_PARAM_SO3 ? 1 : 0;      // (dR, state, adv_counts: null until lin_reserve and the state selection)
    return a;
}

static int stage_euler(dcreg_ctx *c, const dcreg_lin_params *p, LinArgs &a) {
    if (!a.euler) return DCREG_OK;
    // The kernel's Euler branch (search.hpp row_of_plane) evaluates, for k = 0 (roll column) / 1 (pitch) / 2 (yaw),
    //     A[k] = c.x (D[9k+0] p.y + D[9k+1] p.z + D[9k+2] p.x) + c.y (D[9k+3] p.y + ...) + c.z (D[9k+6] p.y + ...)
    // - the shape of icp_test_runner.cpp:2323-2335 with its axis relabelling (pointOri = (p.y, p.z, p.x), coeff = (c.y, c.z, c.x)) undone for c
    // and kept for p, so that every product and every sum is taken in the order of the source text.  The 27 coefficients come from here.
    if (!c->h_euler) {
        HIP_TRY(c, c->h_euler.alloc(27, hipHostMallocDefault));
        HIP_TRY(c, c->d_euler.alloc(27));
    }
    // (the staging block is reused: the launches of the Euler engine are blocking calls, one at a time)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double *D = c->h_euler.data();
    if (p->parameterization == DCREG_PARAM_EULER) {
        // the reference's row, literally (:2299-2346): srx / crx of PITCH, sry / cry of YAW, srz / crz of ROLL; the brackets of arx times coeff.z,
        // coeff.x, coeff.y (LOAM: x, y, z), of ary times coeff.z, coeff.y, of arz times coeff.z, coeff.x, coeff.y; matA row = [arz, arx, ary, ...]
        const double srx = std::sin(p->euler_rpy[1]), crx = std::cos(p->euler_rpy[1]);
        const double sry = std::sin(p->euler_rpy[2]), cry = std::cos(p->euler_rpy[2]);
        const double srz = std::sin(p->euler_rpy[0]), crz = std::cos(p->euler_rpy[0]);
        const double crx_sry = crx * sry, crz_sry = crz * sry, srx_sry = srx * sry, srx_srz = srx * srz;   // :2319-2322
        // arz (:2331-2335) -> column 0
        D[0] = crz * srx_sry - cry * srz;   D[1] = -cry * crz - srx_sry * srz;   D[2] = 0.0;      // x coeff.z (= c.x)
        D[3] = crx * crz;                   D[4] = -(crx * srz);                 D[5] = 0.0;      // x coeff.x (= c.y)
        D[6] = sry * srz + cry * crz * srx; D[7] = crz_sry - cry * srx_srz;      D[8] = 0.0;      // x coeff.y (= c.z)
        // arx (:2323-2326) -> column 1
        D[9] = crx_sry * srz;               D[10] = crx * crz_sry;               D[11] = -srx_sry;        // x coeff.z
        D[12] = -srx_srz;                   D[13] = -(crz * srx);                D[14] = -crx;            // x coeff.x
        D[15] = crx * cry * srz;            D[16] = crx * cry * crz;             D[17] = -(cry * srx);    // x coeff.y
        // ary (:2327-2330) -> column 2 (no coeff.x bracket)
        D[18] = cry * srx_srz - crz_sry;    D[19] = sry * srz + cry * crz * srx; D[20] = crx * cry;       // x coeff.z
        D[21] = 0.0;                        D[22] = 0.0;                         D[23] = 0.0;
        D[24] = -cry * crz - srx_sry * srz; D[25] = cry * srz - crz * srx_sry;   D[26] = -crx_sry;        // x coeff.y
    } else {
        // exact derivatives of R = Rz(yaw) Ry(pitch) Rx(roll) (Pose6D2Matrix, utils.hpp:452-460), columns in the kernel's (p.y, p.z, p.x) order
        const double cr = std::cos(p->euler_rpy[0]), sr = std::sin(p->euler_rpy[0]);
        const double cp = std::cos(p->euler_rpy[1]), sp = std::sin(p->euler_rpy[1]);
        const double cy = std::cos(p->euler_rpy[2]), sy = std::sin(p->euler_rpy[2]);
        const double Rx[9] = {1, 0, 0, 0, cr, -sr, 0, sr, cr}, dRx[9] = {0, 0, 0, 0, -sr, -cr, 0, cr, -sr};
        const double Ry[9] = {cp, 0, sp, 0, 1, 0, -sp, 0, cp}, dRy[9] = {-sp, 0, cp, 0, 0, 0, -cp, 0, -sp};
        const double Rz[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1}, dRz[9] = {-sy, -cy, 0, cy, -sy, 0, 0, 0, 0};
        auto mul3 = [](const double *A, const double *B, const double *C3, double *out) {
            double T[9], O[9];
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += A[i * 3 + k] * B[k * 3 + j]; T[i * 3 + j] = s; }
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { double s = 0; for (int k = 0; k < 3; ++k) s += T[i * 3 + k] * C3[k * 3 + j]; O[i * 3 + j] = s; }
            for (int i = 0; i < 3; ++i) { out[i * 3 + 0] = O[i * 3 + 1]; out[i * 3 + 1] = O[i * 3 + 2]; out[i * 3 + 2] = O[i * 3 + 0]; }
        };
        mul3(Rz, Ry, dRx, D); mul3(Rz, dRy, Rx, D + 9); mul3(dRz, Ry, Rx, D + 18);
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_euler.data(), c->h_euler.data(), 27 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    a.dR = c->d_euler.data();
    return DCREG_OK;
}

// One linearisation = begin (argument checks, buffers, launches: returns as soon as the work is queued) + end (wait for
// the pinned result rows, unpack).  Two slots with their own pose / partial / result buffers let a caller keep one batch
// on the device while the host works on the other (dcreg_linearize_batch_begin / _end); the blocking entry points use
// slot 0.  Debug dumps are synchronous and only exist on slot 0.
static void free_tmp(LinSlot &S) { S.tmp_dev.clear(); }

// after a launch that may not have run: what the states hold is unknown
static void drop_warm(dcreg_ctx *c) {
    c->state_valid = false;
    c->nicp.warm_valid = false;        // (normal_icp.hip: its positions are the active index's too)
    c->nicp.drop_slots();              // (... and the warm slots of its batched launches go with them)
    c->adv_counts_dirty = true;        // (a pass may have run without the k_lin that takes its counts)
    std::fill(c->batch_state_valid.begin(), c->batch_state_valid.end(), (uint8_t)0);
}
// publish a gate record (kernels.hpp GateHost): pose words and checksum first, the number last.  R == null: an abort, the pose words
// stay whatever they were.
static void gate_publish(dcreg_ctx *c, unsigned long long seq_word, const double *R, const double *t) {
    unsigned long long w[kGateWords];
    w[0] = seq_word;
    for (int k = 1; k < kGateWords - 1; ++k) w[k] = c->h_gate.data()->w[k];
    if (R) {
        std::memcpy(&w[1], R, 9 * sizeof(double));
        std::memcpy(&w[10], t, 3 * sizeof(double));
    }
    unsigned long long x = kGateSalt;
    for (int k = 0; k < kGateWords - 1; ++k) x ^= w[k];
    w[kGateWords - 1] = x;
    volatile unsigned long long *dst = c->h_gate.data()->w;
    for (int k = 1; k < kGateWords; ++k) dst[k] = w[k];
    __atomic_store_n(&c->h_gate.data()->w[0], w[0], __ATOMIC_RELEASE);
}
static void gate_call_off(dcreg_ctx *c) { gate_publish(c, (c->gate_seq << 1) | 1ull, nullptr, nullptr); }

// how far a pose (R9, t3) may carry a point of the source from where the pose (R, t) had it
static double pose_jump(const dcreg_ctx *c, const double *R9, const double *t3, const double *R, const double *t) {
    double dr = 0.0, dt = 0.0;
    for (int k = 0; k < 9; ++k) dr += (R9[k] - R[k]) * (R9[k] - R[k]);
    for (int k = 0; k < 3; ++k) dt += (t3[k] - t[k]) * (t3[k] - t[k]);
    return std::sqrt(dr) * c->src_radius + std::sqrt(dt);
}

// dispatch order of the query-block groups (kernels.hpp k_group_cost): estimated cost of every group at this pose, heaviest first
static int estimate_dispatch_order(dcreg_ctx *c, const double *R9, const double *t3, int max_ring) {
    if (!c->d_group_est) HIP_TRY(c, c->d_group_est.alloc(kMaxGroups));
    PoseArg P{};
    for (int k = 0; k < 9; ++k) P.R[k] = R9[k];
    for (int k = 0; k < 3; ++k) P.t[k] = t3[k];
    const uint32_t ng = c->n_groups;
    const uint32_t lead = (blocks(c->n_src, kLinBlock) - ng * c->group_blocks) * (uint32_t)kLinBlock;      // points in front of the first group
    hipLaunchKernelGGL(k_group_cost, dim3(ng), dim3(256), 0, c->stream, c->d_src.data() + lead, (uint32_t)c->n_src - lead, c->map.grid, P, c->group_blocks * (uint32_t)kLinBlock,
                       max_ring, c->d_group_est.data());
    float est[kMaxGroups];
    HIP_TRY(c, hipMemcpyAsync(est, c->d_group_est.data(), sizeof(float) * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t order[kMaxGroups];
    for (uint32_t k = 0; k < (uint32_t)kMaxGroups; ++k) order[k] = k;
    std::stable_sort(order, order + ng, [&](uint32_t x, uint32_t y) { return est[x] > est[y]; });
    for (uint32_t k = 0; k < (uint32_t)kMaxGroups; ++k) c->group_order[k] = (uint8_t)order[k];
    double sum = 0.0, mx = 0.0;
    for (uint32_t k = 0; k < ng; ++k) { sum += est[k]; mx = std::max(mx, (double)est[k]); }
    c->order_uneven = mx * ng > 1.3 * sum;                       // some group costs well above the mean
    std::memcpy(c->est_R, R9, sizeof(c->est_R)); std::memcpy(c->est_t, t3, sizeof(c->est_t));
    c->order_valid = true; c->est_launch = (int64_t)c->seq;
    return DCREG_OK;
}

// A launch as it goes through linearize_begin: the call's arguments, what lin_check settles (kind, points per pose) and what the steps
// after it fill in (kernel arguments, the pose of a single-pose launch, debug buffers, the staged poses of a batch)
struct LinLaunch {
    int slot, n_poses; const double *R9, *t3; const int32_t *state_ids, *frame_ids, *grid_ids; const dcreg_lin_params *p; dcreg_lin_debug *dbg;
    LinKind kind; int64_t n;            // points per pose: the ctx's source, or the largest frame of the launch
    dcreg_ctx::FrameSet *fs;            // frames / pairs: the sources of the poses
    dcreg_ctx::StateKey key; LinArgs a; DebugDev dd;
    PoseArg one;                        // the pose of a single-pose launch (k_lin pose1)
    const PoseArg *d_poses;             // batches: the staged poses (gated launches: the device pose the gate fills)
    const uint2 *d_slices;              // frames: {first point, points} of every pose's frame (kernels.hpp k_lin SLICE)
    const uint32_t *d_grid_ids;         // pairs: every pose's target grid (kernels.hpp k_lin GRIDS)
    bool state_was_valid;               // the ctx's own state held a search before this launch (restored if a gated launch is called off)
    bool state_was_five;                // ... left by a five-neighbour launch (dcreg_ctx::state_five)
    bool own() const { return kind >= LinKind::single; }
    bool uses_state(const dcreg_ctx *c) const { return own() && c->opt_warm; }
};

// Check: every refusal of a launch, before anything is changed (no HIP call; nothing of the ctx but its error text is written)
static int lin_check(dcreg_ctx *c, LinLaunch &L) {
    const bool gated = L.kind == LinKind::gated;
    // a timing probe, not a dump (dcreg_debug.h dcreg_lin_debug::stamps): certificates in use, only the stamps come back
    const dcreg_lin_debug *d = L.dbg;
    const bool stamps_only = d && d->stamps && !d->nn_idx && !d->nn_d2 && !d->flag && !d->normal && !d->r && !d->s && !d->stats;
    // nothing may be queued behind a gate that still waits: it would wait with it
    if (c->gate_slot >= 0) { c->fail("a gated linearisation still waits for its pose (dcreg_linearize_gate_open / _gate_abort first)"); return DCREG_E_STATE; }
    if (gated) {
        static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
        L.R9 = eye; L.t3 = zero; L.n_poses = 1; L.state_ids = nullptr; L.dbg = nullptr;
        // results must arrive through the pinned flags: a stream synchronise would wait for the gate, i.e. for its own caller
        if (!c->opt_spin) { c->fail("gated launches need the \"spin\" option (results through pinned flags)"); return DCREG_E_STATE; }
        // A launch that is to be TIMED (option "time_kernels": HIP events around it) is not gated - the caller starts it the plain way
        // once its pose exists.  Measured (profiles/r04_events_vs_trace.md): the event in front of a gated linearisation is stamped when
        // the gate kernel STARTS, and that can be long before the previous linearisation ends (its last blocks leave most of the device
        // idle): events reported 324 us for a launch the kernel trace gives 228 us.
        if (c->opt_time_kernels > 0 && (c->launch_counter % (uint64_t)c->opt_time_kernels) == 0) {
            c->fail("the next launch is a timed one: not gated"); return DCREG_E_STATE;
        }
    }
    if (L.slot < 0 || L.slot >= dcreg_ctx::kLinSlots) { c->fail("invalid slot"); return DCREG_E_INVALID; }
    if (c->slots[L.slot].pending) { c->fail("slot %d still has a linearisation in flight", L.slot); return DCREG_E_STATE; }
    if (c->nicp.batch_pending()) { c->fail("a batched normal linearisation is still in flight (dcreg_normals_batch_end first)"); return DCREG_E_STATE; }
    if (!L.R9 || !L.t3 || L.n_poses < 1) { c->fail("null argument"); return DCREG_E_INVALID; }
    if (L.n_poses > 65535) { c->fail("at most 65535 poses per batched launch (grid.y limit), got %d", L.n_poses); return DCREG_E_INVALID; }
    // a pose with a NaN or an infinity is refused before anything is queued or changed (the search's cell keys of such a point are undefined)
    if (!poses_finite(L.n_poses, L.R9, L.t3)) { c->fail("a pose with non-finite entries"); return DCREG_E_INVALID; }
    if (!L.grid_ids && c->map.n <= 0) { c->fail("KdTree/target index is not set up in context"); return DCREG_E_STATE; }   // :1639
    L.fs = L.grid_ids ? &c->pair_src : &c->frames;
    if (L.grid_ids) {
        if (!L.frame_ids) { c->fail("pair launches name a source for every pose"); return DCREG_E_INVALID; }
        const dcreg_ctx::PairSet &ps = c->pairs;
        for (int i = 0; i < L.n_poses; ++i) {
            const int32_t t = L.grid_ids[i];
            if (t < 0 || t >= ps.n || !ps.built[(size_t)t]) { c->fail("pair target %d is not built", t); return DCREG_E_INVALID; }
        }
        if (!L.p || search_bound_sq(c, L.p->search_radius) != ps.radius_sq_f) { c->fail("the pair targets were built for another search radius"); return DCREG_E_INVALID; }
    }
    L.n = c->n_src;
    if (L.frame_ids) {
        if (!L.state_ids || L.dbg || gated) { c->fail("frame launches are batched product launches"); return DCREG_E_INVALID; }
        L.n = 0;
        for (int i = 0; i < L.n_poses; ++i) {
            const int32_t f = L.frame_ids[i];
            if (f < 0 || (size_t)f >= L.fs->slice.size() || L.fs->slice[(size_t)f].y == 0u) { c->fail("frame %d is not loaded or empty", f); return DCREG_E_INVALID; }
            L.n = std::max<int64_t>(L.n, L.fs->slice[(size_t)f].y);
        }
    } else
    if (c->n_src <= 0) { c->fail("measure cloud is not set"); return DCREG_E_STATE; }
    L.kind = L.grid_ids ? LinKind::pairs : L.frame_ids ? LinKind::frames : gated ? LinKind::gated : (L.n_poses > 1 || L.state_ids) ? LinKind::batch :
             !L.dbg ? LinKind::single : stamps_only ? LinKind::stamps : LinKind::dump;
    // (the launches that choose their index, the window of a large map or the whole map, need their parameters for that)
    if (!L.p && !gated && (c->roi_active || roi_wanted(c))) { c->fail("null argument"); return DCREG_E_INVALID; }
    const dcreg_lin_params *p = L.p;
    if (!p || !(p->search_radius > 0.0)) { c->fail("invalid linearisation parameters"); return DCREG_E_INVALID; }
    if (p->k != 5 && p->k != 0) { c->fail("only k = 5 is supported (icp_test_runner.cpp:1722)"); return DCREG_E_INVALID; }
    if (p->parameterization != DCREG_PARAM_SO3 && p->parameterization != DCREG_PARAM_EULER && p->parameterization != DCREG_PARAM_EULER_EXACT) { c->fail("unknown parameterization"); return DCREG_E_INVALID; }
    if (L.state_ids && c->opt_warm) {   // batched poses: each may own one of the reserved states, -1 = search cold, keep nothing
        const int64_t n_states = L.frame_ids ? L.fs->n_states : c->n_batch_states;
        std::vector<uint8_t> seen((size_t)std::max<int64_t>(n_states, 1), 0);
        for (int i = 0; i < L.n_poses; ++i) {
            const int32_t sid = L.state_ids[i];
            if (sid < 0) continue;
            if ((int64_t)sid >= n_states) { c->fail("warm state %d was not reserved (dcreg_reserve_warm_states: %lld)", sid, (long long)n_states); return DCREG_E_INVALID; }
            if (seen[(size_t)sid]) { c->fail("warm state %d is used by two poses of one launch", sid); return DCREG_E_INVALID; }
            seen[(size_t)sid] = 1;
        }
    }
    return DCREG_OK;
}

// heavy groups first: single-pose launches of at least two groups, once the order has been estimated (a gated launch does not know its
// pose yet: it uses the order there is).  (A launch whose blocks are all resident at once - 4 per CU - has no order to speak of.)
static bool order_wanted(const dcreg_ctx *c, const LinLaunch &L) {
    return c->opt_dispatch_order && L.own() && c->n_groups >= 2 && blocks(L.n, kLinBlock) > 4u * (uint32_t)c->n_cus &&
           c->hint_misalign > 0.5 * c->map.grid.h;
}

// Plan: how a checked launch is carried out.  fresh: the ctx's own state holds nothing yet (single-pose kinds)
static LinPlan lin_plan(const dcreg_ctx *c, const LinLaunch &L, bool fresh) {
    LinPlan P;
    P.kind = L.kind; P.n_poses = L.n_poses; P.nbx = blocks(L.n, kLinBlock);
    // one pose: the kernels finish the reduction themselves (chunk rows -> pinned memory); many poses: k_finalize
    P.n_chunks = (P.nbx + kChunk - 1) / kChunk;
    // ... and so do batches whose poses are one chunk each (the Monte-Carlo batches: 30 blocks per pose): the last block of a pose sums
    // the pose's rows - block_sum_rows, as k_finalize would - and publishes the pose's result row
    const bool fused = L.n_poses == 1 || P.n_chunks == 1;
    // a launch of one chunk's worth of blocks: the blocks publish their rows themselves and the host adds them (kernels.hpp FinArgs)
    P.direct = fused && L.n_poses == 1 && P.nbx <= (uint32_t)kChunk && c->opt_one_wave < 2;     // (one_wave = 2: tile rows even there - tests)
    P.n_rows = P.direct ? (size_t)P.nbx : (fused ? (size_t)P.n_chunks * (size_t)P.n_poses : (size_t)P.n_poses);
    const bool dbg = L.kind == LinKind::dump || L.kind == LinKind::stamps;
    P.use_cert = L.kind != LinKind::dump && c->opt_use_cert;     // a debug dump searches every point (its statistics are those of the searches)
    P.ordered = order_wanted(c, L) && c->order_valid && c->order_uneven;
    // what the launch is expected to search: what the last completed launch reported (with the engines' pipeline: the launch two back)
    const bool known = c->last_searched >= 0 && c->last_points == L.n;
    const double f = known ? (double)c->last_searched / (double)L.n : -1.0;
    // The advance pass (kernels.hpp k_advance) in front of this launch?  Only where it can pay: a single pose on the ctx's own state,
    // certificates in use, the state filled by an earlier launch; by default ("advance" = 1) a cloud whose query blocks exceed what the
    // device holds at once (below that a launch lasts as long as one search whether its searches are dense or not) in a launch expected
    // to search between 0.5 % and 70 % of its points (profiles/fused_pass_ablation.md section 3: the window in which the pass that builds
    // the rows itself beats k_lin alone by 6 us and more).  Scheduling only: the sums are the same with and without the pass.
    if ((L.kind == LinKind::single || L.kind == LinKind::gated) && c->opt_warm && !fresh && P.use_cert && L.a.count_scale != 0.0) {
        constexpr double kAdvanceLo = 0.005, kAdvanceHi = 0.70;
        // (the two launches behind the end of a series of five-neighbour launches: what the last completed launch searched - everything,
        //  by construction - says nothing about them; the series ended because the pose has nearly settled, the first six-neighbour
        //  launch has left fresh certificates, and a fifth to a half of the points is what such a launch searches: inside the window)
        const bool in_window = (known && f >= kAdvanceLo && f <= kAdvanceHi) || c->five_tail > 0;
        const bool adv = c->opt_advance >= 2 || (c->opt_advance == 1 && P.nbx >= (uint32_t)c->opt_advance_min_blocks && in_window);
        // ... its small-frame form (k_advance_team: sixteen lanes per query, one wave per kTeamTile points): a frame of a few thousand
        // points, whose query blocks leave most of the device idle, in a launch expected to search most of its points (the pass costs
        // ~12 us whatever it finds to do; k_lin alone gets cheaper as its searching waves thin out, so below half it wins again)
        // ... and only against a map whose occupied cells hold several points each: there a query with a loose bound (an OUT point, a
        // jump) has a hundred and more candidates in its 27-cell block and the lock-step search, two trips in flight, is at its slowest;
        // against a sparse map (the 7.5 k-point fixture: 1.6 points per occupied cell) it is as fast as the teams
        constexpr double kTeamPassMaxPoints = 16384.0, kTeamPassMinFrac = 0.5, kTeamPassMinCellPts = 3.0;
        const double per_cell = (double)c->map.n / (double)std::max<uint32_t>(c->map.occupied, 1u);
        const bool team = c->opt_team_pass >= 2 || (c->opt_team_pass == 1 && L.n <= (int64_t)kTeamPassMaxPoints && known && f >= kTeamPassMinFrac &&
                                                    per_cell >= kTeamPassMinCellPts);
        P.pass = team ? LinPass::team : adv ? LinPass::advance : LinPass::none;
        if (c->opt_search_five >= 2 && c->opt_advance < 2 && c->opt_team_pass < 2) P.pass = LinPass::none;    // (tests: five-neighbour launches wherever possible)
    }
    // the one-wave instantiation of k_lin (kernels.hpp): fused single-pose launches of many blocks in which most waves search
    bool one_wave = false;
    if (L.n_poses > 1)      // batched launches of one-chunk poses (the Monte-Carlo batches): trials at every stage of their runs side by side
        one_wave = fused && !dbg && (c->opt_one_wave >= 2 || (c->opt_one_wave_batches && (uint64_t)L.n_poses * P.nbx >= (uint64_t)c->opt_one_wave_min_blocks));
    else if (!P.direct && !dbg && P.pass != LinPass::team) {
        // by the rule: a launch of many blocks whose searches are long - the queries more than a cell and a half from the surface (the
        // engines' hint, as for the dispatch order; unknown at the start of a run = far) - and most of whose points search
        const bool most = !L.uses_state(c) || fresh || !P.use_cert || (known && (double)c->last_searched >= c->opt_one_wave_min_frac * (double)L.n);
        one_wave = c->opt_one_wave >= 2 || (c->opt_one_wave == 1 && P.nbx >= (uint32_t)c->opt_one_wave_min_blocks && P.pass != LinPass::advance && most &&
                                            c->hint_misalign > c->opt_one_wave_min_cells * c->map.grid.h);
    }
    // A gated launch the device holds at once (at most kChunk query blocks) waits for its pose in its FIRST kernel instead of behind a
    // gate kernel (kernels.hpp gate_wait: one kernel boundary less on a launch that lasts a few microseconds); larger launches keep
    // k_gate (every wave would pay for the wait: profiles/r04_gate_in_kernel.txt).  What this relies on and costs: every
    // wave of the gated kernel - at most 64 x 4 of k_lin, at most 4096 one-wave blocks of the teams - is resident and polls the DEVICE copy
    // of the record while the host takes its step; only the first wave of block 0 polls the host record and fills the copy, so progress
    // rests on block 0 being dispatched before the device is full, which holds while blocks are dispatched in index order and the launch
    // fits the device (nbx <= kChunk: it does).  A context that shares its device with other busy contexts holds wave slots idle that way;
    // option "gate_in_kernel" = 0 puts the one-wave k_gate back in front.
    P.gate_inside = L.kind == LinKind::gated && c->opt_gate_in_kernel && P.nbx <= (uint32_t)kChunk && P.pass != LinPass::advance;
    // the k_lin instantiation: a gated k_lin runs in four-wave blocks whatever the one-wave rule says
    P.body = (P.gate_inside && P.pass != LinPass::team) ? LinBody::gated : L.kind == LinKind::stamps ? LinBody::stamps : L.kind == LinKind::dump ? LinBody::dump :
             one_wave ? LinBody::one_wave : fused ? LinBody::fused : LinBody::chunked;
    // the pass carries the launch out alone (kernels.hpp k_advance ROWS: the rows of a tile by the block that worked its list off, no k_lin
    // behind it) wherever k_lin would run as the plain fused kernel behind it; direct launches keep the two kernels (option "advance_fused")
    P.pass_rows = P.pass == LinPass::advance && c->opt_advance_fused != 0 && !P.direct && P.body == LinBody::fused;
    // A five-neighbour launch (kernels.hpp k_lin FIVE)?  What a six-neighbour search leaves for the NEXT launch - the sixth neighbour, the
    // bound of the seventh, the certificate, the plane - is used only if the pose then moves by less than a certificate's radius: a few
    // per cent of the point spacing.  While a trajectory still moves by more than that per launch, every launch searches every point and
    // that part of its work is wasted.  Where it can run: a single pose on the ctx's own state, carried out by the fused or the one-wave
    // k_lin alone (no pass in front, not gated in the kernel, no dump).  By the rule (option "search_five" = 1) on an engine's trajectory
    // only - the first launch of a run the engine announced (dcreg_hint_misalignment(-1)) and the launches queued behind a gate -, when
    // the last completed launch searched at least 95 % of its points (in the engines' pipeline: the launch two back) and the last step
    // known exceeds "search_five_step" cell edges (profiles/five_mode_ab.md has the table both numbers come from).  A five-neighbour launch
    // reports every point as searched, so it is the step that ends the series.  Scheduling only: the sums are bitwise the same.
    const bool can_five = (L.kind == LinKind::single || L.kind == LinKind::gated) && L.uses_state(c) && !dbg && P.pass == LinPass::none &&
                          (P.body == LinBody::fused || P.body == LinBody::one_wave);
    P.five = can_five && (c->opt_search_five >= 2 ||
                          (c->opt_search_five == 1 && P.use_cert && (fresh || (known && f >= c->opt_search_five_frac)) &&
                           c->last_step > c->opt_search_five_step * c->map.grid.h));
    return P;
}

// the poses of a batched launch, their states and (frames, pairs) slices and target ids in one pinned block, and its upload
static int stage_poses(dcreg_ctx *c, LinSlot &S, LinLaunch &L) {
    const int64_t n_states = L.frame_ids ? L.fs->n_states : c->n_batch_states;
    std::vector<uint8_t> &state_valid = L.frame_ids ? L.fs->state_valid : c->batch_state_valid;
    dcreg_ctx::StateKey &states_key = L.frame_ids ? L.fs->key : c->batch_state_key;
    const bool use_states = L.state_ids && c->opt_warm && n_states > 0;
    if (use_states && !(L.key == states_key)) {
        std::fill(state_valid.begin(), state_valid.end(), (uint8_t)0);
        states_key = L.key;
    }
    const int n_poses = L.n_poses;
    // (frames: the poses' slices ride behind the poses in the same block - one copy; pairs: and their target ids behind those)
    const size_t bytes = (size_t)n_poses * sizeof(PoseArg) + (L.frame_ids ? (size_t)n_poses * sizeof(uint2) : 0) +
                         (L.grid_ids ? (size_t)n_poses * sizeof(uint32_t) : 0);
    if (bytes > S.d_poses.cap()) {      // the pinned block stays alive until end(): source of the asynchronous copy
        S.h_poses.reset(); S.d_poses.reset();
        const size_t cap = std::max<size_t>(bytes, 256 * (sizeof(PoseArg) + sizeof(uint2) + sizeof(uint32_t)));
        HIP_TRY(c, S.h_poses.alloc(cap, hipHostMallocDefault));
        if (S.d_poses.alloc(cap) != hipSuccess) { c->fail("hipMalloc(%zu B) failed", cap); return DCREG_E_NOMEM; }
    }
    PoseArg *hp = (PoseArg *)S.h_poses.data();
    for (int i = 0; i < n_poses; ++i) {
        std::memcpy(hp[i].R, L.R9 + 9 * i, sizeof(hp[i].R)); std::memcpy(hp[i].t, L.t3 + 3 * i, sizeof(hp[i].t));
        const bool has = use_states && L.state_ids[i] >= 0;
        hp[i].state = has ? (uint32_t)L.state_ids[i] : kNoIdx;
        hp[i].fresh = (has && state_valid[(size_t)L.state_ids[i]] != 0) ? 0u : 1u;
        if (has) state_valid[(size_t)L.state_ids[i]] = 1;
    }
    if (L.frame_ids) {
        uint2 *hs = (uint2 *)(S.h_poses.data() + (size_t)n_poses * sizeof(PoseArg));
        for (int i = 0; i < n_poses; ++i) hs[i] = L.fs->slice[(size_t)L.frame_ids[i]];
        L.d_slices = (const uint2 *)(S.d_poses.data() + (size_t)n_poses * sizeof(PoseArg));
    }
    if (L.grid_ids) {
        const size_t at = (size_t)n_poses * (sizeof(PoseArg) + sizeof(uint2));
        std::memcpy(S.h_poses.data() + at, L.grid_ids, sizeof(uint32_t) * (size_t)n_poses);
        L.d_grid_ids = (const uint32_t *)(S.d_poses.data() + at);
    }
    // (measured and dropped, profiles/r05_ablation.md: the upload on a copy stream behind an event - the cross-stream dependency costs
    //  more than the 4.6 us copy it hides, C5 1.56 M against 1.64 M it/s - and no upload at all, the kernel reading the pinned block:
    //  +2.7 us per kernel, nothing gained - the experiment is bound by its kernels, two groups of trials alternating on the device)
    HIP_TRY(c, hipMemcpyAsync(S.d_poses.data(), S.h_poses.data(), bytes, hipMemcpyHostToDevice, c->stream));
    L.d_poses = (const PoseArg *)S.d_poses.data();
    if (use_states && L.frame_ids) { L.a.state = L.fs->state.data(); L.a.state_stride = (uint32_t)L.fs->state_stride; }
    else if (use_states) { L.a.state = c->d_state_batch.data(); L.a.state_stride = (uint32_t)c->state_batch_stride; }
    return DCREG_OK;
}

// Reserve: every buffer the plan needs is grown and cleared here, before the first kernel of the launch is queued - a hipFree queued
// behind a gate kernel that waits for the host would wait for it
static int lin_reserve(dcreg_ctx *c, LinSlot &S, LinLaunch &L, const LinPlan &P) {
    if (int rc = stage_euler(c, L.p, L.a)) return rc;
    // (one-wave blocks: a row per TILE)
    if (S.d_partials.ensure(c, (size_t)P.n_poses * P.nbx * kSlots * (P.one_wave() ? kLinBlock / kWave : 1))) return DCREG_E_NOMEM;
    if (P.fused()) {   // tickets: zero when (re)allocated, afterwards every completed launch leaves them zero
        const size_t had = S.d_tickets.cap();
        if (S.d_tickets.ensure(c, (size_t)P.n_chunks * (size_t)P.n_poses * kCounterStride)) return DCREG_E_NOMEM;
        if (S.d_tickets.cap() != had || S.tickets_dirty) {
            HIP_TRY(c, hipMemsetAsync(S.d_tickets.data(), 0, sizeof(unsigned int) * S.d_tickets.cap(), c->stream));
            S.tickets_dirty = false;
        }
    }
    if (P.n_rows * kSlots > S.h_out.cap()) {
        const size_t cap = std::max<size_t>(P.n_rows, 64) * kSlots;
        HIP_TRY(c, S.h_out.alloc(cap, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(S.h_out.data(), 0, cap * sizeof(double));
        std::fill(S.row_chk.begin(), S.row_chk.end(), 0ull);
    }
    if (L.kind == LinKind::gated) {
        if (!c->h_gate) {     // all or nothing: a half-built gate would be taken for a whole one by the next call
            PinnedBuf<GateHost> hg; DevBuf<PoseArg> dp; DevBuf<uint32_t> da; DevBuf<GateDev> gd;
            bool ok = hg.alloc(1, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
            ok = ok && dp.alloc(1) == hipSuccess && da.alloc(1) == hipSuccess;
            // (the device copy of the record, for launches gated in their first kernel: cleared IN THE STREAM - the ctx stream does not
            //  synchronise with the null stream)
            ok = ok && gd.alloc(1) == hipSuccess && hipMemsetAsync(gd.data(), 0, sizeof(GateDev), c->stream) == hipSuccess;
            if (!ok) {
                c->state_valid = L.state_was_valid;
                c->fail("allocating the launch gate failed");
                return DCREG_E_NOMEM;
            }
            std::memset(hg.data(), 0, sizeof(GateHost));
            c->h_gate = std::move(hg); c->d_gate_pose = std::move(dp); c->d_gate_abort = std::move(da); c->d_gate_dev = std::move(gd);
        }
        L.d_poses = c->d_gate_pose.data();
    }
    if (int rc = L.own() ? DCREG_OK : stage_poses(c, S, L)) return rc;
    if (P.pass != LinPass::none && !P.pass_rows) {      // the passes' counts, per query block of k_lin: zero between launches (k_lin takes them and zeroes them again)
        const size_t had = c->d_adv_counts.cap();
        if (c->d_adv_counts.ensure(c, (size_t)kCounterStride * P.nbx)) return DCREG_E_NOMEM;      // (a 128-byte line per query block)
        if (c->d_adv_counts.cap() != had || c->adv_counts_dirty) {
            HIP_TRY(c, hipMemsetAsync(c->d_adv_counts.data(), 0, sizeof(uint32_t) * c->d_adv_counts.cap(), c->stream));
            c->adv_counts_dirty = false;
        }
        L.a.adv_counts = c->d_adv_counts.data();
    }
    if (P.pass == LinPass::team && c->opt_team_stamps) {   // timing probe (dcreg_debug.h dcreg_team_pass_stamps): eight clock words per block of the pass
        const uint32_t n_tiles = blocks(L.n, kTeamTile);
        if (c->d_team_stamps.ensure(c, (size_t)8 * (n_tiles + 1))) return DCREG_E_NOMEM;
        HIP_TRY(c, hipMemsetAsync(c->d_team_stamps.data(), 0, sizeof(unsigned long long) * 8 * (n_tiles + 1), c->stream));
        c->team_stamps_n = n_tiles;
    }
    free_tmp(S);
    if (L.dbg) {
        const dcreg_lin_debug *dbg = L.dbg; const size_t n = (size_t)L.n; DebugDev &dd = L.dd;
        bool oom = false;
        auto alloc = [&](size_t bytes, int fill) -> void * {
            DevBuf<unsigned char> b;
            if (b.alloc(bytes) != hipSuccess) { oom = true; return nullptr; }
            (void)hipMemsetAsync(b.data(), fill, bytes, c->stream);
            S.tmp_dev.push_back(std::move(b));
            return S.tmp_dev.back().data();
        };
        if (dbg->nn_idx) dd.nn_idx = (int32_t *)alloc(sizeof(int32_t) * 5 * n, 0xFF);
        if (dbg->nn_d2) dd.nn_d2 = (float *)alloc(sizeof(float) * 5 * n, 0);
        if (dbg->flag) dd.flag = (uint8_t *)alloc(n, 0);
        if (dbg->normal) dd.normal = (double *)alloc(sizeof(double) * 3 * n, 0);
        if (dbg->r) dd.r = (double *)alloc(sizeof(double) * n, 0);
        if (dbg->s) dd.s = (double *)alloc(sizeof(double) * n, 0);
        if (dbg->stats) dd.stats = (uint32_t *)alloc(sizeof(uint32_t) * n, 0);
        if (dbg->stamps) dd.stamps = (unsigned long long *)alloc(sizeof(unsigned long long) * 8 * (kLinBlock / 64) * (size_t)P.nbx, 0);
        if (oom) { free_tmp(S); drop_warm(c); c->fail("hipMalloc of the debug dump buffers failed"); return DCREG_E_NOMEM; }
    }
    // (a five-neighbour launch on a state whose last launch was one too: every certificate has radius zero - nothing to load or test)
    L.a.use_cert = (P.use_cert && !(P.five && c->state_five && L.state_was_valid)) ? 1 : 0;
    L.a.search_count = c->opt_count_searches ? c->d_search_count.data() : nullptr;
    L.a.group_blocks = std::max<uint32_t>(c->group_blocks, 1u); L.a.n_groups = P.ordered ? c->n_groups : 0u;
    std::memcpy(L.a.group_order, c->group_order, sizeof(L.a.group_order));
    return DCREG_OK;
}

// the k_lin instantiation of a plan (kernels.hpp k_lin<MODE, FUSED, FAST, GATE, ONE, SLICE, GRIDS>)
using LinKernel = decltype(&k_lin<0, true, true>);
template <bool FAST, bool SLICE = false, bool GRIDS = false>
static LinKernel lin_kernel(const LinPlan &P) {
    if constexpr (!SLICE) {
        if (P.kind == LinKind::pairs) return lin_kernel<FAST, true, true>(P);     // every pose reads its own slice and its own target grid
        if (P.kind == LinKind::frames) return lin_kernel<FAST, true>(P);         // every pose reads its own slice
        if (P.body == LinBody::gated) return k_lin<0, true, FAST, true>;         // (MODE 0: a gated launch is never a dump)
        if (P.body == LinBody::stamps) return k_lin<2, true, FAST>;      // (the probe writes the shared state: same fit as the plain launches)
        if (P.body == LinBody::dump) return k_lin<1, true, FAST>;
    }
    if constexpr (!SLICE) {
        if (P.five) return P.one_wave() ? k_lin<0, true, FAST, false, true, false, false, true> : k_lin<0, true, FAST, false, false, false, false, true>;
    }
    if (P.one_wave()) return k_lin<0, true, FAST, false, true, SLICE, GRIDS>;
    return P.fused() ? k_lin<0, true, FAST, false, false, SLICE, GRIDS> : k_lin<0, false, FAST, false, false, SLICE, GRIDS>;
}

// Queue: gate, start event, pass, k_lin (k_sum_tiles behind one-wave blocks; none behind a pass that builds the rows itself), k_finalize,
// end event, dump readback
template <bool FAST>
static int lin_queue(dcreg_ctx *c, LinSlot &S, LinLaunch &L, const LinPlan &P) {
    const bool gated = L.kind == LinKind::gated, team = P.pass == LinPass::team, slice = L.kind == LinKind::frames || L.kind == LinKind::pairs;
    const uint32_t n = (uint32_t)L.n;
    const unsigned long long seq = ++c->seq;
    FinArgs fin{S.d_tickets.data(), S.h_out.dev(), seq, P.direct ? 1u : 0u, P.n_chunks};
    if (P.fused()) S.tickets_dirty = true;    // cleared again once this launch is known to have completed
    // kernel timing: HIP events around every opt_time_kernels-th linearisation (each timed launch costs ~10 us of host time)
    bool timed = c->opt_time_kernels > 0 && (c->launch_counter++ % (uint64_t)c->opt_time_kernels) == 0;
    if (timed && !S.ev0) timed = false;               // (the slot's events are created with the context)
    const uint32_t *abort_flag = nullptr;
    // a launch that was queued and must not run after all (errors below): call the gate off, forget what the states were about to hold
    auto bail = [&](const char *what, hipError_t e) {
        if (e == hipSuccess) return DCREG_OK;
        free_tmp(S);
        if (gated) gate_call_off(c);
        drop_warm(c);
        c->fail("%s failed: %s", what, hipGetErrorString(e));
        return DCREG_E_DEVICE;
    };
    auto record = [&](hipEvent_t ev) { return bail("hipEventRecord", timed ? hipEventRecord(ev, c->stream) : hipSuccess); };
    GateArgs gt{nullptr, nullptr, 0ull, nullptr, nullptr, 0u};
    const PoseArg *lin_poses = L.d_poses;          // what k_lin reads its pose from (null: pose1)
    if (gated) {
        const unsigned long long want = ++c->gate_seq;
        if (P.gate_inside) {
            gt = GateArgs{c->h_gate.dev(), c->d_gate_dev.data(), want, team ? c->d_gate_pose.data() : nullptr, team ? c->d_gate_abort.data() : nullptr, L.one.fresh};
            if (team) abort_flag = c->d_gate_abort.data();        // (k_lin behind the teams reads what their polling wave left, as behind k_gate)
            else lin_poses = nullptr;                      // (k_lin itself is the gated kernel: pose1 carries state / fresh)
        } else {
            hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, c->stream, c->h_gate.dev(), want, c->d_gate_pose.data(), L.one.fresh, c->d_gate_abort.data());
            abort_flag = c->d_gate_abort.data();
        }
    }
    if (int rc = record(S.ev0)) return rc;         // after the gate: the events bracket the linearisation, not the wait for the pose
    if (P.pass == LinPass::advance) {          // (pass_rows: the launch's only linearisation kernel - rows, tickets and chunk rows are its own)
        const auto pass = P.pass_rows ? k_advance<FAST, true> : k_advance<FAST, false>;
        hipLaunchKernelGGL(pass, dim3(blocks(L.n, kAdvTile)), dim3(kLinBlock), 0, c->stream, c->d_src.data(), n, c->map.grid, L.one, L.d_poses, L.a,
                           P.pass_rows ? nullptr : c->d_adv_counts.data(), abort_flag, S.d_partials.data(), P.nbx, fin);
    }
    if (team) {      // with the gate inside, the teams are the gated kernel
        const auto pass = P.gate_inside ? k_advance_team<FAST, true> : k_advance_team<FAST>;
        hipLaunchKernelGGL(pass, dim3(blocks(L.n, kTeamTile)), dim3(kWave), 0, c->stream, c->d_src.data(), n, c->map.grid, L.one, P.gate_inside ? nullptr : L.d_poses,
                           L.a, c->d_adv_counts.data(), P.gate_inside ? nullptr : abort_flag, c->opt_team_stamps ? c->d_team_stamps.data() : nullptr, gt);
    }
    if (P.pass != LinPass::none) {
        if (int rc = bail(team ? "team advance pass launch" : "advance pass launch", hipGetLastError())) return rc;
        c->n_advance_launches += 1;
    }
    const bool one = P.one_wave(); const auto lin = lin_kernel<FAST>(P);      // (one-wave blocks: a grid of tiles)
    if (!P.pass_rows)
    hipLaunchKernelGGL(lin, dim3(one ? P.nbx * (kLinBlock / kWave) : P.nbx, (unsigned)P.n_poses), dim3(one ? kWave : kLinBlock), 0, c->stream,
                       slice ? L.fs->src.data() : c->d_src.data(), n, c->map.grid, L.one, lin_poses, L.a, S.d_partials.data(), P.nbx, fin, L.dd, abort_flag, gt,
                       L.d_slices, L.kind == LinKind::pairs ? c->pairs.d_grids.data() : nullptr, L.d_grid_ids);
    if (one)
        hipLaunchKernelGGL(slice ? k_sum_tiles<true> : k_sum_tiles<false>, dim3(P.n_chunks, (unsigned)P.n_poses), dim3(kLinBlock), 0, c->stream, S.d_partials.data(),
                           P.nbx, S.h_out.dev(), seq, abort_flag, L.d_slices);
    // an invalid launch (bad grid, too many resources) must surface here, not as a spin timeout in end()
    if (int rc = bail("linearisation kernel launch", hipGetLastError())) return rc;
    if (!P.fused()) {
        hipLaunchKernelGGL(slice ? k_finalize<true> : k_finalize<false>, dim3((unsigned)P.n_poses), dim3(kLinBlock), 0, c->stream, S.d_partials.data(), P.nbx,
                           S.h_out.dev(), seq, L.d_slices);
        if (int rc = bail("k_finalize launch", hipGetLastError())) return rc;
    }
    if (int rc = record(S.ev1)) return rc;         // brackets the linearisation's kernels
    if (const dcreg_lin_debug *dbg = L.dbg) {
        const DebugDev &dd = L.dd;
        hipError_t ce = hipSuccess;
        auto back = [&](void *dst, const void *srcp, size_t bytes) { if (ce == hipSuccess && srcp) ce = hipMemcpyAsync(dst, srcp, bytes, hipMemcpyDeviceToHost, c->stream); };
        back(dbg->nn_idx, dd.nn_idx, sizeof(int32_t) * 5 * n);
        back(dbg->nn_d2, dd.nn_d2, sizeof(float) * 5 * n);
        back(dbg->flag, dd.flag, (size_t)n);
        back(dbg->normal, dd.normal, sizeof(double) * 3 * n);
        back(dbg->r, dd.r, sizeof(double) * n);
        back(dbg->s, dd.s, sizeof(double) * n);
        back(dbg->stats, dd.stats, sizeof(uint32_t) * n);
        back(dbg->stamps, dd.stamps, sizeof(unsigned long long) * 8 * (kLinBlock / 64) * (size_t)P.nbx);
        if (ce != hipSuccess) { (void)hipStreamSynchronize(c->stream); return bail("copying the debug dump back", ce); }
    }
    c->n_launches += 1; c->n_poses_launched += P.n_poses; c->n_points_launched += (int64_t)P.n_poses * L.n;
    if (L.uses_state(c)) {
        // (lin_plan's advance rule: the first six-neighbour launch the rule puts behind five-neighbour launches, and the two after it)
        if (P.five) c->five_tail = 0;
        else if (c->opt_search_five == 1 && L.state_was_valid && L.state_was_five) c->five_tail = 2;
        else if (c->five_tail > 0) c->five_tail -= 1;
        c->state_valid = true; c->state_five = P.five;       // once this launch has run, the state holds a search of the current clouds
    }
    S.pending = true; S.plan = P; S.timed = timed; S.seq = seq; S.sync = L.dbg != nullptr;
    S.coded = L.a.count_scale != 0.0;        // how THIS launch's count slots are to be read (the source may be replaced while it is pending)
    if (gated) {
        c->gate_slot = L.slot;
        c->gate_uses_state = L.uses_state(c); c->gate_state_was_valid = L.state_was_valid; c->gate_state_was_five = L.state_was_five;
    }
    return DCREG_OK;
}

// gated = true: a single-pose launch whose pose arrives later through the gate (R9, t3 ignored; dcreg_linearize_gate_open /
// _gate_abort decide its fate)
// frame_ids != null: pose i linearises frame frame_ids[i] of the frames loaded by dcreg_frames_load instead of the ctx's source, with the
// frames' own neighbour states (state_ids name those); the ctx's source and states are not touched
// grid_ids != null (with frame_ids): the scan pairs of dcreg_register_pairs - pose i linearises source frame_ids[i] of the pairs' sources
// against target grid_ids[i] of the pairs' build batch (kernels.hpp k_lin GRIDS); the ctx's target and window index are not touched
static int linearize_begin(dcreg_ctx *c, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                           const dcreg_lin_params *p, dcreg_lin_debug *dbg_host, bool gated = false, const int32_t *frame_ids = nullptr,
                           const int32_t *grid_ids = nullptr) {
    if (!c) return DCREG_E_INVALID;
    LinLaunch L{slot, n_poses, R9, t3, state_ids, frame_ids, grid_ids, p, dbg_host, gated ? LinKind::gated : LinKind::single};
    if (int rc = lin_check(c, L)) return rc;
    if (c->need_set_device) { HIP_TRY(c, hipSetDevice(c->device)); }
    // which index the launch searches (context.hpp, the window of a large map): single-pose product launches the window around their pose, a
    // gated launch whatever is active (its pose is checked when the gate opens, against the window's pad: a gated launch whose search radius
    // needs a larger pad than the window was built with runs on the whole map), everything else the whole map
    if (gated && c->roi_active && roi_pad_for(c, p->search_radius) > c->roi_pad) (void)roi_deactivate(c);
    if (!gated && L.kind != LinKind::pairs && (c->roi_active || roi_wanted(c))) {
        const bool product = L.kind == LinKind::single || L.kind == LinKind::stamps;
        if (int rc = product ? roi_ensure(c, L.R9, L.t3, p->search_radius) : roi_deactivate(c)) return rc;
    }
    L.a = make_lin_args(c, p, L.kind != LinKind::pairs, L.n);
    // the parameters the stored certificates, gate bits and planes depend on (context.hpp StateKey): a launch with other values
    // starts from empty states.  (weight_slope, weight_min and use_weight_derivative are not among them: the weight gate and the row
    // are evaluated on the stored plane in every launch - tests/test_gpu_gate_edges.py alternates them on one context.)
    const LinArgs &a = L.a;
    L.key.radius_sq = a.radius_sq; L.key.max_thick_sq = a.max_thick_sq; L.key.min_norm = a.min_norm;
    L.key.radius_sq_f = a.radius_sq_f; L.key.cert_r_out = a.cert_r_out; L.key.cert_r_in = a.cert_r_in; L.key.fast_plane = c->opt_fast_plane ? 1 : 0;
    if (L.own() && !gated) {
        const double jump = c->last_pose_valid ? pose_jump(c, L.R9, L.t3, c->last_R, c->last_t) : 1e300;
        // (five-neighbour launches, lin_plan: a launch the engine announced as the start of a run is a step of a trajectory, as long as
        //  its pose; anything else is a call nobody said anything about)
        c->last_step = c->hint_unknown ? jump : 0.0;
        if (c->hint_unknown && jump <= 0.5 * c->map.grid.h) c->hint_misalign = c->hint_last;      // the same trajectory, continued
        // ... and what the last completed launch searched says nothing about a launch half a cell or more away from it (the first
        // launch of a new run): expect a search of everything - for this launch and for the one that may be queued behind it before
        // its counts are known (scheduling only: which kernels carry the launch out)
        if (jump > 0.5 * c->map.grid.h) { c->last_searched = c->n_src; c->last_points = c->last_searched; }
        c->hint_unknown = false;
        std::memcpy(c->last_R, L.R9, sizeof(c->last_R)); std::memcpy(c->last_t, L.t3, sizeof(c->last_t));
        c->last_pose_valid = true;
    }
    if (!gated && order_wanted(c, L)) {
        // the estimate holds for poses near the one it was made at (within a cell for every point)
        bool stale = !c->order_valid;
        // (counted in c->seq, the launch number that is never reset: round 6 found this test dead - it compared with n_launches, which
        //  dcreg_launch_stats_get(reset) zeroes, so that after one reset of the statistics the order of the moment was kept for good; with
        //  `bench.py --steps 20 --warmup 5` that was the order estimated at an ALIGNED pose, i.e. none: 355 / 314 / 260 us for the first
        //  launches of every later run instead of 264 / 216 / 205)
        if (!stale && (int64_t)c->seq - c->est_launch >= 16)       // (a loop of ungated launches does not re-estimate at every step)
            stale = pose_jump(c, L.R9, L.t3, c->est_R, c->est_t) > c->map.grid.h;
        if (int rc = stale ? estimate_dispatch_order(c, L.R9, L.t3, a.max_ring) : DCREG_OK) return rc;
    }
    // the ctx's own state (single-pose kinds)
    if (L.uses_state(c) && !(L.key == c->state_key)) { c->state_valid = false; c->state_key = L.key; }
    L.state_was_valid = c->state_valid; L.state_was_five = c->state_five;
    L.one.state = kNoIdx; L.one.fresh = 1;
    if (L.own()) {
        std::memcpy(L.one.R, L.R9, sizeof(L.one.R)); std::memcpy(L.one.t, L.t3, sizeof(L.one.t));
        if (c->opt_warm) {
            const size_t stride = ((size_t)L.n + 63) & ~(size_t)63;
            if (!c->state_valid || c->state_stride != stride) {
                if (c->d_state.ensure(c, kStateRows * stride)) return DCREG_E_NOMEM;
                c->state_stride = stride; c->state_valid = false;
            }
            L.one.state = 0; L.one.fresh = c->state_valid ? 0u : 1u;
            L.a.state = c->d_state.data(); L.a.state_stride = (uint32_t)c->state_stride;
        }
    }
    const LinPlan P = lin_plan(c, L, L.one.fresh != 0u);
    LinSlot &S = c->slots[slot];
    if (int rc = lin_reserve(c, S, L, P)) return rc;
    return c->opt_fast_plane ? lin_queue<true>(c, S, L, P) : lin_queue<false>(c, S, L, P);
}

// wait for the result rows of a launch.  Hot path: spin on the rows the kernels publish into pinned host memory (check word).  A
// launch may be slow but healthy (a GPU shared with other processes, huge clouds), and while it is awaited a gate for the NEXT launch
// may already sit in the stream: a stream synchronise would then wait for that gate, i.e. for this very thread.  So the wait is
// bounded by wall-clock time (far below the gate's own patience); only when it runs out is the stream drained - after calling the
// waiting gate off - to surface a device fault instead of hanging.
static int wait_rows(dcreg_ctx *c, LinSlot &S) {
    using Clk = std::chrono::steady_clock;
    Clk::time_point t0;
    bool clocked = false;
    const uint64_t every = c->opt_wait_seconds < 1.0 ? ((1ull << 6) - 1) : ((1ull << 20) - 1);      // (sub-second patience: tests of this path)
    // a row has arrived when its check word fits the 31 values next to it (kernels.hpp publish_row).  The row is copied out in one
    // piece (plain loads behind a compiler barrier: a torn snapshot fails the check and is read again) and the snapshot that was
    // checked is the one that is used.
    static const struct Mults { unsigned long long m[kSlots]; Mults() { for (int k = 0; k < kSlots; ++k) m[k] = row_check_mult(k); } } mults;
    auto arrived = [&](size_t i) {
        unsigned long long v[kSlots];
        asm volatile("" ::: "memory");
        std::memcpy(v, (const void *)(S.h_out.data() + i * kSlots), sizeof(v));
        unsigned long long c0 = S.seq * mults.m[31], c1 = 0, c2 = 0, c3 = 0;
        for (int k = 0; k < 28; k += 4) { c0 += v[k] * mults.m[k]; c1 += v[k + 1] * mults.m[k + 1]; c2 += v[k + 2] * mults.m[k + 2]; c3 += v[k + 3] * mults.m[k + 3]; }
        c0 += v[28] * mults.m[28]; c1 += v[29] * mults.m[29]; c2 += v[30] * mults.m[30];
        if (c0 + c1 + c2 + c3 != v[31]) return false;
        std::memcpy(S.h_rows.data() + i * kSlots, v, sizeof(v));
        S.row_chk[i] = v[31];
        return true;
    };
    // (cheap look first: a row whose check word is still the one taken last time has not been written again - the word carries the
    // launch number)
    auto touched = [&](size_t i) {
        return __atomic_load_n((const unsigned long long *)(S.h_out.data() + i * kSlots) + 31, __ATOMIC_RELAXED) != S.row_chk[i];
    };
    S.h_rows.resize(S.plan.n_rows * kSlots);
    // rows are taken in the order they arrive (the last one to come is then the only one left to check), not in index order
    S.row_done.assign(S.plan.n_rows, 0);
    if (S.row_chk.size() < S.plan.n_rows) S.row_chk.resize(S.plan.n_rows, 0ull);
    size_t pending = S.plan.n_rows;
    uint64_t spins = 0;
    while (pending) {
        for (size_t i = 0; i < S.plan.n_rows; ++i)
            if (!S.row_done[i] && touched(i) && arrived(i)) { S.row_done[i] = 1; --pending; }
        if (!pending) break;
        __builtin_ia32_pause();
        if ((++spins & every) != 0) continue;
        if (!clocked) { t0 = Clk::now(); clocked = true; continue; }
        if (std::chrono::duration<double>(Clk::now() - t0).count() < c->opt_wait_seconds) continue;
        if (c->gate_slot >= 0) (void)dcreg_linearize_gate_abort(c);      // nothing may wait behind us while we drain the stream
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { c->fail("device fault while waiting for a linearisation: %s", hipGetErrorString(e)); return DCREG_E_DEVICE; }
        for (size_t i = 0; i < S.plan.n_rows; ++i)
            if (!S.row_done[i]) {
                if (!arrived(i)) { c->fail("linearisation result never arrived"); return DCREG_E_DEVICE; }
                S.row_done[i] = 1; --pending;
            }
    }
    return DCREG_OK;
}

static int linearize_end(dcreg_ctx *c, int slot, dcreg_lin_out *outs) {
    if (!c) return DCREG_E_INVALID;
    if (slot < 0 || slot >= dcreg_ctx::kLinSlots) { c->fail("invalid slot"); return DCREG_E_INVALID; }
    LinSlot &S = c->slots[slot];
    if (!S.pending) { c->fail("slot %d has no linearisation in flight", slot); return DCREG_E_STATE; }
    if (!outs) { c->fail("null argument"); return DCREG_E_INVALID; }
    S.pending = false;
    int rc = DCREG_OK;
    if (S.sync || !c->opt_spin) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { c->fail("hipStreamSynchronize failed: %s", hipGetErrorString(e)); rc = DCREG_E_DEVICE; }
        if (rc == DCREG_OK && S.sync) { const hipError_t e2 = hipGetLastError(); if (e2 != hipSuccess) { c->fail("%s", hipGetErrorString(e2)); rc = DCREG_E_DEVICE; } }
        if (rc == DCREG_OK) rc = wait_rows(c, S);       // (the stream is drained: the rows are there; this checks and snapshots them)
    } else {
        rc = wait_rows(c, S);
    }
    free_tmp(S);
    if (rc != DCREG_OK) { drop_warm(c); return rc; }       // what the launch left in the states is unknown
    S.tickets_dirty = false;   // every chunk published its row: all tickets are back to zero
    float launch_ms = -1.f;
    if (S.timed) {
        float ms = 0.f;
        hipError_t te = hipEventElapsedTime(&ms, S.ev0, S.ev1);
        if (te == hipErrorNotReady) { HIP_TRY(c, hipEventSynchronize(S.ev1)); te = hipEventElapsedTime(&ms, S.ev0, S.ev1); }
        HIP_TRY(c, te);
        c->kernel_ms_total += ms; c->kernel_launches += 1;
        launch_ms = ms;
    }
    double total[kSlots];
    const LinPlan &P = S.plan;
    if (P.direct) {  // the rows of the blocks of ONE chunk, added exactly as block_sum_rows adds them on the device (so a pose gives
                     // bitwise the same sums alone and in a batch): lane group g takes rows g, g + G, ..., then the G sums in order
        constexpr int G = kLinBlock / 32;
        for (int k = 0; k < 31; ++k) {
            double tot = 0.0;
            for (int g = 0; g < G; ++g) {
                double t = 0.0;
                for (size_t r = (size_t)g; r < P.n_rows; r += G) t += S.h_rows[r * kSlots + k];
                tot += t;
            }
            total[k] = 0.0 + tot;                            // (the chunk total enters a sum that starts at zero, as everywhere)
        }
    } else if (P.n_poses == 1) {   // add the chunk rows in index order (fixed order: deterministic)
        for (int k = 0; k < 31; ++k) total[k] = 0.0;
        for (uint32_t ch = 0; ch < P.n_chunks; ++ch) {
            const double *row = S.h_rows.data() + (size_t)ch * kSlots;
            for (int k = 0; k < 31; ++k) total[k] += row[k];
        }
    }
    // the count slots carry two numbers each when the launch was asked to report what it did (LinArgs::count_scale): exact integers
    const bool coded = S.coded;
    int64_t searched = coded ? 0 : -1, refitted = coded ? 0 : -1;
    for (int i = 0; i < P.n_poses; ++i) {
        const double *o = P.n_poses == 1 ? total : S.h_rows.data() + (size_t)i * kSlots;      // (batches: one row per pose)
        lin_out_of_row(o, outs[i]);
        if (coded) {
            const int64_t S26 = (int64_t)1 << 26;
            searched += outs[i].n_eff / S26; refitted += outs[i].n_pt / S26;
            outs[i].n_eff %= S26; outs[i].n_pt %= S26;
        }
    }
    c->last_points = (int64_t)P.n_poses * c->n_src;
    // (a point whose new certificate has no slack at all - distance ties - is served by an advance pass and searched again by k_lin: it is
    // counted twice.  The scheduling rules and the launch log read fractions: never more than every point.  ADVICE round 5)
    if (searched > c->last_points) searched = c->last_points;
    if (refitted > c->last_points) refitted = c->last_points;
    c->last_searched = searched; c->last_refitted = refitted;
    if (c->opt_record_launches && c->launch_series.size() < ((size_t)1 << 20))
        c->launch_series.push_back(dcreg_ctx::LaunchRec{(double)launch_ms, searched, refitted, c->last_points, P.passes(), P.structure()});
    return DCREG_OK;
}

int launch_linearize(dcreg_ctx *c, int n_poses, const double *R9, const double *t3, const dcreg_lin_params *p,
                     dcreg_lin_out *outs, dcreg_lin_debug *dbg_host) {
    if (c && !outs) { c->fail("null argument"); return DCREG_E_INVALID; }
    static const bool timing = std::getenv("DCREG_HOST_TIMING") != nullptr;     // diagnostic: where a blocking call's host time goes
    using Clk = std::chrono::steady_clock;
    const auto t0 = Clk::now();
    int rc = linearize_begin(c, 0, n_poses, R9, t3, nullptr, p, dbg_host);
    if (rc) return rc;
    const auto t1 = Clk::now();
    rc = linearize_end(c, 0, outs);
    if (rc && c) c->slots[0].pending = false;
    if (timing && c) {
        static double s_begin = 0.0, s_end = 0.0, s_between = 0.0;
        static long n = 0;
        static Clk::time_point last;
        const auto t2 = Clk::now();
        if (n > 0) s_between += std::chrono::duration<double, std::micro>(t0 - last).count();
        s_begin += std::chrono::duration<double, std::micro>(t1 - t0).count();
        s_end += std::chrono::duration<double, std::micro>(t2 - t1).count();
        last = t2;
        if (++n % 100 == 0)
            std::fprintf(stderr, "[dcreg host timing] %ld blocking linearisations: enqueue %.2f us, wait for the result %.2f us, caller between calls %.2f us (means)\n",
                         n, s_begin / n, s_end / n, s_between / (n - 1));
    }
    return rc;
}

// k-NN of arbitrary queries (host pointer) or of the transformed source cloud (q == nullptr)
int launch_knn(dcreg_ctx *c, const GridDev &grid, const float4 *d_q, int64_t n, int k, double max_radius, const PoseArg *pose,
               int32_t *d_idx, float *d_d2, bool sweep) {
    float bound = INFINITY;
    int max_ring;
    if (max_radius > 0.0 && std::isfinite(max_radius)) {
        const double r2 = max_radius * max_radius;
        float rf = (float)r2; if ((double)rf < r2) rf = std::nextafterf(rf, INFINITY);
        bound = std::nextafterf(rf, INFINITY);
        max_ring = rings_for_bound(grid, bound);
        if (max_ring < 0) max_ring = 100000;      // (the rule ran out: the walk still stops there, it does not sweep)
    } else {
        bound = 3.0e38f;
        max_ring = -1;   // unbounded: the kernel sweeps as many rings as the grid needs
    }
    PoseArg P{};
    if (pose) P = *pose;
    if (sweep) {       // the linearisation's way of covering what lies beyond the 27-cell block, in the plain kernel (k = 5, bounded)
        if (k != 5 || max_ring < 0 || !grid.ymask) { c->fail("the row sweep needs k = 5, a radius and the target grid"); return DCREG_E_INVALID; }
        hipLaunchKernelGGL((k_knn<5, true>), dim3(blocks(n, kBlock)), dim3(kBlock), 0, c->stream, d_q, (uint32_t)n, grid, bound, max_ring, P, pose ? 1 : 0, d_idx, d_d2);
        HIP_TRY(c, hipGetLastError());
        return DCREG_OK;
    }
    if (k == 1)
        hipLaunchKernelGGL(k_knn<1>, dim3(blocks(n, kBlock)), dim3(kBlock), 0, c->stream, d_q, (uint32_t)n, grid, bound, max_ring, P, pose ? 1 : 0, d_idx, d_d2);
    else
        hipLaunchKernelGGL(k_knn<5>, dim3(blocks(n, kBlock)), dim3(kBlock), 0, c->stream, d_q, (uint32_t)n, grid, bound, max_ring, P, pose ? 1 : 0, d_idx, d_d2);
    HIP_TRY(c, hipGetLastError());
    return DCREG_OK;
}

}  // namespace dcreg

using namespace dcreg;

void dcreg_ctx::fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof(err), fmt, ap);
    va_end(ap);
}

extern "C" {

int dcreg_backend_create(dcreg_ctx **out, int device) {
    if (!out) return DCREG_E_INVALID;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        std::fprintf(stderr, "[dcreg] no usable HIP device (%s); this library has no CPU fallback\n",
                     e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return DCREG_E_DEVICE;
    }
    if (device < 0 || device >= count) return DCREG_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return DCREG_E_DEVICE;
    dcreg_ctx *c = new (std::nothrow) dcreg_ctx();
    if (!c) return DCREG_E_NOMEM;
    c->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->n_cus = cus;
    }
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        c->d_scratch.alloc(256 / sizeof(uint32_t)) != hipSuccess) {
        delete c;
        return DCREG_E_DEVICE;
    }
    c->stream = c->own_stream;
    for (LinSlot &S : c->slots)       // "time_kernels": the events of each slot's launch (created here, not in a timed region)
        if (hipEventCreate(&S.ev0) != hipSuccess || hipEventCreate(&S.ev1) != hipSuccess) { S.ev0 = S.ev1 = nullptr; }
    *out = c;
    return DCREG_OK;
}

void dcreg_backend_destroy(dcreg_ctx *c) {
    if (!c) return;
    (void)dcreg_comm_destroy(c);
    (void)hipSetDevice(c->device);
    (void)dcreg_linearize_gate_abort(c);
    (void)hipStreamSynchronize(c->stream);
    if (c->h_stage_ev) (void)hipEventDestroy(c->h_stage_ev);
    if (c->null_ev) (void)hipEventDestroy(c->null_ev);
    kdtree_free(c->kd); c->kd = nullptr;
    for (LinSlot &S : c->slots) {
        if (S.ev0) (void)hipEventDestroy(S.ev0);
        if (S.ev1) (void)hipEventDestroy(S.ev1);
    }
    for (auto &B : c->nicp.batch) if (B.done) (void)hipEventDestroy(B.done);
    (void)hipEventDestroy(c->ev0); (void)hipEventDestroy(c->ev1);
    (void)hipStreamDestroy(c->own_stream);
    delete c;                         // (the buffers go with it)
}

const char *dcreg_last_error(const dcreg_ctx *c) { return c ? c->err : "null context"; }
// (dcreg_debug.h) the host translation units above the device seam leave their error text here
void dcreg_set_error_message(dcreg_ctx *c, const char *msg) { if (c && msg) c->fail("%s", msg); }

int dcreg_set_stream(dcreg_ctx *c, void *s) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    (void)hipStreamSynchronize(c->stream);
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return DCREG_OK;
}

int dcreg_set_option(dcreg_ctx *c, const char *key, double v) {
    if (!c || !key) return DCREG_E_INVALID;
    const std::string k(key);
    if (k == "cell") c->opt_cell = v;
    else if (k == "cell_factor") c->opt_cell_factor = v > 0.1 ? v : 2.0;
    else if (k == "use_certificates") c->opt_use_cert = v != 0.0;
    else if (k == "count_searches") {
        if (v != 0.0 && !c->d_search_count) {
            HIP_TRY(c, c->d_search_count.alloc(kSearchCountBytes / sizeof(unsigned long long)));
            HIP_TRY(c, hipMemsetAsync(c->d_search_count.data(), 0, kSearchCountBytes, c->stream));
        }
        c->opt_count_searches = v != 0.0;
    }
    else if (k == "cert_margin" || k == "cert_inflate" || k == "warm_start" || k == "fast_plane_fit") {
        // options the neighbour states depend on: not while a queued launch may still write them (a later _gate_abort would also
        // restore state_valid, undoing the drop)
        if (c->gate_slot >= 0) { c->fail("a gated linearisation is queued: open or abort it before changing \"%s\"", key); return DCREG_E_STATE; }
        if (k == "cert_margin") c->opt_cert_margin = v >= 1e-4 ? std::min(v, 1.0) : 1e-4;    // the cells follow at the next dcreg_set_target
        else if (k == "cert_inflate") c->opt_cert_inflate = v >= 0.0 ? std::min(v, 1.0) : 0.0;
        else if (k == "warm_start") c->opt_warm = v != 0.0;
        else c->opt_fast_plane = v != 0.0;   // 1 (default) = plane_fit_qr_fast, 0 = the Eigen-shaped plane_fit_qr
        drop_warm(c);
    }
    else if (k == "wait_seconds") c->opt_wait_seconds = v > 0.0 ? v : 30.0;
    else if (k == "x_subdiv") { int sx = 1; while (sx < 16 && (double)(sx * 2) <= v) sx *= 2; c->opt_x_subdiv = sx; }
    else if (k == "time_kernels") { c->opt_time_kernels = v > 0.0 ? (int)v : 0; c->launch_counter = 0; }
    else if (k == "record_launches") { c->opt_record_launches = v != 0.0; if (v == 0.0) c->launch_series.clear(); }
    else if (k == "curve_x_scale") c->opt_curve_x_scale = (v > 0.0 && v <= 1.0) ? v : 1.0;   // next dcreg_set_source: patches of the curve order 1 / v times as long in x
    else if (k == "roi_index") { c->opt_roi_index = (int)std::min(std::max(v, 0.0), 2.0); c->roi_built = false; }   // 0 never, 1 auto, 2 always (next single-pose launch)
    else if (k == "roi_margin") { c->opt_roi_margin = std::min(std::max(v, 0.0), 1.0e6); c->roi_built = false; }
    else if (k == "pair_max_table_entries") c->opt_pair_max_table_entries = (int64_t)std::min(std::max(v, 4096.0), 2147483648.0);   // per target of dcreg_register_pairs
    else if (k == "pairs_max_bytes") c->opt_pairs_max_bytes = std::max(v, 0.0);     // device bytes of one build batch of dcreg_register_pairs (0: a quarter of the free memory)
    else if (k == "visibility_max_bytes") c->opt_visibility_max_bytes = std::max(v, 0.0);   // device bytes of the range images of one batch of members (visibility.hip)
    else if (k == "visibility_order") c->opt_visibility_order = (int)v;   // dcreg_target_remove_dynamic votes over the map in index order (0) or in cell order (1, default)
    else if (k == "max_table_entries") c->opt_max_table_entries = (int64_t)std::min(std::max(v, 1048576.0), 2147483648.0);   // next dcreg_set_target
    else if (k == "advance") c->opt_advance = (int)v;            // the advance pass in front of single-pose launches: 0 never, 1 (default) by the host's rule, 2 whenever possible
    else if (k == "advance_fused") c->opt_advance_fused = (int)v;   // ... carried out by one kernel (1, default: the pass builds the rows itself) or by k_advance + k_lin (0)
    else if (k == "one_wave") c->opt_one_wave = (int)v;                  // k_lin in one-wave blocks: 0 never, 1 by the rule (launches of many blocks in which most waves search), 2 wherever possible
    else if (k == "one_wave_batches") c->opt_one_wave_batches = v != 0.0;
    else if (k == "one_wave_min_frac") c->opt_one_wave_min_frac = v;
    else if (k == "one_wave_min_cells") c->opt_one_wave_min_cells = v;
    else if (k == "one_wave_min_blocks") c->opt_one_wave_min_blocks = (int)v;
    else if (k == "gate_in_kernel") c->opt_gate_in_kernel = v != 0.0;     // pipelined launches of at most 64 query blocks wait for their pose in their first kernel (1, default) or behind k_gate (0)
    else if (k == "team_stamps") c->opt_team_stamps = v != 0.0;   // timing probe of the small-frame pass (dcreg_team_pass_stamps)
    else if (k == "team_pass") c->opt_team_pass = (int)v;        // the small-frame advance pass: 0 never, 1 (default) by the host's rule, 2 whenever possible
    else if (k == "advance_min_blocks") c->opt_advance_min_blocks = (int)v;   // ... and the cloud has at least this many query blocks
    else if (k == "search_five") c->opt_search_five = (int)std::min(std::max(v, 0.0), 2.0);     // five-neighbour launches: 0 never, 1 (default) by the rule of lin_plan, 2 wherever possible
    else if (k == "search_five_step") c->opt_search_five_step = std::max(v, 0.0);             // ... the rule's step, in cell edges
    else if (k == "search_five_frac") c->opt_search_five_frac = std::min(std::max(v, 0.0), 1.0);   // ... and its searched share
    else if (k == "team_search") c->opt_team_max = (int)v;        // lanes a sparse wave serves cooperatively (0 = off, default 7)
    else if (k == "spin") c->opt_spin = v != 0.0;
    else if (k == "far_bound") c->opt_far_bound = v != 0.0;       // next dcreg_set_target: start bound of far queries from the nearest occupied cell
    else if (k == "dispatch_order") { c->opt_dispatch_order = v != 0.0; c->order_valid = false; }   // heavy query groups first (kernels.hpp k_group_cost)
    else if (k == "keep_source_order") c->opt_keep_source_order = v != 0.0;   // next dcreg_set_source: no Hilbert sort
    else if (k == "gap_field") c->opt_gap_field = v != 0.0;      // takes effect at the next dcreg_set_target
    else if (k == "map_update") c->opt_map_update = v != 0.0 ? 1 : 0;    // dcreg_target_insert / _crop: 1 merge into the current grid where possible, 0 always re-derive it
    else if (k == "normals_follow") c->opt_normals_follow = v != 0.0 ? 1 : 0;   // map updates refit the kept normals of dcreg_target_normals_keep instead of dropping them
    else if (k == "normals_follow_full_share") c->opt_normals_follow_full_share = std::min(std::max(v, 0.0), 1.0);   // dirty share past which a followed update recomputes everything (no result depends on it)
    else if (k == "voxels_follow") c->opt_voxels_follow = v != 0.0 ? 1 : 0;     // map updates refit the kept voxel map of dcreg_target_voxels_keep instead of dropping it
    else if (k == "voxels_follow_full_share") c->opt_voxels_follow_full_share = std::min(std::max(v, 0.0), 1.0);   // share of points in touched voxels past which a followed update runs the full keep (no result depends on it)
    else if (k == "gicp_epsilon") {                              // dcreg_linearize_gicp: the small eigenvalue of both plane covariances, read at every call
        if (!(v >= 1.0e-6 && v <= 1.0)) { c->fail("gicp_epsilon is %g: 1e-6 .. 1 expected", v); return DCREG_E_INVALID; }
        c->opt_gicp_epsilon = v;
    }
    else if (k == "robust_kernel") {                             // dcreg_linearize_normals / _gicp and every form built on them: read at every launch
        if (!(v == (double)DCREG_ROBUST_NONE || v == (double)DCREG_ROBUST_HUBER || v == (double)DCREG_ROBUST_CAUCHY || v == (double)DCREG_ROBUST_GEMAN_MCCLURE)) {
            c->fail("robust_kernel is %g: 0 (none), 1 (Huber), 2 (Cauchy) or 3 (Geman-McClure) expected", v); return DCREG_E_INVALID;
        }
        c->opt_robust_kernel = (int)v;
    }
    else if (k == "robust_scale" || k == "gicp_robust_scale") {  // the kernel's scale c: metres for the second engine, whitened units for the third
        if (!(v >= 1.0e-6 && v <= 1.0e6)) { c->fail("%s is %g: 1e-6 .. 1e6 expected", key, v); return DCREG_E_INVALID; }
        (k == "robust_scale" ? c->opt_robust_scale : c->opt_gicp_robust_scale) = v;
    }
    else if (k == "voxels_source_cov") {                         // dcreg_linearize_voxels: 0 point-to-distribution, 1 distribution-to-distribution, read at every call
        if (!(v == 0.0 || v == 1.0)) { c->fail("voxels_source_cov is %g: 0 or 1 expected", v); return DCREG_E_INVALID; }
        c->opt_voxels_source_cov = (int)v;
    }
    else if (k == "voxels_neighbors") {                          // dcreg_linearize_voxels: the stencil of voxels a point is matched to (1, 7 or 27), read at every call
        if (!(v == 1.0 || v == 7.0 || v == 27.0)) { c->fail("voxels_neighbors is %g: 1, 7 or 27 expected", v); return DCREG_E_INVALID; }
        c->opt_voxels_neighbors = (int)v;
    }
    else if (k == "feature_match_split") c->opt_feature_match_split = (int64_t)std::min(std::max(v, 0.0), 2147483647.0);   // dcreg_feature_match: rows of b per block column (0: from the sizes; no result depends on it)
    else if (k == "align_score_split") c->opt_align_score_split = (int64_t)std::min(std::max(v, 0.0), 2147483647.0);   // dcreg_align_correspondences: used pairs per block column of k_align_score (0: from the sizes; no result depends on it)
    else if (k == "verify_poses_per_launch") c->opt_verify_poses_per_launch = (int64_t)std::min(std::max(v, 0.0), 65535.0);   // dcreg_verify_poses*: poses per launch of k_verify (0: all; no result depends on it)
    else if (k == "map_grow_margin") c->opt_map_grow_margin = std::min(std::max(v, 0.0), 1.0e4);   // metres around the map when an update re-derives the grid
    else { c->fail("unknown option '%s'", key); return DCREG_E_INVALID; }
    return DCREG_OK;
}

int dcreg_set_target(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, double r) { return set_target(c, xyz, n, stride, r, false); }
int dcreg_set_target_device(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, double r) { return set_target(c, xyz, n, stride, r, true); }
int dcreg_target_insert(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const double R[9], const double t[3], double min_spacing,
                        dcreg_map_update *info) {
    return map_insert(c, xyz, n, stride, false, false, R, t, min_spacing, info);
}
int dcreg_target_insert_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride, const double R[9], const double t[3], double min_spacing,
                               dcreg_map_update *info) {
    return map_insert(c, d_xyz, n, stride, true, false, R, t, min_spacing, info);
}
int dcreg_target_insert_source(dcreg_ctx *c, const double R[9], const double t[3], double min_spacing, dcreg_map_update *info) {
    return map_insert(c, nullptr, 0, 3, false, true, R, t, min_spacing, info);
}
int dcreg_target_crop(dcreg_ctx *c, const double lo[3], const double hi[3], dcreg_map_update *info) { return map_crop(c, lo, hi, info); }
int dcreg_target_get(const dcreg_ctx *c, float *xyz_out, int64_t capacity_points) { return target_get(c, xyz_out, capacity_points); }
int dcreg_debug_index_check(dcreg_ctx *c, int64_t mismatches[5]) {
    if (!c || !mismatches) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (whole_map(c).n <= 0) { c->fail("no target"); return DCREG_E_STATE; }
    HIP_TRY(c, hipSetDevice(c->device));
    return index_check(c, mismatches);
}
int dcreg_set_source(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride) { return set_source(c, xyz, n, stride, false); }
int dcreg_set_source_device(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride) { return set_source(c, xyz, n, stride, true); }

// dcreg_set_source_voxel* / dcreg_set_target_voxel*: the voxel pass writes its output packed into c->d_aligned.data() - where set_source / set_target
// upload and check a cloud - with its bounds from the pass's one readback, and the commit of the plain calls takes it from there
static void voxel_info(dcreg_voxel_info *info, const VoxelResult &r) {
    if (info) { info->n_in = r.n_in; info->n_finite = r.n_finite; info->n_voxels = r.n_voxels; info->n_out = r.n_out; }
}
static int set_cloud_voxel(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, const dcreg_voxel_params *p, bool target,
                           double radius_hint, dcreg_voxel_info *info, DeskewRun *dsk = nullptr, dcreg_deskew_info *dinfo = nullptr,
                           const GatherRun *gat = nullptr) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (n <= 0) { c->fail("%s cloud is null or empty", target ? "target" : "measure"); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t off[2] = {0, n};
    VoxelResult r;
    int rc = voxel_pass(c, 1, xyz, off, stride, on_device, p, true, r, dsk, gat);
    if (rc) return rc;
    voxel_info(info, r);
    if (dsk) deskew_info(*dsk, n, dinfo);
    if (r.n_out <= 0) { c->fail("no point of the %s cloud is left after the voxel pass", target ? "target" : "measure"); return DCREG_E_INVALID; }
    if (target) {
        const double box[6] = {r.mn[0], r.mn[1], r.mn[2], r.mx[0], r.mx[1], r.mx[2]};
        return target_commit(c, r.n_out, box, radius_hint);
    }
    return source_commit(c, r.n_out, r.mn, r.mx, true);
}
// dcreg_set_source_deskew*: the records are deskewed while they are packed into c->d_aligned.data() (upload_cloud), then everything goes on
// as dcreg_set_source (bounds on the device - the deskewed points are not on the host -, a non-finite point refuses) or as
// dcreg_set_source_voxel goes on
// (pt: the path form, dcreg_set_source_deskew_path*; m otherwise)
static int set_source_deskew(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, const dcreg_time_field *f,
                             const dcreg_sweep_motion *m, const PathTable *pt, const dcreg_voxel_params *p, dcreg_deskew_info *info,
                             dcreg_voxel_info *vinfo) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (n <= 0) { c->fail("measure cloud is null or empty"); return DCREG_E_INVALID; }
    const int64_t off[2] = {0, n};
    DeskewRun d;
    int rc = pt ? deskew_path_prepare(c, 1, off, stride, f, *pt, d) : deskew_prepare(c, 1, off, stride, f, m, d);
    if (rc) return rc;
    if (p) return set_cloud_voxel(c, xyz, n, stride, on_device, p, false, 0.0, vinfo, &d, info);
    HIP_TRY(c, hipSetDevice(c->device));
    rc = upload_cloud(c, xyz, n, stride, on_device, c->d_aligned, &d);
    if (rc) return rc;
    double mn[3], mx[3];
    rc = device_bounds(c, c->d_aligned.data(), n, mn, mx, &d);
    if (rc) return rc;
    deskew_info(d, n, info);
    for (int a = 0; a < 3; ++a) if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) { c->fail("source cloud has non-finite coordinates"); return DCREG_E_INVALID; }
    return source_commit(c, n, mn, mx, true);
}
int dcreg_set_source_deskew(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const dcreg_time_field *f, const dcreg_sweep_motion *m,
                            const dcreg_voxel_params *p, dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    return set_source_deskew(c, xyz, n, stride, false, f, m, nullptr, p, info, vinfo);
}
int dcreg_set_source_deskew_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride, const dcreg_time_field *f, const dcreg_sweep_motion *m,
                                   const dcreg_voxel_params *p, dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    return set_source_deskew(c, d_xyz, n, stride, true, f, m, nullptr, p, info, vinfo);
}
int dcreg_set_source_deskew_path(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const dcreg_time_field *f, int64_t n_knots,
                                 const double *knot_stamps, const double *knot_poses, const dcreg_sweep_path *path, const dcreg_voxel_params *p,
                                 dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    const PathTable pt = {n_knots, knot_stamps, knot_poses, path};
    return set_source_deskew(c, xyz, n, stride, false, f, nullptr, &pt, p, info, vinfo);
}
int dcreg_set_source_deskew_path_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride, const dcreg_time_field *f, int64_t n_knots,
                                        const double *knot_stamps, const double *knot_poses, const dcreg_sweep_path *path,
                                        const dcreg_voxel_params *p, dcreg_deskew_info *info, dcreg_voxel_info *vinfo) {
    const PathTable pt = {n_knots, knot_stamps, knot_poses, path};
    return set_source_deskew(c, d_xyz, n, stride, true, f, nullptr, &pt, p, info, vinfo);
}
int dcreg_set_source_voxel(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const dcreg_voxel_params *p, dcreg_voxel_info *info) {
    return set_cloud_voxel(c, xyz, n, stride, false, p, false, 0.0, info);
}
int dcreg_set_source_voxel_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride, const dcreg_voxel_params *p, dcreg_voxel_info *info) {
    return set_cloud_voxel(c, d_xyz, n, stride, true, p, false, 0.0, info);
}
int dcreg_set_target_voxel(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const dcreg_voxel_params *p, double r, dcreg_voxel_info *info) {
    return set_cloud_voxel(c, xyz, n, stride, false, p, true, r, info);
}
int dcreg_set_target_voxel_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride, const dcreg_voxel_params *p, double r,
                                  dcreg_voxel_info *info) {
    return set_cloud_voxel(c, d_xyz, n, stride, true, p, true, r, info);
}

// dcreg_set_source_outliers* / dcreg_set_target_outliers*: the cloud - packed by upload_cloud, or the packed output of the voxel pass - is
// filtered where it lies in c->d_aligned.data(), the kept points are packed beside it and swapped in, and the commit of the plain calls takes them
static int set_cloud_outliers(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, bool on_device, const dcreg_voxel_params *vp,
                              const dcreg_outlier_params *p, bool target, double radius_hint, dcreg_voxel_info *vinfo, dcreg_outlier_info *info) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (int rc = outlier_check(c, p)) return rc;
    if (n <= 0) { c->fail("%s cloud is null or empty", target ? "target" : "measure"); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    int64_t m = n;
    int rc;
    if (vp) {
        const int64_t off[2] = {0, n};
        VoxelResult v;
        rc = voxel_pass(c, 1, xyz, off, stride, on_device, vp, true, v);
        if (rc) return rc;
        voxel_info(vinfo, v);
        if (v.n_out <= 0) { c->fail("no point of the %s cloud is left after the voxel pass", target ? "target" : "measure"); return DCREG_E_INVALID; }
        m = v.n_out;
    } else {
        rc = upload_cloud(c, xyz, n, stride, on_device, c->d_aligned);
        if (rc) return rc;
    }
    OutlierResult r;
    rc = outlier_pass(c, c->d_aligned.data(), m, p, nullptr, r);
    if (rc) return rc;
    outlier_info(info, r);
    if (r.n_out <= 0) { c->fail("no point of the %s cloud is left after the outlier filter", target ? "target" : "measure"); return DCREG_E_INVALID; }
    rc = outlier_write_packed(c, c->d_aligned.data(), m, r.n_out);
    if (rc) return rc;
    c->d_aligned.swap(c->outl.out4);
    double box[6];
    rc = device_bounds(c, c->d_aligned.data(), r.n_out, box, box + 3);
    if (rc) return rc;
    if (target) return target_commit(c, r.n_out, box, radius_hint);
    return source_commit(c, r.n_out, box, box + 3, true);
}
int dcreg_set_source_outliers(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const dcreg_voxel_params *voxel, const dcreg_outlier_params *p,
                              dcreg_voxel_info *vinfo, dcreg_outlier_info *info) {
    return set_cloud_outliers(c, xyz, n, stride, false, voxel, p, false, 0.0, vinfo, info);
}
int dcreg_set_source_outliers_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride, const dcreg_voxel_params *voxel,
                                     const dcreg_outlier_params *p, dcreg_voxel_info *vinfo, dcreg_outlier_info *info) {
    return set_cloud_outliers(c, d_xyz, n, stride, true, voxel, p, false, 0.0, vinfo, info);
}
int dcreg_set_target_outliers(dcreg_ctx *c, const float *xyz, int64_t n, int64_t stride, const dcreg_voxel_params *voxel, const dcreg_outlier_params *p,
                              double r, dcreg_voxel_info *vinfo, dcreg_outlier_info *info) {
    return set_cloud_outliers(c, xyz, n, stride, false, voxel, p, true, r, vinfo, info);
}
int dcreg_set_target_outliers_device(dcreg_ctx *c, const float *d_xyz, int64_t n, int64_t stride, const dcreg_voxel_params *voxel,
                                     const dcreg_outlier_params *p, double r, dcreg_voxel_info *vinfo, dcreg_outlier_info *info) {
    return set_cloud_outliers(c, d_xyz, n, stride, true, voxel, p, true, r, vinfo, info);
}
int dcreg_target_remove_outliers(dcreg_ctx *c, const dcreg_outlier_params *p, dcreg_outlier_info *info) { return map_remove_outliers(c, p, info); }
int dcreg_target_remove_dynamic(dcreg_ctx *c, int64_t n_members, const int64_t *member_ids, const double *member_poses,
                                const dcreg_visibility_params *p, dcreg_visibility_info *info) {
    return map_remove_dynamic(c, n_members, member_ids, member_poses, p, info);
}

int dcreg_default_lin_params(dcreg_lin_params *p, double radius) {
    if (!p) return DCREG_E_INVALID;
    std::memset(p, 0, sizeof(*p));            // parameterization = DCREG_PARAM_SO3
    p->search_radius = radius; p->max_plane_thickness_sq = 0.2 * 0.2; p->min_normal_norm = 1e-6;
    p->weight_slope = 0.9; p->weight_min = 0.1; p->use_weight_derivative = 0; p->k = 5;
    return DCREG_OK;
}

int dcreg_linearize(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out) {
    return launch_linearize(c, 1, R, t, p, out, nullptr);
}
int dcreg_linearize_batch(dcreg_ctx *c, int n, const double *R9, const double *t3, const dcreg_lin_params *p, dcreg_lin_out *outs) {
    return launch_linearize(c, n, R9, t3, p, outs, nullptr);
}
int dcreg_linearize_batch_begin(dcreg_ctx *c, int slot, int n, const double *R9, const double *t3, const dcreg_lin_params *p) {
    return linearize_begin(c, slot, n, R9, t3, nullptr, p, nullptr);
}
int dcreg_linearize_batch_begin_warm(dcreg_ctx *c, int slot, int n, const double *R9, const double *t3, const int32_t *state_ids,
                                     const dcreg_lin_params *p) {
    return linearize_begin(c, slot, n, R9, t3, state_ids, p, nullptr);
}
int dcreg_reserve_warm_states(dcreg_ctx *c, int64_t n_states) {
    if (!c) return DCREG_E_INVALID;
    if (n_states < 0) { c->fail("negative state count"); return DCREG_E_INVALID; }
    for (const LinSlot &S : c->slots) if (S.pending) { c->fail("a linearisation is still in flight"); return DCREG_E_STATE; }
    c->n_batch_states = 0;
    c->batch_state_valid.clear();
    if (n_states == 0 || c->n_src <= 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t stride = ((size_t)c->n_src + 63) & ~(size_t)63;
    // nothing is cleared: a state is "fresh" (host-side flag) until its first launch has filled it
    if (c->d_state_batch.ensure(c, kStateRows * stride * (size_t)n_states)) return DCREG_E_NOMEM;
    c->state_batch_stride = stride;
    c->n_batch_states = n_states;
    c->batch_state_valid.assign((size_t)n_states, 0);
    return DCREG_OK;
}
int dcreg_hint_misalignment(dcreg_ctx *c, double metres) {
    if (!c) return DCREG_E_INVALID;
    if (metres >= 0.0) { c->hint_misalign = metres; c->hint_last = metres; c->hint_unknown = false; }
    else { c->hint_misalign = 1e300; c->hint_unknown = true; }            // (also NaN: no knowledge - resolved in linearize_begin)
    return DCREG_OK;
}
int dcreg_reset_warm_state(dcreg_ctx *c, int64_t state_id) {
    if (!c) return DCREG_E_INVALID;
    if (state_id == -1) {            // the context's own state (single-pose launches): as after dcreg_set_source - what a fresh ICPContext holds
        if (c->gate_slot >= 0) { c->fail("a gated linearisation is queued: open or abort it before dropping the neighbour state"); return DCREG_E_STATE; }
        for (const LinSlot &S : c->slots) if (S.pending) { c->fail("a linearisation is still in flight"); return DCREG_E_STATE; }
        c->state_valid = false;
        return DCREG_OK;
    }
    if (state_id < 0 || state_id >= c->n_batch_states) { c->fail("warm state %lld was not reserved", (long long)state_id); return DCREG_E_INVALID; }
    c->batch_state_valid[(size_t)state_id] = 0;
    return DCREG_OK;
}
int dcreg_linearize_batch_end(dcreg_ctx *c, int slot, dcreg_lin_out *outs) { return linearize_end(c, slot, outs); }
int dcreg_frames_load(dcreg_ctx *c, int n_frames, const float *xyz, const int64_t *frame_offsets, int64_t stride_floats) {
    if (c) for (const LinSlot &S : c->slots) if (S.pending) { c->fail("a linearisation is still in flight"); return DCREG_E_STATE; }
    if (c && c->nicp.batch_pending()) { c->fail("a batched normal linearisation is still in flight (dcreg_normals_batch_end first)"); return DCREG_E_STATE; }
    if (c) c->nicp.drop_slots();           // (normal_icp.hip: the warm slots of the batched form belong to the frames that were loaded)
    if (c) c->frames.normals_kept = false; // (normals.hip: ... and so do the frames' kept normals)
    return frames_load(c, c->frames, n_frames, xyz, frame_offsets, stride_floats);
}
static int frames_reserve_states(dcreg_ctx *c, dcreg_ctx::FrameSet &fs, int64_t n_states) {
    if (n_states < 0) { c->fail("negative state count"); return DCREG_E_INVALID; }
    for (const LinSlot &S : c->slots) if (S.pending) { c->fail("a linearisation is still in flight"); return DCREG_E_STATE; }
    fs.n_states = 0;
    fs.state_valid.clear();
    if (n_states == 0 || fs.max_points <= 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t stride = ((size_t)fs.max_points + 63) & ~(size_t)63;       // one stride: the largest frame's
    if (fs.state.ensure(c, kStateRows * stride * (size_t)n_states)) return DCREG_E_NOMEM;
    fs.state_stride = stride;
    fs.n_states = n_states;
    fs.state_valid.assign((size_t)n_states, 0);
    return DCREG_OK;
}
static int frames_reset_state(dcreg_ctx *c, dcreg_ctx::FrameSet &fs, int64_t state_id) {
    if (state_id < 0 || state_id >= fs.n_states) { c->fail("frame state %lld was not reserved", (long long)state_id); return DCREG_E_INVALID; }
    fs.state_valid[(size_t)state_id] = 0;
    return DCREG_OK;
}
int dcreg_frames_reserve_states(dcreg_ctx *c, int64_t n_states) { return c ? frames_reserve_states(c, c->frames, n_states) : DCREG_E_INVALID; }
int dcreg_frames_reset_state(dcreg_ctx *c, int64_t state_id) { return c ? frames_reset_state(c, c->frames, state_id) : DCREG_E_INVALID; }
static int pairs_plan(dcreg_ctx *c, int n_pairs, const int64_t *tgt_offsets, int64_t stride_floats, double extra, int32_t *batch_end, int *n_batches,
                      bool voxels = false) {
    if (!c || n_pairs < 0 || !tgt_offsets || !batch_end || !n_batches) return DCREG_E_INVALID;
    // build batches of pair targets within the byte budget (pairs_budget): at least one pair each, fewer than 2^31 points each
    const double budget = pairs_budget(c);
    int nb = 0;
    double bytes = 0.0;
    int64_t pts = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t m = tgt_offsets[p + 1] - tgt_offsets[p];
        const double b = voxels ? pair_voxel_target_bytes(m, stride_floats) : pair_target_bytes(c, m, stride_floats, extra);
        if (p > 0 && (bytes + b > budget || pts + m >= ((int64_t)1 << 31) - 1)) { batch_end[nb++] = p; bytes = 0.0; pts = 0; }
        bytes += b; pts += m;
    }
    if (n_pairs > 0) batch_end[nb++] = n_pairs;
    *n_batches = nb;
    return DCREG_OK;
}
int dcreg_pairs_plan(dcreg_ctx *c, int n_pairs, const int64_t *tgt_offsets, int64_t stride_floats, int32_t *batch_end, int *n_batches) {
    return pairs_plan(c, n_pairs, tgt_offsets, stride_floats, 0.0, batch_end, n_batches);
}
// ... for the 1-NN engines: a batch also holds its targets' kept normals (16 B a point) and the scratch of their estimation (3 + 1 floats)
int dcreg_pairs_plan_normals(dcreg_ctx *c, int n_pairs, const int64_t *tgt_offsets, int64_t stride_floats, int32_t *batch_end, int *n_batches) {
    return pairs_plan(c, n_pairs, tgt_offsets, stride_floats, 32.0, batch_end, n_batches);
}
// ... for the fourth engine: a batch is counted with what pairs_voxels_build allocates (pair_voxel_target_bytes), not with a cell table
int dcreg_pairs_plan_voxels(dcreg_ctx *c, int n_pairs, const int64_t *tgt_offsets, int64_t stride_floats, int32_t *batch_end, int *n_batches) {
    return pairs_plan(c, n_pairs, tgt_offsets, stride_floats, 0.0, batch_end, n_batches, true);
}
int dcreg_pairs_sources_load(dcreg_ctx *c, int n_pairs, const float *xyz, const int64_t *src_offsets, int64_t stride_floats) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    // (normal_icp.hip: warm slots sized for the pairs' sources belong to the sources that were loaded, and so do their kept normals)
    if (c->nicp.slots_for == dcreg_ctx::NormalIcpBufs::SlotsFor::pairs) c->nicp.drop_slots();
    c->pair_src.normals_kept = false;
    return frames_load(c, c->pair_src, n_pairs, xyz, src_offsets, stride_floats);
}
int dcreg_pairs_build(dcreg_ctx *c, int n_targets, const float *xyz, const int64_t *tgt_offsets, int64_t stride_floats, double search_radius) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    return pairs_build(c, n_targets, xyz, tgt_offsets, stride_floats, search_radius);
}
int dcreg_pairs_reserve_states(dcreg_ctx *c, int64_t n_states) { return c ? frames_reserve_states(c, c->pair_src, n_states) : DCREG_E_INVALID; }
int dcreg_pairs_reset_state(dcreg_ctx *c, int64_t state_id) { return c ? frames_reset_state(c, c->pair_src, state_id) : DCREG_E_INVALID; }
int dcreg_pairs_batch_begin(dcreg_ctx *c, int slot, int n, const double *R9, const double *t3, const int32_t *state_ids, const int32_t *source_ids,
                            const int32_t *target_ids, const dcreg_lin_params *p) {
    if (c && (!source_ids || !state_ids || !target_ids)) { c->fail("null argument"); return DCREG_E_INVALID; }
    return linearize_begin(c, slot, n, R9, t3, state_ids, p, nullptr, false, source_ids, target_ids);
}
int dcreg_frames_batch_begin(dcreg_ctx *c, int slot, int n, const double *R9, const double *t3, const int32_t *state_ids, const int32_t *frame_ids,
                             const dcreg_lin_params *p) {
    if (c && (!frame_ids || !state_ids)) { c->fail("null argument"); return DCREG_E_INVALID; }
    return linearize_begin(c, slot, n, R9, t3, state_ids, p, nullptr, false, frame_ids);
}
int dcreg_linearize_gated_begin(dcreg_ctx *c, int slot, const dcreg_lin_params *p) {
    return linearize_begin(c, slot, 1, nullptr, nullptr, nullptr, p, nullptr, true);
}
int dcreg_linearize_gate_open(dcreg_ctx *c, const double R[9], const double t[3]) {
    if (!c) return DCREG_E_INVALID;
    if (c->gate_slot < 0 || !R || !t) { c->fail("no gated linearisation waits for a pose"); return DCREG_E_STATE; }
    if (!poses_finite(1, R, t)) { c->fail("a pose with non-finite entries: the gate still waits"); return DCREG_E_INVALID; }
    if (c->roi_active && !roi_covers(c, R, t, c->roi_pad)) {
        // the queued launch was built on a window this pose has left: it is called off; the caller starts the launch the plain way
        // (DCREG_E_STATE = "no launch waits", as after a timeout) and that builds the window around the new pose
        (void)dcreg_linearize_gate_abort(c);
        c->fail("the pose left the window of the map the queued launch was built on: launch called off");
        return DCREG_E_STATE;
    }
    gate_publish(c, c->gate_seq << 1, R, t);
    c->last_step = c->last_pose_valid ? pose_jump(c, R, t, c->last_R, c->last_t) : 1e300;
    std::memcpy(c->last_R, R, sizeof(c->last_R)); std::memcpy(c->last_t, t, sizeof(c->last_t));
    c->last_pose_valid = true;
    c->gate_slot = -1;
    return DCREG_OK;
}
int dcreg_linearize_gate_abort(dcreg_ctx *c) {
    if (!c) return DCREG_E_INVALID;
    if (c->gate_slot < 0) return DCREG_OK;                                  // nothing queued
    gate_call_off(c);
    LinSlot &S = c->slots[c->gate_slot];
    S.pending = false;                 // no result will come; tickets_dirty stays set, so the next launch of the slot clears them
    free_tmp(S);
    // the kernels behind the gate return without touching anything: the state, its pose and the list counters are as before
    if (c->gate_uses_state) { c->state_valid = c->gate_state_was_valid; c->state_five = c->gate_state_was_five; }
    c->gate_slot = -1;
    return DCREG_OK;
}
int dcreg_linearize_debug(dcreg_ctx *c, const double R[9], const double t[3], const dcreg_lin_params *p, dcreg_lin_out *out, dcreg_lin_debug *dbg) {
    return launch_linearize(c, 1, R, t, p, out, dbg);
}

int dcreg_knn(dcreg_ctx *c, const float *q, int64_t n, int64_t stride, int k, double max_radius, int32_t *idx, float *d2) {
    if (!c) return DCREG_E_INVALID;
    if (int rc = refuse_in_flight(c)) return rc;
    if (!q || !idx || !d2 || n < 0 || (k != 1 && k != 5)) { c->fail("invalid k-NN arguments (k must be 1 or 5)"); return DCREG_E_INVALID; }
    (void)roi_deactivate(c);
    if (c->map.n <= 0) { c->fail("target index is not set"); return DCREG_E_STATE; }
    if (n == 0) return DCREG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = upload_cloud(c, q, n, stride, false, c->d_aligned);
    if (rc) return rc;
    if (c->d_nn_idx.ensure(c, (size_t)n * k) || c->d_nn_d2.ensure(c, (size_t)n * k)) return DCREG_E_NOMEM;
    rc = launch_knn(c, c->map.grid, c->d_aligned.data(), n, k, max_radius, nullptr, c->d_nn_idx.data(), c->d_nn_d2.data());
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(idx, c->d_nn_idx.data(), sizeof(int32_t) * (size_t)n * k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d2, c->d_nn_d2.data(), sizeof(float) * (size_t)n * k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return DCREG_OK;
}

int dcreg_index_info_get(const dcreg_ctx *c, dcreg_index_info *info) {
    if (!c || !info) return DCREG_E_INVALID;
    const IndexSet &w = whole_map(c);
    const dcreg::GridDev &g = w.grid;
    info->cell = g.h;
    info->origin[0] = g.ox; info->origin[1] = g.oy; info->origin[2] = g.oz;
    info->dims[0] = g.nx; info->dims[1] = g.ny; info->dims[2] = g.nz;
    info->n_cells = w.n_cells; info->n_target = w.n;
    info->n_source = c->n_src; info->max_ring = c->last_max_ring;
    return DCREG_OK;
}

int dcreg_roi_info(const dcreg_ctx *c, double info[11]) {
    if (!c || !info) return DCREG_E_INVALID;
    for (int a = 0; a < 3; ++a) { info[a] = c->roi_lo[a]; info[3 + a] = c->roi_hi[a]; }
    const bool have = c->roi_built && !c->roi_empty;
    const IndexSet &win = c->roi_active ? c->map : c->roi_store;       // the window's index, whichever is active
    info[6] = have ? (double)win.n : 0.0;
    info[7] = have ? win.grid.h : 0.0;
    info[8] = (double)c->roi_rebuilds; info[9] = c->roi_active ? 1.0 : 0.0; info[10] = c->whole_capped ? 1.0 : 0.0;
    return DCREG_OK;
}

int dcreg_launch_stats_get(dcreg_ctx *c, dcreg_launch_stats *st, int reset) {
    if (!c || !st) return DCREG_E_INVALID;
    if (c->opt_count_searches && c->d_search_count) if (int rc = refuse_in_flight(c)) return rc;    // (the counters are read behind every launch)
    st->launches = c->n_launches; st->poses = c->n_poses_launched; st->points = c->n_points_launched;
    st->points_searched = -1; st->points_team = -1;
    if (c->opt_count_searches && c->d_search_count) {      // synchronous: every launch so far has finished when this returns
        std::vector<unsigned long long> v(kSearchCountBytes / sizeof(unsigned long long));
        HIP_TRY(c, hipMemcpyAsync(v.data(), c->d_search_count.data(), kSearchCountBytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        unsigned long long tot = 0, team = 0;
        for (size_t k = 0; k < v.size(); k += kCounterStride / 2) { tot += v[k]; team += v[k + 1]; }
        st->points_searched = (int64_t)tot;
        st->points_team = (int64_t)team;
        if (reset) HIP_TRY(c, hipMemsetAsync(c->d_search_count.data(), 0, kSearchCountBytes, c->stream));
    }
    if (reset) { c->n_launches = 0; c->n_poses_launched = 0; c->n_points_launched = 0; }
    return DCREG_OK;
}

int dcreg_launch_series(dcreg_ctx *c, double *ms, int64_t *searched, int64_t *refitted, int64_t *points, int64_t cap, int reset) {
    if (!c || cap < 0) return -1;
    const int64_t n = std::min<int64_t>(cap, (int64_t)c->launch_series.size());
    for (int64_t i = 0; i < n; ++i) {
        const dcreg_ctx::LaunchRec &r = c->launch_series[(size_t)i];
        if (ms) ms[i] = r.ms;
        if (searched) searched[i] = r.searched;
        if (refitted) refitted[i] = r.refitted;
        if (points) points[i] = r.points;
    }
    const int64_t total = (int64_t)c->launch_series.size();
    if (reset) c->launch_series.clear();
    return (int)std::min<int64_t>(total, 0x7FFFFFFF);
}

int dcreg_launch_series_passes(dcreg_ctx *c, uint8_t *advanced, int64_t cap) {
    if (!c || cap < 0) return -1;
    const int64_t n = std::min<int64_t>(cap, (int64_t)c->launch_series.size());
    for (int64_t i = 0; i < n; ++i) if (advanced) advanced[i] = (uint8_t)c->launch_series[(size_t)i].advanced;
    return (int)std::min<int64_t>((int64_t)c->launch_series.size(), 0x7FFFFFFF);
}

int dcreg_launch_series_structure(dcreg_ctx *c, uint8_t *structure, int64_t cap) {
    if (!c || cap < 0) return -1;
    const int64_t n = std::min<int64_t>(cap, (int64_t)c->launch_series.size());
    for (int64_t i = 0; i < n; ++i) if (structure) structure[i] = (uint8_t)c->launch_series[(size_t)i].structure;
    return (int)std::min<int64_t>((int64_t)c->launch_series.size(), 0x7FFFFFFF);
}

int dcreg_team_pass_stamps(dcreg_ctx *c, uint64_t *out, int64_t cap_blocks) {
    if (!c || cap_blocks < 0) return -1;
    if (!c->d_team_stamps || c->team_stamps_n == 0) return 0;
    const int64_t n = std::min<int64_t>(cap_blocks, (int64_t)c->team_stamps_n + 1);      // (+ 1: the outcome histogram behind the blocks)
    if (out && n > 0) {
        if (int rc = refuse_in_flight(c)) return rc;
        HIP_TRY(c, hipMemcpyAsync(out, c->d_team_stamps.data(), sizeof(unsigned long long) * 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return (int)std::min<int64_t>((int64_t)c->team_stamps_n, 0x7FFFFFFF);
}

int dcreg_kernel_time(dcreg_ctx *c, double *ms_total, int64_t *launches, int reset) {
    if (!c) return DCREG_E_INVALID;
    if (ms_total) *ms_total = c->kernel_ms_total;
    if (launches) *launches = c->kernel_launches;
    if (reset) { c->kernel_ms_total = 0.0; c->kernel_launches = 0; }
    return DCREG_OK;
}

}  // extern "C"

// dcreg_set_target_keyframes (keyframes.hip has checked the members): the gather stands where the upload of set_target / set_cloud_voxel stands
int dcreg::set_target_gathered(dcreg_ctx *c, const GatherRun &g, const dcreg_voxel_params *p, double radius_hint, dcreg_voxel_info *info) {
    if (p) return set_cloud_voxel(c, nullptr, g.n, 3, true, p, true, radius_hint, info, nullptr, nullptr, &g);
    if (g.n <= 0) { c->fail("target cloud is null or empty"); return DCREG_E_INVALID; }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = upload_cloud(c, nullptr, g.n, 3, true, c->d_aligned, nullptr, &g);
    if (rc) return rc;
    double box[6];
    rc = device_bounds(c, c->d_aligned.data(), g.n, box, box + 3);
    if (rc) return rc;
    for (int a = 0; a < 6; ++a) if (!std::isfinite(box[a])) { c->fail("target cloud has non-finite coordinates"); return DCREG_E_INVALID; }
    if (info) { info->n_in = info->n_finite = info->n_out = g.n; info->n_voxels = 0; }
    return target_commit(c, g.n, box, radius_hint);
}
