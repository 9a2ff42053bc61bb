/*
 * dcreg_debug.h -- test, profiling and experiment hooks of libdcreg_hip.so.  NOT part of the drop-in boundary (dcreg.h is; see
 * INTEGRATION.md): nothing a maintainer of the reference binds lives here.  Used by tests/, bench.py and scripts/.
 */
#ifndef DCREG_DEBUG_H
#define DCREG_DEBUG_H

#include "dcreg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-point dump for parity tests (original source order; any pointer may be NULL).
 * flag: 1 valid, 0 radius/knn gate, 2 |x|<min_normal_norm, 3 plane thickness, 4 weight<=weight_min.
 * nn_idx / nn_d2 are the reference's result list of nearestKSearch (icp_test_runner.cpp:1722) for the points that pass its radius
 * gate (:1726, flag != 0); for the others (flag 0) the reference never looks at the list and the dump holds -1 / +inf. */
typedef struct dcreg_lin_debug {
    int32_t *nn_idx; /* [5*n] original target indices, ascending (d2, idx); -1 = none */
    float *nn_d2;    /* [5*n] */
    uint8_t *flag;   /* [n] */
    double *normal;  /* [3*n] */
    double *r;       /* [n] */
    double *s;       /* [n] */
    uint32_t *stats; /* [n] search statistics: candidates evaluated | outermost shell << 16 */
    uint64_t *stamps; /* [8 * 4 * ceil(n / 256)] timing probe: per wave (query block x 4 + wave) shader-clock stamps at the phase boundaries
                         of the linearisation kernel + its searched / refitted lane counts.  With ONLY this pointer set the call is not a
                         dump: certificates are used as in a plain call and nothing else is copied back (scripts/wave_phases.py) */
} dcreg_lin_debug;

/* dcreg_linearize with the dump; always searches every point (k_full), shares the ctx's neighbour state with the plain calls */
int dcreg_linearize_debug(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *,
                          dcreg_lin_out *, dcreg_lin_debug *);

/* per-point dump of dcreg_linearize_normals (original source order; any pointer may be NULL).  flag: 1 effective, 0 radius gate,
 * 2 the nearest point has no normal, 4 weight <= weight_min.  nn_idx / nn_d2: the nearest map point (original index) and its float d2
 * for the points that pass the radius gate; -1 / +inf for flag 0.  normal: the kept normal of that point as stored (flag 2: with its
 * non-finite components), r and s for flags 1 and 4, row = [A0..A5, b, r] for flag 1; everything else is 0. */
typedef struct dcreg_nlin_debug {
    int32_t *nn_idx; /* [n] */
    float *nn_d2;    /* [n] */
    uint8_t *flag;   /* [n] */
    double *normal;  /* [3*n] */
    double *r;       /* [n] */
    double *s;       /* [n] */
    double *row;     /* [8*n] */
} dcreg_nlin_debug;
/* dcreg_linearize_normals with the dump; searches every point cold and leaves the warm bounds of the plain calls as they were */
int dcreg_linearize_normals_debug(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *, dcreg_lin_out *,
                                  dcreg_nlin_debug *);

/* per-point dump of dcreg_linearize_gicp (original source order; any pointer may be NULL).  flag: 1 effective, 0 radius gate, 2 the
 * nearest map point has no normal, 3 the source point has none, 5 the pair's covariance is not positive definite.  nn_idx / nn_d2: the
 * nearest map point (original index) and its float d2 for the points that pass the radius gate; -1 / +inf for flag 0.  normal_map /
 * normal_src: the kept normal of that map point and the point's own kept normal as stored, for every point that passes the radius gate
 * (with their non-finite components).  For flag 1: w = the whitening matrix W = L^-1 row-major (its upper triangle 0), r = the three
 * whitened residuals, row = the three rows [A0..A5, -r_k, r_k]; everything else is 0. */
typedef struct dcreg_glin_debug {
    int32_t *nn_idx;     /* [n] */
    float *nn_d2;        /* [n] */
    uint8_t *flag;       /* [n] */
    double *normal_map;  /* [3*n] */
    double *normal_src;  /* [3*n] */
    double *w;           /* [9*n] */
    double *r;           /* [3*n] */
    double *row;         /* [3*8*n] */
} dcreg_glin_debug;
/* dcreg_linearize_gicp with the dump; searches every point cold and leaves the warm bounds of the plain calls as they were */
int dcreg_linearize_gicp_debug(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *, dcreg_lin_out *,
                               dcreg_glin_debug *);

/* per-point dump of dcreg_linearize_voxels (original source order; any pointer may be NULL).  flag: 1 effective, 0 no kept voxel holds
 * the transformed point, 3 the source point has no normal (mode 1), 5 the covariance is not positive definite.  voxel_idx: the voxel's
 * position in dcreg_target_voxels_get order, -1 for flag 0.  mean / cov: the voxel's record widened to double, for every point with a
 * voxel.  normal_src: the point's own kept normal as stored (with its non-finite components), in mode 1 for every point with a voxel.
 * For flag 1: w = the whitening matrix W = L^-1 row-major (its upper triangle 0), r = the three whitened residuals, row = the three rows
 * [A0..A5, -r_k, r_k] (scaled where a robust kernel is on); everything else is 0.
 * With "voxels_neighbors" = S > 1 every array but normal_src holds S entries per point, one per correspondence in stencil order:
 * correspondence j of point i is entry i*S + j - voxel_idx[n*S], flag[n*S], mean[3*n*S], cov[6*n*S], w[9*n*S], r[3*n*S], row[3*8*n*S] -
 * each with the correspondence's own flag and the meaning above (voxel_idx -1 where the stencil's voxel is not kept or lies outside the
 * map's box).  normal_src stays per point, [3*n]: in mode 1 the normal of every point with at least one correspondence.  The sizes
 * below are those of S = 1; the caller sizes the arrays for the value of the option in force at the call. */
typedef struct dcreg_vlin_debug {
    int32_t *voxel_idx;  /* [n] */
    uint8_t *flag;       /* [n] */
    double *mean;        /* [3*n] */
    double *cov;         /* [6*n] */
    double *normal_src;  /* [3*n] */
    double *w;           /* [9*n] */
    double *r;           /* [3*n] */
    double *row;         /* [3*8*n] */
} dcreg_vlin_debug;
/* dcreg_linearize_voxels with the dump */
int dcreg_linearize_voxels_debug(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *, dcreg_lin_out *,
                                 dcreg_vlin_debug *);

/* total duration (ms, HIP events on the ctx stream around ALL kernels of a linearisation) of the timed linearisations since the
 * last reset, and their number; option "time_kernels" = N > 0 brackets every N-th linearisation of slot 0 (an event pair costs ~10 us
 * of host time), 0 = off */
int dcreg_kernel_time(dcreg_ctx *, double *ms_total, int64_t *launches, int reset);

/* what the linearisations since the last reset did.  points_searched needs the option "count_searches" = 1 (one atomic per searching
 * wave: off by default) and makes this call wait for the launches queued so far; -1 when the option is off. */
typedef struct dcreg_launch_stats {
    int64_t launches;          /* kernel launches (a batched launch counts once) */
    int64_t poses;             /* poses linearised */
    int64_t points;            /* source points those poses had, all told */
    int64_t points_searched;   /* ... of which went through the 6-NN search (the others' certificates held) */
    int64_t points_team;       /* ... of which were searched by a whole wave at a time (search.hpp team_search6: waves with a few
                                  lanes to search), the rest in lock-step; -1 like points_searched */
} dcreg_launch_stats;
int dcreg_launch_stats_get(dcreg_ctx *, dcreg_launch_stats *, int reset);

/* Log of the launches completed since the option "record_launches" = 1 was set (or since the last reset), oldest first: duration
 * (ms, HIP events; -1 for a launch that was not timed - see "time_kernels"), points that went through the 6-NN search (level 1),
 * points whose known neighbours were only re-ordered and refitted (level 2), points the launch linearised in all (poses x source
 * points).  The two counts travel in the count slots of the launch's own result rows (no atomics, no extra transfer); -1 for clouds of
 * more than 2^26 points.  Any array may be NULL; at most `cap` entries are written; returns the number of entries logged (which may
 * exceed cap), < 0 on invalid arguments.  bench.py's per-regime roofline is built from this. */
int dcreg_launch_series(dcreg_ctx *, double *ms, int64_t *searched, int64_t *refitted, int64_t *points, int64_t cap, int reset);
/* ... and, for the same log (call it BEFORE the resetting dcreg_launch_series): 1 where the advance pass (kernels.hpp k_advance: the
 * searches and refits of a launch in dense waves, in front of the linearisation kernel) ran, 2 where its small-frame form did
 * (k_advance_team: sixteen lanes per query), 0 where neither did; the duration and the counts of such a launch cover both kernels.
 * Bit 2 (+ 4): the linearisation kernel ran in one-wave blocks with k_sum_tiles behind it (option "one_wave"; its duration covers
 * both).  Returns the number of entries logged. */
int dcreg_launch_series_passes(dcreg_ctx *, uint8_t *advanced, int64_t cap);
/* ... and which kernels carried each launch of that log out: 0 = the linearisation kernel alone, 1 = a pass and the linearisation kernel
 * behind it, 2 = the advance pass alone (kernels.hpp k_advance ROWS: it builds the rows of its tiles and finishes the launch itself;
 * option "advance_fused").  Bit 2 (+ 4): a five-neighbour launch (option "search_five").  Call it before the resetting
 * dcreg_launch_series too.  Returns the number of entries logged. */
int dcreg_launch_series_structure(dcreg_ctx *, uint8_t *structure, int64_t cap);

/* Timing probe of the small-frame advance pass (option "team_stamps" = 1): of the LAST launch that ran the pass, per block (one wave,
 * kTeamTile points) eight shader-clock words - start, tests done, old neighbours gathered, rows listed, rows cut (table loads), candidates
 * taken, ranked, state written (first round of the block; 0 where a block had nothing to do); one more row of eight outcome counts
 * follows the blocks.  Copies at most cap_blocks x 8 words;
 * returns the number of blocks of that launch.  Waits for the stream. */
int dcreg_team_pass_stamps(dcreg_ctx *, uint64_t *out, int64_t cap_blocks);

/* The window index of a large map (options "roi_index" 0 never / 1 when "max_table_entries" enlarged the whole map's cell edge by more than one step or took its x sub-cells (default) /
 * 2 always, "roi_margin" metres, default 20): single-pose linearisations of such a map search an index over the map's points inside a box
 * around the transformed source - same neighbours, same sums (bitwise), cells sized for the local density instead of the map's extent;
 * everything else (dcreg_knn, dcreg_p2p_error, batches, dumps) runs on the whole map.  info[0..5] = the box (min xyz, max xyz),
 * info[6] = points in the window, info[7] = its cell edge, info[8] = windows built since the context was created, info[9] = 1 while the
 * window is the active index, info[10] = 1 when the whole map's build was cut by the table budget. */
int dcreg_roi_info(const dcreg_ctx *, double info[11]);

/* the analysis as the pipelined engine takes it: the part the step needs first, then what that left owed (*owed: 4 = the axis alignment of the Schur eigenvectors, 1 = the full
 * eigen-decomposition block, 2 = the diagonal blocks of the Schur analysis); the record must equal dcreg_analyze_degeneracy's */
int dcreg_analyze_degeneracy_two_part(const double H[36], int detection, int handling, const dcreg_config *, dcreg_analysis *, int *owed);

/* A kd-tree over the target cloud as a COMPARATOR of the grid index (SURVEY.md 7.1 "benchmark both"): median splits along the widest
 * axis, a complete implicit tree with at most leaf_size points per leaf, built on the host from the cloud of the last dcreg_set_target.
 * dcreg_knn_timed runs the exact k-NN (k = 1 or 5) of dcreg_knn on the grid (index 0: the ring walk of dcreg_knn; index 2: the row
 * sweep the linearisation uses, k = 5 with a radius only) or on the tree (index 1): one untimed launch, then `repeats` launches between
 * two HIP events; all return the same lists, bit for bit.  scripts/kdtree_compare.py. */
int dcreg_kdtree_build(dcreg_ctx *, int leaf_size);
int dcreg_kdtree_info(const dcreg_ctx *, int32_t *depth, int32_t *leaf_size, double *build_ms);
int dcreg_knn_timed(dcreg_ctx *, const float *q_xyz, int64_t n, int64_t stride_floats, int k, double max_radius, int index, int repeats,
                    int32_t *idx, float *d2, double *kernel_ms);

/* test and measurement knobs of dcreg_set_option (defaults are what the product runs with; none changes a result):
 *   "time_kernels"       see dcreg_kernel_time;
 *   "count_searches"     see dcreg_launch_stats;
 *   "record_launches"    see dcreg_launch_series;
 *   "use_certificates"   0 = search every point in every launch (the old neighbours still bound the searches), 1 = default;
 *   "keep_source_order"  1 = the next dcreg_set_source keeps the caller's point order instead of the Hilbert-curve sort;
 *   "advance"            the advance pass in front of single-pose launches: 0 = never, 1 (default) = when the last completed launch searched
 *                        between 0.5 % and 70 % of its points and the cloud has at least "advance_min_blocks" (2048) query blocks, 2 = whenever
 *                        the launch can take it (warm state, certificates in use): tests;
 *   "advance_fused"      1 (default) = a launch that takes the advance pass is ONE kernel: the pass builds the rows of its tiles and finishes
 *                        the launch itself (launches of at most 64 query blocks excepted); 0 = the pass and the linearisation kernel behind
 *                        it, two kernels (A/B and the bitwise comparisons of the tests);
 *   "team_pass"          the small-frame advance pass (sixteen lanes per query) in front of single-pose launches: 0 = never, 1 (default) =
 *                        for clouds of at most 16384 points when the last completed launch searched at least half of them and the map holds
 *                        at least 3 points per occupied cell, 2 = whenever the launch can take it; "team_stamps": see dcreg_team_pass_stamps;
 *   "search_five"        five-neighbour launches (kernels.hpp k_lin FIVE: the searches keep the five nearest and nothing for the next launch -
 *                        no sixth neighbour, no certificate, no stored plane; the next launch on the state searches every point again):
 *                        0 = never, 1 (default) = by the rule - on an engine's trajectory (the first launch of a run announced by
 *                        dcreg_hint_misalignment(-1) and the launches queued behind a gate) while the last completed launch searched at
 *                        least "search_five_frac" (0.95) of its points and the last known step of the pose exceeds "search_five_step"
 *                        (0.04) cell edges -, 2 = every single-pose launch on the context's own state that the fused or the one-wave
 *                        kernel carries out alone (the passes chosen by a rule give way): tests.  Scheduling only: no sum changes;
 *   "one_wave"           the linearisation kernel in one-wave blocks (a tile row per wave, k_sum_tiles behind it): 0 = never, 1 (default) =
 *                        single-pose launches of at least "one_wave_min_blocks" (1024) query blocks most of whose points are expected to
 *                        search ("one_wave_min_frac", 0.5) while the misalignment hint is above "one_wave_min_cells" (1.5) cells - the
 *                        first launches of a run; 2 = every fused launch, small ones included: tests; "one_wave_batches" (1): batched
 *                        launches of one-chunk poses (the Monte-Carlo batches: trials at every stage of their runs side by side) with
 *                        at least "one_wave_min_blocks" query blocks in all run that way too (+ 6 % on the experiment);
 *   "gate_in_kernel"     1 (default) = a pipelined launch of at most 64 query blocks waits for its pose in its first kernel (one kernel boundary
 *                        less); 0 = behind the one-wave gate kernel, like larger launches;
 *   "team_search"        lanes a wave serves one query at a time with all 64 lanes instead of searching in lock-step (0 = never, 7 = default);
 *   "visibility_order"   dcreg_target_remove_dynamic votes over the map's points in cell order (1, default: neighbouring lanes look at
 *                        neighbouring pixels) or in index order (0); the same bits either way;
 *   "curve_x_scale"      next dcreg_set_source: the cells of the source's Hilbert-curve order are 1 / v times as long in x as in y and z
 *                        (v <= 1; default 1 = cubes).
 * Settled and no longer options (rounds 3-5, profiles/r0?_ablation.md): query blocks are dealt to the XCDs in runs of 16;
 * launches of at most 64 query blocks publish their block rows straight to pinned memory; batched launches of one-chunk poses finish inside
 * the kernel; a start bound counts as loose 1.5 cells beyond the nearest occupied cell; the windows of the two advance passes as above. */

/* internal: the device seam of dcreg_register_frames (engine.cpp).  dcreg_frames_load checks, uploads and orders the frames of one call
 * (arguments as there; waits for the stream); dcreg_frames_reserve_states / _reset_state are dcreg_reserve_warm_states / dcreg_reset_warm_state
 * for the frames' own neighbour states (one per slot, sized for the largest frame); dcreg_frames_batch_begin is
 * dcreg_linearize_batch_begin_warm with pose i linearising frame frame_ids[i] (dcreg_linearize_batch_end collects it).  None of them touches
 * the context's own source or states. */
int dcreg_frames_load(dcreg_ctx *, int n_frames, const float *xyz, const int64_t *frame_offsets, int64_t stride_floats);
int dcreg_frames_reserve_states(dcreg_ctx *, int64_t n_states);
int dcreg_frames_reset_state(dcreg_ctx *, int64_t state_id);
int dcreg_frames_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                             const int32_t *frame_ids, const dcreg_lin_params *);

/* internal: the device seam of dcreg_register_frames_normals and dcreg_icp_run_trials_normals (engine.cpp): dcreg_linearize_normals for
 * n_poses poses in ONE launch.  Pose i linearises frame frame_ids[i] of the frames dcreg_frames_load left on the device or, frame_ids ==
 * NULL, the context's own source, against the whole map's index and the kept normals; its 31 sums are bitwise what dcreg_set_source(that
 * cloud) + dcreg_linearize_normals(pose i) return.  dcreg_normals_reserve_slots reserves n_slots warm slots - per point the sorted
 * position of its last nearest neighbour, a bound of the next search and nothing more - sized for the largest loaded frame (frames != 0)
 * or for the own source (frames == 0); state_ids[i] names the slot pose i reads and updates (-1, or state_ids == NULL: search cold, keep
 * nothing), dcreg_normals_reset_slot marks one empty.  A map change, a new source, dcreg_frames_load and an index swap empty all of them;
 * the context's own warm positions (dcreg_linearize_normals) are neither read nor written.  Two launch slots (0, 1) with their own
 * buffers: _begin queues the pose upload and the kernels on the context's stream and returns, _end waits for that slot's results only.
 * While a slot is pending every call that queues work returns DCREG_E_STATE (the list of dcreg_linearize_batch_begin in dcreg.h, and
 * dcreg_linearize_normals, dcreg_target_normals_*, dcreg_frames_load); so does _begin while a launch of the first engine is pending or gated.
 * Refusals as dcreg_linearize_normals (SO(3) only, search_radius finite and > 0, every pose finite: DCREG_E_INVALID; no target, no
 * kept normals, no source / no frames: DCREG_E_STATE), and DCREG_E_INVALID for a frame_id outside the loaded frames or naming an empty
 * frame, a state_id outside the reserved slots or used twice in one launch, slots reserved for the other kind of cloud, a bad slot;
 * DCREG_E_STATE for a slot already pending.  Nothing is queued on a refusal. */
int dcreg_normals_reserve_slots(dcreg_ctx *, int64_t n_slots, int frames);
int dcreg_normals_reset_slot(dcreg_ctx *, int64_t slot_id);
int dcreg_normals_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                              const int32_t *frame_ids, const dcreg_lin_params *);
int dcreg_normals_batch_end(dcreg_ctx *, int slot, dcreg_lin_out *outs);

/* internal: the device seam of dcreg_register_frames_gicp and dcreg_icp_run_trials_gicp (engine.cpp).
 * Kept normals for the frames dcreg_frames_load left on the device, beside their points (float4 {nx, ny, nz, curvature} in every frame's
 * curve order): dcreg_frames_normals_keep estimates them with the given rule for all frames in ONE batched pass (dcreg_normals_clouds'
 * build and kernel over the frames in upload order, then one gather) - frame f's are bitwise what dcreg_source_normals_get returns after
 * dcreg_set_source(frame f) + dcreg_source_normals_keep; infos (may be NULL): one record per frame.  dcreg_frames_normals_set stores the
 * caller's normals as given (n_points = all points of the load, in its upload order, stride_floats >= 3 floats apart; curvature NaN).
 * dcreg_frames_normals_kept: 1 while they are kept.  Every dcreg_frames_load drops them (the loads of dcreg_register_frames* included, and a load refused for its frames with DCREG_E_INVALID too: the frames that were on the device stay, their normals do not; a load refused with DCREG_E_STATE for a linearisation in flight drops nothing);
 * the context's own kept source normals are never touched.  Refusals as the dcreg_source_normals_* calls (DCREG_E_INVALID: null
 * parameters or a parameter out of range, null normals, stride < 3, a point count that is not the load's; DCREG_E_STATE: a linearisation
 * in flight), and DCREG_E_STATE without loaded frames.
 * dcreg_gicp_batch_begin / _end are dcreg_normals_batch_begin / _end for dcreg_linearize_gicp: arguments, refusals, the two launch
 * slots - they ARE the second engine's: a pending slot of either engine refuses the other - and the warm slots of
 * dcreg_normals_reserve_slots (both engines look for the same nearest point; the word bounds the search and decides nothing).  Pose i
 * linearises frame frame_ids[i] with that frame's kept normals or, frame_ids == NULL, the context's own source with its kept source
 * normals; its 31 sums are bitwise what dcreg_set_source(that cloud) + dcreg_source_normals_keep / _set + dcreg_linearize_gicp(pose i)
 * return.  "gicp_epsilon" is read at _begin, and so are "robust_kernel" and "gicp_robust_scale" ("robust_kernel" and "robust_scale" by
 * dcreg_normals_batch_begin and dcreg_pairs_normals_batch_begin): dcreg.h, "robust kernels".  Two more DCREG_E_STATE refusals: no kept frame normals (frame_ids given), no kept source
 * normals (frame_ids == NULL).  dcreg_normal_params_check: the parameter refusals of dcreg_normals on their own (DCREG_OK: none). */
int dcreg_frames_normals_keep(dcreg_ctx *, const dcreg_normal_params *, dcreg_normal_info *infos);
int dcreg_frames_normals_set(dcreg_ctx *, const float *normals, int64_t n_points, int64_t stride_floats);
int dcreg_frames_normals_kept(const dcreg_ctx *);
int dcreg_gicp_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                           const int32_t *frame_ids, const dcreg_lin_params *);
int dcreg_gicp_batch_end(dcreg_ctx *, int slot, dcreg_lin_out *outs);
int dcreg_normal_params_check(dcreg_ctx *, const dcreg_normal_params *);

/* internal: the device seam of dcreg_register_frames_voxels and dcreg_icp_run_trials_voxels (engine.cpp): dcreg_linearize_voxels for
 * n_poses poses in ONE launch (voxel_icp.hip k_vlin_batch).  Pose i linearises frame frame_ids[i] of the frames dcreg_frames_load left on
 * the device - in mode 1 with that frame's kept normals (dcreg_frames_normals_keep / _set) - or, frame_ids == NULL, the context's own
 * source (mode 1: with its kept source normals) against the kept voxel map; its 31 sums are bitwise what dcreg_set_source(that cloud)
 * [+ dcreg_source_normals_keep / _set] + dcreg_linearize_voxels(pose i) return.  There are no state_ids: a voxel launch keeps nothing.
 * It runs in the two launch slots of dcreg_normals_batch_begin - they ARE the second engine's: a pending slot of any of the three
 * engines refuses the others, and every call that dcreg_normals_batch_begin's pending slot refuses (dcreg_set_source*,
 * dcreg_target_voxels_keep / _drop, dcreg_linearize_voxels, dcreg_frames_load, the map updates, ...) is refused meanwhile; _end waits for
 * that slot's results only.  "voxels_source_cov", "voxels_neighbors", "gicp_epsilon", "robust_kernel" and "gicp_robust_scale" are read at _begin.  Of the
 * parameter block only parameterization is read (search_radius is not, as in the single-pose call).  The launch neither reads nor writes
 * warm words, warm slots or neighbour states, the window index (it is neither made active nor deactivated) or the map's kept normals.
 * Refusals, in this order, nothing queued on any: a null context, a bad slot, null R9 / t3 / parameters or n_poses < 1, n_poses > 65535
 * (DCREG_E_INVALID); a gated or pending launch of the first engine, the slot already pending (DCREG_E_STATE); a parameterization other
 * than SO3, a non-finite pose (DCREG_E_INVALID); no target, no kept voxels (DCREG_E_STATE); with frame_ids: no frames loaded
 * (DCREG_E_STATE), an id outside the load or naming an empty frame (DCREG_E_INVALID); without: no source (DCREG_E_STATE); in mode 1 no
 * kept frame normals / no kept source normals (DCREG_E_STATE). */
int dcreg_voxels_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3,
                             const int32_t *frame_ids /* NULL: the context's own source */, const dcreg_lin_params *);
int dcreg_voxels_batch_end(dcreg_ctx *, int slot, dcreg_lin_out *outs);

/* internal: the device seam of dcreg_register_pairs (engine.cpp).  dcreg_pairs_plan cuts the pairs into build batches of their targets
 * (batch b = pairs [batch_end[b - 1], batch_end[b]); option "pairs_max_bytes"); dcreg_pairs_sources_load is dcreg_frames_load for the
 * pairs' sources (kept apart from the context's frames); dcreg_pairs_build indexes the targets of one batch (host memory, offsets from 0,
 * cells for the search radius; waits for the stream); dcreg_pairs_reserve_states / _reset_state are the sources' neighbour states;
 * dcreg_pairs_batch_begin is dcreg_frames_batch_begin with pose i against target target_ids[i] of the batch.  None of them touches the
 * context's own target, source, states, frames or window index. */
int dcreg_pairs_plan(dcreg_ctx *, int n_pairs, const int64_t *tgt_offsets, int64_t stride_floats, int32_t *batch_end, int *n_batches);
int dcreg_pairs_sources_load(dcreg_ctx *, int n_pairs, const float *xyz, const int64_t *src_offsets, int64_t stride_floats);
int dcreg_pairs_build(dcreg_ctx *, int n_targets, const float *xyz, const int64_t *tgt_offsets, int64_t stride_floats, double search_radius);
int dcreg_pairs_reserve_states(dcreg_ctx *, int64_t n_states);
int dcreg_pairs_reset_state(dcreg_ctx *, int64_t state_id);
int dcreg_pairs_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                            const int32_t *source_ids, const int32_t *target_ids, const dcreg_lin_params *);

/* internal: the device seam of dcreg_register_pairs_normals and dcreg_register_pairs_gicp (engine.cpp), on top of the one above.
 * dcreg_pairs_plan_normals is dcreg_pairs_plan with 32 more bytes per target point (a batch's kept normals, 16 B, and the scratch of their
 * estimation).  Kept normals of the build batch dcreg_pairs_build left on the device - float4 {nx, ny, nz, curvature}, target after target,
 * each in its own index order, target t from the batch's offset t: dcreg_pairs_normals_keep estimates them for all targets in ONE launch of
 * the many-clouds normal kernel over the batch's own grids (no second index); target t's are bitwise dcreg_normals of that target alone,
 * and so what dcreg_target_normals_get returns after dcreg_set_target(target t) + dcreg_target_normals_keep; a target with fewer than k
 * points has none (NaN); infos (may be NULL): one record per target, as dcreg_normals fills it.  dcreg_pairs_normals_set stores the caller's
 * normals as given (n_points = all points of the batch in its upload order, stride_floats >= 3 apart; curvature NaN); _get copies them
 * out, 4 floats per point; _kept: 1 while they are kept.  Every dcreg_pairs_build drops them.  dcreg_pairs_sources_normals_keep / _set /
 * _get are dcreg_frames_normals_keep / _set for the sources dcreg_pairs_sources_load left on the device (source p's are bitwise what
 * dcreg_source_normals_get returns after dcreg_set_source(source p) + dcreg_source_normals_keep; _get: upload order, 4 floats per point);
 * every dcreg_pairs_sources_load drops them.  Refusals as the dcreg_frames_normals_* calls; DCREG_E_STATE without a built batch / loaded
 * sources.
 * dcreg_pairs_normals_reserve_slots is dcreg_normals_reserve_slots sized for the largest pair source (slots reserved for the own source
 * or the frames are replaced, and the other way round; dcreg_normals_reset_slot marks one empty).  dcreg_pairs_normals_batch_begin /
 * dcreg_pairs_gicp_batch_begin are dcreg_normals_batch_begin / dcreg_gicp_batch_begin with pose i linearising source source_ids[i] against
 * target target_ids[i] of the batch and that target's kept normals (the GICP form: and the source's kept normals); its 31 sums are bitwise
 * what dcreg_linearize_normals / dcreg_linearize_gicp return on a context with that target, those normals and that source.  A warm slot
 * holds positions in its pose's own target's sorted points: reset it (dcreg_normals_reset_slot) before it serves another pair - a stale
 * word only bounds the search from a valid point or is ignored, it never decides the result.  The state refusals become: no pair batch
 * built, no kept pair normals, no loaded pair sources and - GICP - no kept pair source normals; DCREG_E_INVALID also for a target that is
 * not built (empty) and for a search radius other than the batch's.  Results through dcreg_normals_batch_end. */
int dcreg_pairs_plan_normals(dcreg_ctx *, int n_pairs, const int64_t *tgt_offsets, int64_t stride_floats, int32_t *batch_end, int *n_batches);
int dcreg_pairs_normals_keep(dcreg_ctx *, const dcreg_normal_params *, dcreg_normal_info *infos);
int dcreg_pairs_normals_set(dcreg_ctx *, const float *normals, int64_t n_points, int64_t stride_floats);
int dcreg_pairs_normals_get(dcreg_ctx *, float *out, int64_t capacity_points);
int dcreg_pairs_normals_kept(const dcreg_ctx *);
int dcreg_pairs_sources_normals_keep(dcreg_ctx *, const dcreg_normal_params *, dcreg_normal_info *infos);
int dcreg_pairs_sources_normals_set(dcreg_ctx *, const float *normals, int64_t n_points, int64_t stride_floats);
int dcreg_pairs_sources_normals_get(dcreg_ctx *, float *out, int64_t capacity_points);
int dcreg_pairs_normals_reserve_slots(dcreg_ctx *, int64_t n_slots);
int dcreg_pairs_normals_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                                    const int32_t *source_ids, const int32_t *target_ids, const dcreg_lin_params *);
int dcreg_pairs_gicp_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const int32_t *state_ids,
                                 const int32_t *source_ids, const int32_t *target_ids, const dcreg_lin_params *);

/* internal: the device seam of dcreg_register_pairs_voxels (engine.cpp), beside the two above; the pairs' sources are those of
 * dcreg_pairs_sources_load (mode 1: with dcreg_pairs_sources_normals_keep / _set).
 * dcreg_pairs_plan_voxels is dcreg_pairs_plan with a batch counted at what this form allocates - no cell table: per target point the
 * upload, the packed point, the voxel pass's per-point scratch, the sort's key / value arrays and its temporary storage, and a bound for
 * the per-voxel scratch and the kept members (context.hip pair_voxel_target_bytes has the formula); a batch never exceeds the budget it was
 * planned with, and never splits a pair.
 * dcreg_pairs_voxels_build uploads and packs the targets of one batch (host memory, offsets from 0) and keeps a voxel map for every one
 * of them, all at once (voxel.hip pairs_voxels_build: one upload, one pack, one or two sorts, two scans, one reduction over the voxels of
 * all targets, four synchronises, whatever the number of targets); it builds no grid.  Target t's member is bitwise what
 * dcreg_set_target(target t, any radius) + dcreg_target_voxels_keep(params) keep; infos (may be NULL): one record per target, as
 * dcreg_target_voxels_keep fills it.  A target that keeps no voxel (empty, or every voxel below min_points or degenerate) has no member.
 * DCREG_E_INVALID, the batch a previous build left untouched: the parameter refusals of dcreg_target_voxels_keep, bad offsets, a
 * non-finite coordinate, a voxel coordinate of magnitude 2^62 or more, a target that spans 2^21 or more voxels on an axis; DCREG_E_STATE: a
 * linearisation in flight.  Every build replaces the batch; the index batch of dcreg_pairs_build and the context's own target, kept
 * voxels, source and frames are not touched.  dcreg_pairs_voxels_kept: the kept voxels of one target of the batch (0: no member, or no
 * such target); dcreg_pairs_voxels_get: that member in dcreg_target_voxels_get's order and layout.  dcreg_voxel_map_params_check: the
 * parameter refusals of dcreg_target_voxels_keep on their own; dcreg_pairs_voxels_box_check: what a build refuses of a target with these
 * coordinate-wise float bounds (floor((double)x / leaf) is monotonic in x: a cloud's voxel box is that of its bounds).
 * dcreg_pairs_voxels_batch_begin is dcreg_voxels_batch_begin with pose i linearising pair source source_ids[i] against the member of
 * target target_ids[i] of the batch (voxel_icp.hip k_vlin_pairs); its 31 sums are bitwise what dcreg_linearize_voxels returns on a context
 * with that target's kept voxels and that source (a target without a member: all zero).  No state_ids; the two launch slots are those of
 * dcreg_normals_batch_begin; results through dcreg_voxels_batch_end.  The refusals are dcreg_voxels_batch_begin's in its order, the state
 * refusals being: no pair voxel batch built, no pair sources, in mode 1 no kept pair source normals; DCREG_E_INVALID also for null ids, a
 * source id outside the load or naming an empty source, and a target id outside the batch. */
int dcreg_pairs_plan_voxels(dcreg_ctx *, int n_pairs, const int64_t *tgt_offsets, int64_t stride_floats, int32_t *batch_end, int *n_batches);
int dcreg_pairs_voxels_build(dcreg_ctx *, int n_targets, const float *xyz, const int64_t *tgt_offsets, int64_t stride_floats,
                             const dcreg_voxel_map_params *, dcreg_voxel_map_info *infos /* per target, may be NULL */);
int dcreg_pairs_voxels_get(dcreg_ctx *, int target, int64_t *coords, int32_t *count, float *mean, float *cov, int64_t capacity_voxels);
int dcreg_pairs_voxels_kept(const dcreg_ctx *, int target);
int dcreg_voxel_map_params_check(dcreg_ctx *, const dcreg_voxel_map_params *);
int dcreg_pairs_voxels_box_check(dcreg_ctx *, const float mn[3], const float mx[3], double leaf, int target);
int dcreg_pairs_voxels_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const int32_t *source_ids,
                                   const int32_t *target_ids, const dcreg_lin_params *);

/* Checks the whole map's index after updates (dcreg_target_insert*, dcreg_target_crop): rebuilds the current grid (same origin, cell
 * edge, dims and x sub-cells) from scratch in scratch buffers from the raw points and counts the entries that differ, bitwise:
 * mismatches[0] sorted points (kPtsPad tail included), [1] cell table, [2] row words, [3] gap field, [4] owners.  All zero = the index is
 * exactly what a full build of that grid gives. */
int dcreg_debug_index_check(dcreg_ctx *, int64_t mismatches[5]);

/* The SPFH records behind the last dcreg_fpfh* / dcreg_target_fpfh* call of this context (tests: where the device's atan2 puts a pair
 * at a bin edge of theta, the counts say which pair moved).  36 bytes per input point: the 33 counts, m, 1 when the point has an SPFH,
 * and a zero; all zero for an unused point.  Only directly behind that call: the report reads the points of the index the call searched,
 * which lie in scratch that the next call of the descriptor, normal and outlier families reuses, or in the map.  Once any index of the
 * context has been built since (such a call on a cloud, a dcreg_set_target* / dcreg_set_source* form, a window built by a
 * linearisation), the map has been updated (dcreg_target_insert*, _crop, _remove_*) or its active index has changed, the report is
 * refused with DCREG_E_STATE before anything is queued.  DCREG_E_STATE also without such a call, DCREG_E_INVALID for a null buffer or a
 * capacity below the call's points. */
int dcreg_fpfh_debug_counts(dcreg_ctx *, uint8_t *counts_out, int64_t capacity_points);

/* The same behind the last dcreg_fpfh_radius* / dcreg_target_fpfh_radius* call: 35 uint32 per input point - the 33 counts c_b, the m
 * that the info sums (max_neighbors + 1 for a crowded point, whose counts are 0), 1 when the point has an SPFH; all zero for an unused
 * point.  A call of either rule ends the other's report: DCREG_E_STATE then, without any such call, and for a report whose index has
 * been rebuilt or whose map has changed since, as above; DCREG_E_INVALID as above. */
int dcreg_fpfh_radius_debug_counts(dcreg_ctx *, uint32_t *counts_out, int64_t capacity_points);

/* internal: the host-only translation units above the device seam (engine.cpp) store their error text where dcreg_last_error finds it */
void dcreg_set_error_message(dcreg_ctx *, const char *msg);

#ifdef __cplusplus
}
#endif
#endif /* DCREG_DEBUG_H */
