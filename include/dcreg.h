/*
 * dcreg.h -- C-ABI of the MI355X-native DCReg hot path (libdcreg_hip.so).
 *
 * The reference (JokerJohn/DCReg) has no FFI layer: the point-to-plane ICP inner loop sits behind two
 * C++ seams.  This header is the drop-in boundary a maintainer binds instead:
 *
 *   device seam  (steps 1-5 of one ICP iteration, DCReg/src/icp_test_runner.cpp:1704-1919)
 *       ICPContext::setTargetCloud           DCReg/include/utils.hpp:393-424     -> dcreg_set_target
 *       measure_cloud argument               DCReg/include/icp_test_runner.h:92  -> dcreg_set_source
 *       correspondence + plane fit + A,b + AtA/Atb   icp_test_runner.cpp:1714-1915 -> dcreg_linearize
 *   solver seam  (host, 6x6)
 *       DCReg::analyzeDegeneracy             DCReg/include/dcreg.hpp:45-166      -> dcreg_analyze_degeneracy
 *       DCReg::solveDegenerateSystem         DCReg/include/dcreg.hpp:168-264     -> dcreg_solve_degenerate_system
 *   engine seam
 *       TestRunner::Point2PlaneICP_SO3_OpenMP  icp_test_runner.h:92-102, icp_test_runner.cpp:1611-2060
 *                                                                                 -> dcreg_icp_run
 *       TestRunner::Point2PlaneICP (Euler / LOAM parameterisation)  icp_test_runner.h:72-82, icp_test_runner.cpp:2064-2830
 *                                                                                 -> dcreg_icp_run_euler
 *       TestRunner::runMethod num_runs loop  icp_test_runner.cpp:331-390         -> dcreg_icp_run_trials
 *       calculatePointToPointError           utils.hpp:538-589                   -> dcreg_p2p_error
 *       ICPContext::setTargetCloud's pcl::NormalEstimation (targetNormals)  utils.hpp:393-424
 *                                                                                 -> dcreg_target_normals[_device], dcreg_normals[_device]
 *   plane-to-plane registration (Generalized-ICP; not in the reference)
 *       normals kept beside the map and beside the source                        -> dcreg_target_normals_keep / _set,
 *                                                                                   dcreg_source_normals_keep / _set[_device] / _get[_device] /
 *                                                                                   _kept / _drop
 *       one linearisation, the engine                                            -> dcreg_linearize_gicp, dcreg_icp_run_gicp
 *   registration against per-voxel Gaussians (voxelised GICP / NDT; not in the reference)
 *       one distribution per voxel kept beside the map                           -> dcreg_target_voxels_keep / _get / _kept / _drop
 *       one linearisation, the engine                                            -> dcreg_linearize_voxels, dcreg_icp_run_voxels
 *       many frames / many start poses in one call                               -> dcreg_register_frames_voxels, dcreg_icp_run_trials_voxels
 *   raw clouds (not in the reference, which reads clouds a pcl::VoxelGrid filtered beforehand)
 *       voxel-grid downsampling of many clouds                                   -> dcreg_voxel_downsample[_device]
 *       ... of one cloud, kept as the source / target                            -> dcreg_set_source_voxel[_device],
 *                                                                                   dcreg_set_target_voxel[_device]
 *       statistical / radius outlier removal of one cloud                        -> dcreg_outlier_filter[_device],
 *       ... kept as the source / target, ... of the resident map in place           dcreg_set_source_outliers[_device],
 *                                                                                   dcreg_set_target_outliers[_device],
 *                                                                                   dcreg_target_remove_outliers
 *       motion compensation (deskew) of sweeps from per-point stamps             -> dcreg_deskew[_device],
 *                                                                                   dcreg_set_source_deskew[_device]
 *       ... along a sampled trajectory, through a sensor-to-body extrinsic       -> dcreg_deskew_path[_device],
 *                                                                                   dcreg_set_source_deskew_path[_device]
 *   keyframes (not in the reference: the clouds a mapper has registered, kept on the device by index)
 *       the store                                                                -> dcreg_keyframes_reset / _count / _sizes / _get,
 *                                                                                   dcreg_keyframes_add_clouds[_device], _add_source
 *       submaps assembled from (keyframe id, pose) members                       -> dcreg_keyframes_submaps[_device]
 *       ... as the map: a rebuild after a pose-graph update, a local map         -> dcreg_set_target_keyframes
 *   correspondences for a global alignment (not in the reference: a start pose outside the ICP's basin)
 *       FPFH descriptors of a cloud / of the resident map                        -> dcreg_fpfh[_device], dcreg_target_fpfh[_device]
 *       ... over every point within a radius (PCL setRadiusSearch)               -> dcreg_fpfh_radius[_device], dcreg_target_fpfh_radius[_device]
 *       nearest and second-nearest rows in feature space, mutual flags           -> dcreg_feature_match[_device]
 *       the pose most point pairs agree on (seeded RANSAC), the best T as start poses -> dcreg_align_correspondences[_device]
 *       ... at inlier shares of a per cent: a compatibility graph's consensus sets -> dcreg_consensus_correspondences[_device]
 *       candidate poses scored against the map: inlier count and integer cost, ranked -> dcreg_verify_poses, dcreg_verify_poses_cloud[_device]
 *
 * Conventions: plain pointers and sizes only; the caller owns host buffers (borrowed for the call);
 * a ctx owns its device memory, stream and events; return 0 = ok, <0 = error; a ctx is
 * single-threaded (one per GPU / stream), several may run concurrently.  Results are deterministic
 * (fixed reduction order, no floating-point atomics).  There is NO CPU fallback: without a usable
 * HIP device every device-seam call fails with DCREG_E_DEVICE.
 */
#ifndef DCREG_H
#define DCREG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCREG_OK 0
#define DCREG_E_INVALID (-1)
#define DCREG_E_NOMEM (-2)
#define DCREG_E_DEVICE (-3)
#define DCREG_E_STATE (-4)

/* DetectionMethod / HandlingMethod: numeric values follow DCReg/include/utils.hpp:106-121 */
enum dcreg_detection {
    DCREG_NONE_DETE = 0,
    DCREG_SCHUR_CONDITION_NUMBER = 1,
    DCREG_FULL_EVD_MIN_EIGENVALUE = 2,
    DCREG_EVD_SUB_CONDITION = 3,
    DCREG_FULL_SVD_CONDITION = 4
};
enum dcreg_handling {
    DCREG_NONE_HAND = 0,
    DCREG_STANDARD_REGULARIZATION = 1,
    DCREG_ADAPTIVE_REGULARIZATION = 2,
    DCREG_PRECONDITIONED_CG = 3,
    DCREG_SOLUTION_REMAPPING = 4,
    DCREG_TRUNCATED_SVD = 5
};

typedef struct dcreg_ctx dcreg_ctx;

/* constants of one linearisation; defaults = the literals in icp_test_runner.cpp */
typedef struct dcreg_lin_params {
    double search_radius;          /* Config::search_radius, icp_test_runner.cpp:1725 */
    double max_plane_thickness_sq; /* 0.2*0.2, :1772 */
    double min_normal_norm;        /* 1e-6,    :1750 */
    double weight_slope;           /* 0.9,     :1776 */
    double weight_min;             /* 0.1,     :1785 */
    int use_weight_derivative;     /* USE_WEIGHT_DERIVATIVE, :1691 (0 = released source, 1 = paper) */
    int k;                         /* 5 (only value supported) */
    int parameterization;          /* enum dcreg_parameterization below */
    int reserved_;
    double euler_rpy[3];           /* DCREG_PARAM_EULER / _EULER_EXACT: roll, pitch, yaw of the pose the R passed alongside was built
                                      from (Pose6D2Matrix: R = Rz(yaw) Ry(pitch) Rx(roll), utils.hpp:452-460) */
} dcreg_lin_params;

/* DCREG_PARAM_SO3         right perturbation on SO(3), math_utils.hpp:102-121 (first engine, icp_test_runner.cpp:1863-1907);
 * DCREG_PARAM_EULER       the roll / pitch / yaw row of the second engine AS THE REFERENCE WRITES IT, icp_test_runner.cpp:2299-2346:
 *                         LOAM's three brackets per angle, multiplied by coeff.z, coeff.x, coeff.y (:2323-2335) where LOAM / LIO-SAM
 *                         multiply by coeff.x, coeff.y, coeff.z.  With the reference's order the rotation columns are not the
 *                         derivative of the residual; this value reproduces the reference, term by term;
 * DCREG_PARAM_EULER_EXACT additive, not in the reference: the exact derivative of c . (Rz(yaw) Ry(pitch) Rx(roll) p) by roll /
 *                         pitch / yaw (= LOAM's coefficient order). */
enum dcreg_parameterization { DCREG_PARAM_SO3 = 0, DCREG_PARAM_EULER = 1, DCREG_PARAM_EULER_EXACT = 2 };

typedef struct dcreg_lin_out {
    double H_upper[21]; /* A^T A, row-major upper triangle, order [wx wy wz x y z] (hessian_computer.h:89-94) */
    double g[6];        /* A^T b  (the reference logs gradient = -g, :1918) */
    double sum_r2;      /* sum r^2 over effective points (:1803) -> rmse */
    double sum_b2;      /* sum (float(s r))^2 -> objective = 0.5*sum_b2 (:1919) */
    int64_t n_eff;      /* correspondence_count (:1802) */
    int64_t n_pt;       /* correspondence_pt_count (:1731) -> fitness */
} dcreg_lin_out;

typedef struct dcreg_index_info {
    double cell;        /* grid cell edge (m) */
    double origin[3];
    int32_t dims[3];
    int64_t n_cells;
    int64_t n_target;
    int64_t n_source;
    int32_t max_ring;   /* rings needed to cover search_radius of the last linearisation */
} dcreg_index_info;

/* ---------------- device seam ---------------- */
int dcreg_backend_create(dcreg_ctx **out, int device);
void dcreg_backend_destroy(dcreg_ctx *);
const char *dcreg_last_error(const dcreg_ctx *);
/* use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) - every later call is queued on it and so ordered after
 * what the caller queued there before; NULL = the ctx-owned stream.  torch's DEFAULT stream is the legacy null stream (cuda_stream == 0),
 * so dcreg_set_stream(ctx, torch.cuda.current_stream().cuda_stream) selects the ctx-owned stream there; that stream is non-blocking, and
 * dcreg_set_*_device order themselves after the work queued on the null stream instead (below).  Like every call that queues work,
 * refused (DCREG_E_STATE) while a linearisation is in flight (dcreg_linearize_gated_begin, dcreg_linearize_batch_begin). */
int dcreg_set_stream(dcreg_ctx *, void *hip_stream);
/* options (every one of them but fast_plane_fit changes speed only: results are identical whatever their values)
 *   "warm_start"    1 (default) = keep, per source point, the neighbours its last search found and a certificate of how far the
 *                   point may move before the nearest five can change; later linearisations skip the search of every point whose
 *                   certificate still holds and bound the searches that remain by the old neighbours.  0 = search every point
 *                   from scratch in every call;
 *   "cert_margin"   default 0.05: searches cover search_radius * (1 + margin), so that "the 5th neighbour is beyond the radius" can
 *                   be certified too (takes effect at the next dcreg_set_target: the grid cells follow the search radius);
 *   "cert_inflate"  default 0.005: searches among nearby points look 0.5 % further than they must, which yields the second kind of
 *                   certificate ("the five nearest are among these six"; search.hpp);
 *   "fast_plane_fit" 1 (default) = the reduced-instruction 5x3 plane fit; 0 = the Eigen-shaped factorisation operation for operation,
 *                   as the oracle computes it: its planes, residuals, weights and gate flags are bitwise the oracle's.  The fast fit's
 *                   planes agree with those to a few ulp, so its gate flags can differ from the oracle's for a point whose normal norm,
 *                   plane thickness or weight lies within 1e-11 relative of its threshold (measured on an MI355X for points up to
 *                   50 m out: flips at up to 5e-13 for the thickness gate, 5e-14 for the weight and 6e-17 for the normal norm, none
 *                   at 5e-12 or beyond; tests/test_gpu_gate_edges.py); a flag that differs changes n_eff and everything after it.
 *                   See DESIGN.md;
 *   "spin"          1 (default) = wait for results on the pinned result flags instead of hipStreamSynchronize;
 *   "wait_seconds"  default 30: how long a result is awaited before the stream is drained to look for a device fault;
 *   "dispatch_order" 1 (default) = launches with more query blocks than the device holds at once hand them out heaviest group
 *                   first while dcreg_hint_misalignment says the clouds are misaligned (kernels.hpp k_group_cost); 0 = index order;
 *   "far_bound"     1 (default) = a query whose bound is loose (nothing known yet, or neighbours of a pose far away) starts its
 *                   search from the points around the nearest occupied cell (next dcreg_set_target);
 *   "cell", "cell_factor", "x_subdiv", "gap_field": the grid index (cell edge in metres, 0 = auto = cell_factor x the estimated
 *                   5th-neighbour distance; x sub-cells per cell 1..16, default 8; 1 = build the empty-space distance field) at the
 *                   next dcreg_set_target;
 *   "max_table_entries" default 2^30 (at most 2^31): entries of the dense cell table - one uint32 per x sub-cell of the target's
 *                   bounding box; a map whose cells at the wanted edge would need more gets fewer x sub-cells first and a larger cell
 *                   edge after that (next dcreg_set_target);
 *   "map_update"    1 (default) = dcreg_target_insert* / dcreg_target_crop update the index in the grid it has where they can (new
 *                   points inside its box, density at most twice what the cell edge was sized for), 0 = every update re-derives the grid;
 *   "map_grow_margin" default 20: metres added on each side of the map's box in x and y (not z) when an update re-derives the grid (a
 *                   map that grows along a path re-derives it once per that many metres, not at every keyframe);
 *   "normals_follow" 0 (default) = every update of the map drops the kept normals; 1 = dcreg_target_insert*, dcreg_target_crop,
 *                   dcreg_target_remove_outliers and dcreg_target_remove_dynamic refit the kept normals of dcreg_target_normals_keep
 *                   where the update can have changed them and carry the rest ("kept normals that follow the map" below); read
 *                   at the time of the update;
 *   "normals_follow_full_share" default 0.25 (0 .. 1): the share of the map's points a followed update may have to refit before it
 *                   recomputes all of them instead (the results do not depend on it);
 *   "voxels_follow" 0 (default) = every update of the map drops the kept voxel map; 1 = dcreg_target_insert*, dcreg_target_crop,
 *                   dcreg_target_remove_outliers and dcreg_target_remove_dynamic refit the voxels of dcreg_target_voxels_keep that an added
 *                   or removed point lies in and carry the rest ("kept voxel map that follows the map" below); read at the time of
 *                   the update;
 *   "voxels_follow_full_share" default 0.25 (0 .. 1): the share of the updated map's points lying in touched voxels beyond which a
 *                   followed update runs the full keep instead (the results do not depend on it);
 *   "gicp_epsilon"  default 1e-3 (1e-6 .. 1, DCREG_E_INVALID outside): the small eigenvalue of both plane covariances of
 *                   dcreg_linearize_gicp; read at the time of every linearisation;
 *   "robust_kernel" default 0 = DCREG_ROBUST_NONE; DCREG_ROBUST_HUBER (1), DCREG_ROBUST_CAUCHY (2), DCREG_ROBUST_GEMAN_MCCLURE (3).  The
 *                   robust kernel of dcreg_linearize_normals and dcreg_linearize_gicp and of every form built on them ("robust
 *                   kernels" below); any other value - a non-integer, a value that is not finite - is DCREG_E_INVALID and the old
 *                   value stays.  Read at the time of every linearisation: at the call for a single-pose launch, at *_batch_begin
 *                   for a batched one;
 *   "robust_scale"  default 0.1 (1e-6 .. 1e6, DCREG_E_INVALID outside or not finite, the old value stays): the kernel's scale c for
 *                   dcreg_linearize_normals, in metres; read with "robust_kernel";
 *   "gicp_robust_scale" default 1.0 (same range, same refusal): the kernel's scale c for dcreg_linearize_gicp, in whitened
 *                   (Mahalanobis) units; read with "robust_kernel".  Both defaults are starting values: nobody has tuned them;
 *   "visibility_max_bytes" default 2^28 (256 MiB): device bytes the range images of one batch of members may take in the visibility
 *                   calls (a batch always holds at least one image; the results do not depend on it);
 *   "roi_index", "roi_margin": the WINDOW index of a large map.  A map whose table ran into that budget is searched through cells that
 *                   grow with its extent; dcreg_linearize / the engines' single-pose launches therefore search such a map through a
 *                   second index over the map's points inside a box around the transformed source cloud (its bounding box at the pose +
 *                   the search radius + roi_margin metres, default 20) - the same neighbours and bitwise the same sums, cells sized for
 *                   the local density.  Built by the first linearisation (about 4 ms, whatever the map's size), kept until a
 *                   pose leaves the box, then rebuilt around that pose (a queued gated launch is called off: dcreg_linearize_gate_open
 *                   returns DCREG_E_STATE and the caller starts the launch with dcreg_linearize_batch_begin, as the engines do).
 *                   A gated launch whose search radius needs more of the box than the window was built for runs on the whole map.
 *                   roi_index 1 (default) = for maps whose cell edge the budget enlarged by more than one step (x 1.26) or whose x sub-cells it took, 0 = never, 2 = always.  dcreg_knn,
 *                   dcreg_p2p_error, batched launches and debug dumps always run on the whole map; dcreg_index_info_get describes
 *                   the whole map's index (dcreg_debug.h dcreg_roi_info: the window).
 * Profiling / experiment knobs are listed in dcreg_debug.h. */
int dcreg_set_option(dcreg_ctx *, const char *key, double value);
/* target cloud: copies + builds the device spatial index (stands for kd-tree build, utils.hpp:403).
 * search_radius_hint bounds the cell size (cell <= radius); pass Config::search_radius. */
int dcreg_set_target(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, double search_radius_hint);
/* _device: d_xyz is device memory of the ctx's device (x y z first, stride_floats floats per point, 4-byte aligned), read on the ctx's
 * stream: on a stream given by dcreg_set_stream it is read after the work queued there before the call; on the ctx-owned stream after
 * the work queued on the legacy null stream before the call (an asynchronous event wait: torch's default stream is that stream).  Work
 * the caller queued on any other stream must be finished or waited for by the caller.  Consumed when the call returns, as a host buffer.
 * A refused cloud (null, stride < 3, n <= 0, non-finite coordinates) leaves the ctx's clouds as they were. */
int dcreg_set_target_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, double search_radius_hint);
/* source ("measure") cloud: copies, orders along a space-filling curve.  The caller's buffer is consumed when the call returns - it
 * may be reused or freed at once, whatever kind of host memory it is.  A frame of at most 65536 points (and 2^20 floats) is copied
 * into the context's own pinned block and queued from there without a stream synchronise (the registration path: the first
 * linearisation runs behind the sort): a device fault of the upload or the sort then surfaces at that linearisation, not here.
 * Clouds with non-finite coordinates are refused (DCREG_E_INVALID), source and target alike. */
int dcreg_set_source(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats);
int dcreg_set_source_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats);
int dcreg_default_lin_params(dcreg_lin_params *, double search_radius);
/* one ICP linearisation (steps 1-5): R row-major 3x3, t 3.
 * Every launch at a caller's pose - dcreg_linearize, _batch, _batch_begin[_warm], dcreg_frames_batch_begin, dcreg_pairs_batch_begin,
 * dcreg_linearize_debug, the engines' initial poses - refuses a pose with a NaN or an infinity anywhere in R or t (of any of its n_poses)
 * with DCREG_E_INVALID before anything is queued: warm states, window index and gate stay as they were.  dcreg_linearize_gate_open
 * refuses such a pose the same way and leaves the gate waiting (open it again with a finite pose, or abort it). */
int dcreg_linearize(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *, dcreg_lin_out *);
/* the same for n_poses independent poses of the same cloud pair in ONE launch (Monte-Carlo trials) */
int dcreg_linearize_batch(dcreg_ctx *, int n_poses, const double *R9, const double *t3, const dcreg_lin_params *,
                          dcreg_lin_out *outs);
/* asynchronous pair of the above: _begin queues the copy + kernels on the ctx's stream and returns, _end waits for the
 * results of that slot (pinned-memory sequence numbers) and unpacks them.  While any slot is in flight (or a gated launch waits, below)
 * the calls that queue work, wait for the stream or replace buffers return DCREG_E_STATE at once: dcreg_set_target[_device],
 * dcreg_set_source[_device], dcreg_set_stream, dcreg_knn, dcreg_p2p_error, dcreg_reserve_warm_states, dcreg_reset_warm_state(-1),
 * dcreg_register_frames[_normals], dcreg_icp_run_trials[_normals], dcreg_register_frames_voxels, dcreg_icp_run_trials_voxels, dcreg_register_pairs, dcreg_register_pairs_normals, dcreg_register_pairs_gicp, dcreg_register_pairs_voxels, dcreg_linearize_normals, dcreg_linearize_gicp, dcreg_target_normals_keep / _set / _drop, dcreg_source_normals_keep / _set / _get / _drop,
 * the launches, and dcreg_debug.h's dcreg_frames_load, dcreg_normals_reserve_slots (a pending launch slot of dcreg_normals_batch_begin counts as a slot in flight), dcreg_knn_timed, dcreg_kdtree_build, dcreg_team_pass_stamps and
 * dcreg_launch_stats_get with "count_searches" on; readers of host state (dcreg_index_info_get, dcreg_last_error, ...) stay allowed.  Two slots (0, 1) with their own buffers: keep
 * one batch on the device while the host solves the other (dcreg_icp_run_trials does).  R9 / t3 are copied by _begin. */
int dcreg_linearize_batch_begin(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3, const dcreg_lin_params *);
/* pipelined single-pose launches (what dcreg_icp_run does between two iterations): _gated_begin queues a linearisation on `slot`
 * whose pose is not known yet - a one-wave gate kernel in front of it waits for it - typically while the previous linearisation
 * still runs; _gate_open publishes the pose (two stores, the device starts at once: no launch on the critical path); _gate_abort
 * calls the queued linearisation off (it returns without touching results or warm state).  Exactly one of the two must follow every
 * _gated_begin, before anything else is queued on the context (other launches are refused meanwhile); results come through
 * dcreg_linearize_batch_end(slot).  Needs the default "spin" option (a stream synchronise would wait for the gate).  A gate nobody
 * opens gives up after two minutes. */
int dcreg_linearize_gated_begin(dcreg_ctx *, int slot, const dcreg_lin_params *);
int dcreg_linearize_gate_open(dcreg_ctx *, const double R[9], const double t[3]);
int dcreg_linearize_gate_abort(dcreg_ctx *);
int dcreg_linearize_batch_end(dcreg_ctx *, int slot, dcreg_lin_out *outs);
/* Neighbour states for batched launches.  A single-pose linearisation reuses what its own previous call found (neighbours +
 * certificates, kept inside the ctx); poses of a batch belong to different trajectories, so each needs a state of its own:
 * reserve n_states of them (76 B per source point each; nothing is cleared - a state counts as empty until its first launch
 * has filled it), then name the state of every pose in state_ids (0 <= id < n_states, each id at most once per launch,
 * -1 = search from scratch, keep nothing).  A state is read and updated by the launch, so consecutive launches of one
 * Monte-Carlo trial under the same id skip the searches their certificates cover.  dcreg_reset_warm_state marks one state
 * empty again (a trial slot that takes the next trial); state_id = -1 names the context's OWN state, the one single-pose launches and
 * dcreg_icp_run keep: after it the next launch searches every point from scratch, as the first launch after dcreg_set_source does
 * (the reference builds a fresh ICPContext for every run, icp_test_runner.cpp:408-409: bench.py's `cold_run`).  Results are identical
 * with or without states.
 * dcreg_set_target / dcreg_set_source drop all states. */
/* Scheduling hint, never needed for correctness: how far (metres, roughly) the source points are expected to lie from the map at the
 * poses of the next single-pose linearisations - e.g. the RMS residual of the last iteration.  While it is above half a grid cell
 * (and the context's own cost estimate of the cloud pair is uneven) the query blocks of a launch are handed out heaviest group first
 * instead of in index order (longest processing time first: a launch ends when its slowest block does); while it is above a cell and
 * a half, launches of large clouds most of whose points search run the linearisation kernel in one-wave blocks (kernels.hpp
 * k_lin<.., ONE>: worth a tenth of such a launch, a few microseconds lost on others).  The 31 sums do not depend on it.  Default: +infinity (no knowledge: assume misaligned).  dcreg_icp_run* call it themselves. */
int dcreg_hint_misalignment(dcreg_ctx *, double metres);
int dcreg_reserve_warm_states(dcreg_ctx *, int64_t n_states);
int dcreg_reset_warm_state(dcreg_ctx *, int64_t state_id);
int dcreg_linearize_batch_begin_warm(dcreg_ctx *, int slot, int n_poses, const double *R9, const double *t3,
                                     const int32_t *state_ids, const dcreg_lin_params *);
/* exact k-NN (k = 1 or 5) of host queries against the target index; float sq. distances, (d2, idx) order */
int dcreg_knn(dcreg_ctx *, const float *q_xyz, int64_t n, int64_t stride_floats, int k, double max_radius,
              int32_t *idx, float *d2);
int dcreg_index_info_get(const dcreg_ctx *, dcreg_index_info *);

/* ---------------- updates of the resident map ----------------
 * A mapping front-end grows its map at every keyframe and now and then drops what lies far behind.  These calls do it on the device,
 * without a host copy of the map or a full index build.  For every call that returns DCREG_OK, every later call behaves bitwise as on a
 * context with the same options given dcreg_set_target(M', search_radius_hint of the last dcreg_set_target), M' = the updated cloud in
 * index order (dcreg_target_get) - linearisations, the engines, dcreg_register_frames, dcreg_knn, dcreg_p2p_error, the window index.
 * An update that changes the map drops what dcreg_set_target drops: neighbour states (own, reserved, of loaded frames), the dispatch
 * estimate, the window index and the kd-tree comparator.  info may be NULL.
 * Refusals leave the map, its index and every state as they were: DCREG_E_INVALID (null or negative arguments, stride < 3, non-finite
 * coordinates or pose, more than 2^31 - 1 points in all, a crop that would keep no point), DCREG_E_STATE (no target, no source for
 * _insert_source, a linearisation in flight), DCREG_E_NOMEM (the new arrays are built beside the old ones and swapped in at the end;
 * one exception: on a context whose window index was active, the switch back to the whole map's index has already dropped the neighbour
 * states - results are unaffected).  An insert merged into the current grid whose follow-up re-derivation (density doubled) finds no
 * memory returns DCREG_OK with rebuilt = 0: the merged map is complete and exact, and the next update tries again.
 * Memory: after the first update the context keeps a second sorted array and, after a crop, a second raw array (16 B per map point
 * each); after a re-derivation a second cell table; and field scratch of 10 B per cell of the last change's box grown by two field
 * radii.  They are reused by later updates and freed with the context. */
typedef struct dcreg_map_update {
    int64_t n_offered;   /* points passed in (insert) / map points before the call (crop) */
    int64_t n_added;     /* points appended to the map (insert, after min_spacing) */
    int64_t n_removed;   /* points dropped (crop) */
    int64_t n_target;    /* map points after the call */
    int rebuilt;         /* 0 = merged into the current grid, 1 = grid re-derived */
    int reserved_;
} dcreg_map_update;
/* Point i becomes q_i = R p_i + t (double arithmetic, float store: the transform of the linearisation) and is appended with index
 * n_old + (its rank among the appended points, input order) unless min_spacing > 0 and the map as it stood before the call has a point
 * with float d2 < (float)(min_spacing^2) to it (d2 as dcreg_knn with k = 1 computes it).  New points are not thinned against each
 * other.  An insert that appends nothing changes nothing.  _device: d_xyz as dcreg_set_target_device reads it. */
int dcreg_target_insert(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const double R[9], const double t[3], double min_spacing,
                        dcreg_map_update *info);
int dcreg_target_insert_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const double R[9], const double t[3],
                               double min_spacing, dcreg_map_update *info);
/* the source cloud of the last dcreg_set_source, in its input order (set_source + dcreg_icp_run + insert_source(result): no second upload) */
int dcreg_target_insert_source(dcreg_ctx *, const double R[9], const double t[3], double min_spacing, dcreg_map_update *info);
/* keeps the points with lo[a] <= p[a] <= hi[a] on every axis (float coordinate widened to double), renumbered 0.. in their old order */
int dcreg_target_crop(dcreg_ctx *, const double lo[3], const double hi[3], dcreg_map_update *info);
/* the map in index order, 3 floats per point; DCREG_E_INVALID when capacity_points is below the map's size */
int dcreg_target_get(const dcreg_ctx *, float *xyz_out, int64_t capacity_points);

/* ---------------- voxel-grid downsampling of raw clouds ----------------
 * A raw LiDAR sweep (an organised cloud holds NaN where a beam had no return) or a dense map thinned on the device, with PCL VoxelGrid's
 * semantics (INTEGRATION.md lists where it differs).  For each cloud:
 *   - a point is used only when x, y and z are all finite (the others are dropped and counted);
 *   - its voxel is v_a = floor((double)p_a / leaf[a]) per axis (an IEEE double division);
 *   - voxels are output in ascending (v_z, v_y, v_x) order (x fastest), the points of a voxel taken in ascending input index;
 *   - a voxel with fewer than max(min_points, 1) points is dropped;
 *   - DCREG_VOXEL_CENTROID: the output point is (float)(S_a / count), S_a = the double sum of (double)p_a over the voxel's points, left to
 *     right in input order (S_a = p_0 for one point); DCREG_VOXEL_FIRST: the voxel's lowest-index point, copied bitwise.
 * A voxel's result depends on its own points only (not on other clouds of the call, nor on the launch configuration).  Each cloud is keyed
 * relative to its own minimum voxel.  DCREG_E_INVALID, and nothing is written: a leaf that is not finite and > 0, an unknown mode, offsets
 * that do not start at 0 or decrease, stride < 3, more than 2^31 - 1 points in all, a cloud that spans 2^21 or more voxels on an axis (at a
 * 1 cm leaf 20 km) or has a voxel coordinate of magnitude 2^62 or more; DCREG_E_STATE: a linearisation in flight.  The pass sums every voxel
 * sequentially in one lane: a cloud whose points crowd into a few voxels pays for the longest of them.
 * Device memory: about 120 B per input point of scratch, kept by the context for the next call. */
#define DCREG_VOXEL_CENTROID 0
#define DCREG_VOXEL_FIRST 1
typedef struct dcreg_voxel_params {
    double leaf[3];      /* voxel edge per axis (m) */
    int mode;            /* DCREG_VOXEL_CENTROID / DCREG_VOXEL_FIRST */
    int min_points;      /* PCL setMinimumPointsNumberPerVoxel; <= 1 keeps every voxel */
} dcreg_voxel_params;
typedef struct dcreg_voxel_info {    /* summed over the clouds of the call */
    int64_t n_in;        /* points passed in */
    int64_t n_finite;    /* ... with three finite coordinates */
    int64_t n_voxels;    /* occupied voxels */
    int64_t n_out;       /* ... with at least min_points points: points written */
} dcreg_voxel_info;
/* Many clouds in one call: cloud c = points [offsets[c], offsets[c + 1]) of xyz (n_clouds + 1 offsets, in points, from 0; stride_floats
 * floats per point, x y z first); the output points, 3 floats each, go to out_xyz cloud after cloud, cloud c from out_offsets[c]
 * (n_clouds + 1 entries) - the pair (out_xyz, out_offsets) is what dcreg_register_frames takes with stride 3.  capacity_points = offsets[n_clouds]
 * is always enough; a smaller capacity that the output does not fit returns DCREG_E_INVALID with out_offsets and info filled (the size
 * needed) and nothing written to out_xyz.  offsets, out_offsets and info are host memory; info may be NULL.  Waits for the stream. */
int dcreg_voxel_downsample(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats,
                           const dcreg_voxel_params *, float *out_xyz, int64_t capacity_points, int64_t *out_offsets,
                           dcreg_voxel_info *);
/* _device: d_xyz is read as dcreg_set_source_device reads a cloud; d_out_xyz is device memory, written on the ctx's stream */
int dcreg_voxel_downsample_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                  const dcreg_voxel_params *, float *d_out_xyz, int64_t capacity_points, int64_t *out_offsets,
                                  dcreg_voxel_info *);
/* One cloud voxelised and kept as the source / target: the context is left exactly as dcreg_set_source / dcreg_set_target of the output of
 * dcreg_voxel_downsample leaves it (the output goes from the pass to the source / target build on the device, no host round trip).  A
 * refused call - the refusals of dcreg_voxel_downsample, n <= 0, no point left after the pass - leaves the context's source / target
 * as it was.  info may be NULL.  _device: d_xyz as dcreg_set_source_device / dcreg_set_target_device read it. */
int dcreg_set_source_voxel(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *,
                           dcreg_voxel_info *);
int dcreg_set_source_voxel_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *,
                                  dcreg_voxel_info *);
int dcreg_set_target_voxel(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *,
                           double search_radius_hint, dcreg_voxel_info *);
int dcreg_set_target_voxel_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *,
                                  double search_radius_hint, dcreg_voxel_info *);

/* ---------------- motion compensation (deskew) of raw sweeps from per-point stamps ----------------
 * A spinning LiDAR measures each column of a sweep from a different sensor pose.  These calls move every point into the sensor frame at one
 * reference instant of the sweep, on the device, while the records are packed (no extra pass over memory).  For each point i of cloud c:
 *   - its stamp is stored in its record at float slot `column` of the stride_floats floats, read as raw 32-bit words: DCREG_TIME_F32 a float,
 *     DCREG_TIME_F64 a double over slots column, column + 1 (little-endian, any alignment), DCREG_TIME_U32 an unsigned tick count,
 *     DCREG_TIME_U64 an unsigned tick count over two slots (little-endian); s_i = scale * (double)stamp_i, in seconds;
 *   - the cloud's motion D = (R, t) is the sensor pose at t_end expressed in the frame of the pose at t_begin (R row-major); its twist
 *     xi = Log(D) is computed once per cloud on the host in double (below);
 *   - the span [t_begin, t_end] is the caller's, or with span_from_data the minimum and maximum s_i over the cloud's points whose x, y, z
 *     and s_i are all finite (integer atomics on order-preserving keys: deterministic);
 *   - tau_i = (s_i - t_begin) / (t_end - t_begin) (an IEEE double division), a_i = tau_i - ref; a_i = 0 for a zero-length span;
 *     (R_i, t_i) = Exp(a_i xi), p'_i = (float)(R_i p_i + t_i) in double with p_i = (double) x y z.  This is T(ref)^-1 T(s_i) p_i: the output
 *     is expressed in the sensor frame at the reference instant, and a registration of it estimates the sensor pose at that instant;
 *   - Exp(w, v), theta = |w|: R = I + A [w]x + B [w]x^2, V = I + B [w]x + C [w]x^2, t = V v with A = sin(theta)/theta, B = (1 - cos(theta))/theta^2,
 *     C = (theta - sin(theta))/theta^3, and for theta < 1e-3 their series through theta^4 (A = 1 - theta^2/6 + theta^4/120, B = 1/2 - theta^2/24
 *     + theta^4/720, C = 1/6 - theta^2/120 + theta^4/5040); Log is its inverse (angle-axis of R, then v = V^-1 t);
 *   - where every component of a_i xi is exactly zero (a zero-length span, an identity motion, a stamp at the reference instant) the point
 *     is copied bit for bit (-0.0 stays -0.0);
 *   - a point whose x, y, z or s_i is not finite comes out as three NaN (it is not counted in n_finite); a finite s_i outside the span is
 *     extrapolated and counted in n_outside (a span taken from the data has no such point; a zero-length span copies them).
 * A point's result depends on its own record and its cloud's motion only (not on other clouds of the call, nor on the launch configuration).
 * DCREG_E_INVALID, and nothing is written: t_end < t_begin, a non-finite span or ref, ref outside [0, 1]; a non-finite R or t, an R that is
 * not a rotation (an element of |R^T R - I| above 1e-6, or det(R) <= 0) or rotates by pi/2 or more; a column outside [3, stride_floats)
 * (column + 1 < stride_floats too for the 64-bit types); an unknown type; a scale that is not finite and > 0; null field or motions; and the
 * voxel pass's own refusals when a voxel block is given.  DCREG_E_STATE: a linearisation in flight. */
#define DCREG_TIME_F32 0
#define DCREG_TIME_F64 1
#define DCREG_TIME_U32 2
#define DCREG_TIME_U64 3
typedef struct dcreg_time_field {
    int column;          /* float slot of the stamp in each record (>= 3: x y z come first) */
    int type;            /* DCREG_TIME_F32 / _F64 / _U32 / _U64 */
    double scale;        /* seconds per stamp unit (1 for seconds, 1e-9 for nanosecond ticks) */
} dcreg_time_field;
typedef struct dcreg_sweep_motion {
    double R[9], t[3];   /* sensor pose at t_end in the frame of the pose at t_begin */
    double t_begin, t_end;   /* span in seconds (ignored with span_from_data) */
    double ref;          /* reference instant in [0, 1] of the span: 0 start, 0.5 middle, 1 end */
    int span_from_data;  /* 1: the span is the minimum / maximum finite stamp of the cloud */
    int reserved_;
} dcreg_sweep_motion;
typedef struct dcreg_deskew_info {   /* over the clouds of the call */
    int64_t n_in;        /* points passed in */
    int64_t n_finite;    /* ... with finite x, y, z and stamp */
    int64_t n_outside;   /* ... of those, stamps outside their cloud's span (extrapolated) */
    double t_min, t_max; /* smallest / largest s_i of those (NaN when there is none) */
} dcreg_deskew_info;
/* Many clouds (offsets as dcreg_voxel_downsample), one motion per cloud.  voxel == NULL: every point comes out, in input order, 3 floats each,
 * and out_offsets = offsets (an organised sweep stays organised; capacity_points must hold offsets[n_clouds]).  voxel != NULL: the output is
 * bitwise dcreg_voxel_downsample of the deskewed clouds (what dcreg_register_frames takes with stride 3), capacity as there.  info and
 * vinfo may be NULL.  Waits for the stream.  _device: d_xyz read as dcreg_voxel_downsample_device reads it, d_out_xyz device memory. */
int dcreg_deskew(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_time_field *,
                 const dcreg_sweep_motion *motions, const dcreg_voxel_params *voxel, float *out_xyz, int64_t capacity_points,
                 int64_t *out_offsets, dcreg_deskew_info *info, dcreg_voxel_info *vinfo);
int dcreg_deskew_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_time_field *,
                        const dcreg_sweep_motion *motions, const dcreg_voxel_params *voxel, float *d_out_xyz, int64_t capacity_points,
                        int64_t *out_offsets, dcreg_deskew_info *info, dcreg_voxel_info *vinfo);
/* One sweep deskewed and kept as the source: the context is left bitwise as dcreg_set_source (voxel == NULL: a point that comes out
 * non-finite refuses the call, as there) or dcreg_set_source_voxel (voxel != NULL) of the dcreg_deskew output leaves it.  A refused call
 * leaves the source as it was.  _device: d_xyz as dcreg_set_source_device reads it. */
int dcreg_set_source_deskew(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_time_field *,
                            const dcreg_sweep_motion *, const dcreg_voxel_params *voxel, dcreg_deskew_info *info, dcreg_voxel_info *vinfo);
int dcreg_set_source_deskew_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_time_field *,
                                   const dcreg_sweep_motion *, const dcreg_voxel_params *voxel, dcreg_deskew_info *info,
                                   dcreg_voxel_info *vinfo);

/* ---------------- deskew along a sampled trajectory, through a sensor-to-body extrinsic ----------------
 * The same calls in the same place (inside the pack), for callers that have an odometry or IMU-propagated pose many times per sweep instead of
 * one twist.  A call carries one knot table and one path block per cloud:
 *   - knot table: n_knots instants knot_stamps[j] (seconds) and poses knot_poses[12 j ..] = R[9] row-major then t[3], the pose of the BODY
 *     in any fixed frame at that instant;
 *   - the path block of cloud c names its window [first_knot, first_knot + n_knots) of the table (K = n_knots >= 2 knots with stamps s[0..K-1]
 *     and poses P[0..K-1]; windows of different clouds may overlap or coincide: one trajectory for a whole drive, or one table per cloud),
 *     the reference instant t_ref (seconds, absolute) and the extrinsic E = (ext_R, ext_t), the pose of the SENSOR in the body frame
 *     (identity: the knots are the sensor's own poses);
 *   - the time field is decoded exactly as above: s_i = scale * (double)stamp_i;
 *   - segment twists, on the host in double: xi_k = Log(P_k^-1 P_k+1), k = 0..K-2 (P_k^-1 P_k+1 = (R_k^T R_k+1, R_k^T (t_k+1 - t_k)));
 *   - the segment of an instant s: k(s) = the number of j in [1, K-2] with s[j] <= s (an instant on a knot belongs to the segment that
 *     starts there, the last knot to the last segment); u(s) = (s - s[k]) / (s[k+1] - s[k]) (an IEEE double division);
 *     B(s) = P_k Exp(u xi_k), Exp as above;
 *   - an instant before s[0] or after s[K-1] is extrapolated along the first / last segment (u < 0, u > 1) and counted in n_outside;
 *   - p'_i = (float)(E^-1 B(t_ref)^-1 B(s_i) E p_i), evaluated in double as q = E p_i, q = Exp(u_i xi_k) q, p'_i = G_k q with
 *     G_k = E^-1 B(t_ref)^-1 P_k computed once per (cloud, segment) on the host in double, translations taken relative to the knot that
 *     starts t_ref's segment (knots kilometres from the origin cost no precision).  The output is the sweep in the SENSOR frame at t_ref:
 *     a registration of it estimates the sensor pose B(t_ref) E at that instant (the body pose is that times E^-1);
 *   - a point whose x, y, z or s_i is not finite comes out as three NaN (it is not counted in n_finite).  dcreg_deskew_info is the one
 *     above; n_outside counts the finite stamps outside [s[0], s[K-1]] of their cloud's window;
 *   - there is no bit-for-bit clause here: a path that stands still returns the points to within rounding (G_k of equal poses is the
 *     identity up to rounding only), not their bits.
 * A point's result depends on its own record, its cloud's path block and that block's knot window only.
 * DCREG_E_INVALID, and nothing is written: a null table or null blocks with clouds present; a window outside the table or with fewer than 2
 * knots; stamps of a window that are not finite and strictly increasing; a knot pose or extrinsic that is not finite or not a rotation (as
 * above); a segment that rotates by pi/2 or more; a t_ref that is not finite or lies outside [s[0], s[K-1]]; the time field's refusals and,
 * with a voxel block, the voxel pass's.  Only knots inside some cloud's window are checked.  DCREG_E_STATE: a linearisation in flight. */
typedef struct dcreg_sweep_path {
    int64_t first_knot;  /* the cloud's window of the knot table: [first_knot, first_knot + n_knots) */
    int n_knots;         /* >= 2 */
    int reserved_;
    double t_ref;        /* reference instant in seconds, inside [s[0], s[n_knots - 1]] of the window */
    double ext_R[9], ext_t[3];   /* pose of the sensor in the body frame (R row-major) */
} dcreg_sweep_path;
/* The four forms of the constant-twist deskew with (n_knots, knot_stamps, knot_poses, paths) in place of motions: the table and the blocks
 * (one per cloud) are host memory in all four; voxel block, output layout, capacity, info / vinfo, stream and in-flight behaviour are those
 * of dcreg_deskew* / dcreg_set_source_deskew*. */
int dcreg_deskew_path(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_time_field *,
                      int64_t n_knots, const double *knot_stamps, const double *knot_poses, const dcreg_sweep_path *paths,
                      const dcreg_voxel_params *voxel, float *out_xyz, int64_t capacity_points, int64_t *out_offsets, dcreg_deskew_info *info,
                      dcreg_voxel_info *vinfo);
int dcreg_deskew_path_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                             const dcreg_time_field *, int64_t n_knots, const double *knot_stamps, const double *knot_poses,
                             const dcreg_sweep_path *paths, const dcreg_voxel_params *voxel, float *d_out_xyz, int64_t capacity_points,
                             int64_t *out_offsets, dcreg_deskew_info *info, dcreg_voxel_info *vinfo);
int dcreg_set_source_deskew_path(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_time_field *, int64_t n_knots,
                                 const double *knot_stamps, const double *knot_poses, const dcreg_sweep_path *path,
                                 const dcreg_voxel_params *voxel, dcreg_deskew_info *info, dcreg_voxel_info *vinfo);
int dcreg_set_source_deskew_path_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_time_field *,
                                        int64_t n_knots, const double *knot_stamps, const double *knot_poses, const dcreg_sweep_path *path,
                                        const dcreg_voxel_params *voxel, dcreg_deskew_info *info, dcreg_voxel_info *vinfo);

/* ---------------- place recognition: Scan Context descriptors, a database of them, exhaustive search ----------------
 * dcreg_register_frames and dcreg_register_pairs verify loop-closure and relocalisation candidates; these calls produce them.  A sweep gets a
 * Scan Context descriptor (Kim & Kim, IROS 2018: the maximum height per polar bin) on the device, descriptors are kept in a database that
 * lives in the context, and a query is compared with every entry of an index range at every column shift.
 * Descriptor of one cloud: n_rings x n_sectors floats, ring-major (d[ring * n_sectors + sector]).
 *   - a point is used when x, y and z are finite and min_range^2 <= rho2 < max_range^2 with rho2 = x^2 + y^2 in double (the squares are
 *     exact: one rounding);
 *   - ring coordinate a = sqrt(rho2) * n_rings / max_range, ring = min(floor(a), n_rings - 1);
 *   - theta = atan2(y, x), plus 2 pi when negative; sector coordinate b = theta * n_sectors / (2 pi), sector = min(floor(b), n_sectors - 1);
 *   - a bin's value is the maximum over its points of (float)((double)z + z_offset); an empty bin holds 0;
 *   - the formulas are evaluated in double as they are written, one rounding per operation, left to right: (sqrt(rho2) * n_rings) /
 *     max_range and (theta * n_sectors) / 6.283185307179586, with that same double for the 2 pi of the sum.  A point on an edge falls in
 *     the bin this evaluation gives, which need not be the mathematical one: with 60 sectors (0, 4) has b = 14.999999999999998 and
 *     lies in sector 14, not 15; (4, -1e-30) has theta + 2 pi == 2 pi and the last sector only through the clamp.  rho2 == min_range^2
 *     is used, rho2 == max_range^2 is not; -0.0 is not negative, so theta = -0.0 (y = -0.0, x > 0) lies in sector 0;
 *   - this fixes the bin wherever theta is fixed: on the axes, where atan2 is +-0, +-pi/2 or +-pi rounded to double (C Annex F, the
 *     origin included: theta = 0 for x = +0, pi for x = -0); on the diagonals |x| == |y|, where it is +-pi/4 or +-3 pi/4 rounded to
 *     double; and beside the +x axis, where |theta| is so small that 2 pi absorbs it.  sqrt is correctly rounded, so the ring of
 *     every point is fixed (rho2 a perfect square reaches a ring edge exactly);
 *   - elsewhere a point whose b lies within 1e-9 of an integer may fall in either neighbouring sector (atan2 differs between libraries
 *     in its last bits); every other point falls in the bin the formulas give.
 * The maximum is taken with integer atomics on order-preserving keys, so a descriptor does not depend on the order of the points, on the
 * launch configuration, or on the other clouds of the call.
 * Distance of a query descriptor q and an entry c at shift n in [0, n_sectors), everything in double: over the columns j for which both
 * q's column j and c's column (j + n) mod n_sectors have a non-zero norm (m of them), D_n = (1/m) sum_j (1 - q_j . c_(j+n) / (|q_j| |c_(j+n)|));
 * D_n = 1 when m = 0.  The distance of the pair is min_n D_n and its shift the smallest n that attains it.  The sums run in a fixed
 * order: results are bitwise repeatable.
 * Geometry: a query taken at the entry's position with its sensor frame yawed by +psi has its best shift at psi * n_sectors / (2 pi).  The
 * start pose for registering the query (source) against the entry's cloud (target) is therefore R0 = Rz(2 pi * shift / n_sectors), t0 = 0,
 * good to half a sector: what dcreg_register_pairs takes.
 * Search: for each query the k entries (k in [1, 64]) of the index range [first, last) with the smallest distance, ordered by (distance,
 * index): idx[q k + s] (int32), shift[q k + s] (int32), dist[q k + s] (double).  Slots beyond the range's size hold index -1, shift 0 and
 * distance +inf.  The range is how a mapping loop leaves out its most recent keyframes.  The result for a (query, entry) pair depends on
 * those two descriptors only: not on the number of queries, the range, k, or the database's size.  There is no ring-key or tree
 * prefilter: every entry of the range is compared (DESIGN.md says why).
 * The database is created by dcreg_places_reset, which fixes its parameters, and freed by dcreg_backend_destroy.  It needs no target, and
 * it is not dropped by dcreg_set_target, dcreg_set_source, the map updates or the registration calls: a map and its places live side by
 * side.  None of these calls changes the target, the source, neighbour states, loaded frames or the window index.
 * DCREG_E_INVALID: n_rings outside [1, 64], n_sectors outside [1, 128], a max_range that is not finite and > 0, a min_range that is not
 * finite, is below 0 or is not below max_range, a z_offset that is not finite; the cloud refusals of dcreg_voxel_downsample (offsets,
 * stride, 2^31 - 1 points); first > last or a range outside [0, count]; k outside [1, 64]; a host descriptor with a value that is not
 * finite; null buffers.  DCREG_E_STATE: a linearisation in flight; add, get or query before dcreg_places_reset; a _source form without a
 * source.  A refused call and a failed allocation (DCREG_E_NOMEM) leave the database as it was.  All calls wait for the stream.
 * Device memory: 4 B per bin and 8 B per column of every entry, and scratch of 12 B per (query, entry) pair of a query batch (at most 2^24
 * pairs at once). */
typedef struct dcreg_place_params {
    int n_rings;         /* radial bins, 1 .. 64 */
    int n_sectors;       /* azimuthal bins, 1 .. 128 */
    double max_range;    /* points at this horizontal distance or beyond are not used (m) */
    double min_range;    /* points nearer than this are not used (m) */
    double z_offset;     /* added to z: heights must come out positive for an occupied bin to differ from an empty one (the sensor height) */
} dcreg_place_params;
typedef struct dcreg_place_info {    /* summed over the clouds of the call */
    int64_t n_in;        /* points passed in */
    int64_t n_finite;    /* ... with three finite coordinates */
    int64_t n_used;      /* ... of those, inside the range gate */
} dcreg_place_info;
/* 20 rings, 60 sectors, max_range 80, min_range 0, z_offset 2 */
int dcreg_default_place_params(dcreg_place_params *);
/* The descriptors of many clouds (offsets as dcreg_voxel_downsample) to desc_out[n_clouds * n_rings * n_sectors], host memory; the database is
 * not touched and need not exist.  info may be NULL.  _device: d_xyz as dcreg_voxel_downsample_device reads it, d_desc_out device memory. */
int dcreg_place_descriptors(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, const dcreg_place_params *,
                            float *desc_out, dcreg_place_info *info);
int dcreg_place_descriptors_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                   const dcreg_place_params *, float *d_desc_out, dcreg_place_info *info);
/* empties the database and fixes its parameters */
int dcreg_places_reset(dcreg_ctx *, const dcreg_place_params *);
/* entries in the database (0 before dcreg_places_reset) */
int64_t dcreg_places_count(const dcreg_ctx *);
/* appends n host descriptors (what dcreg_places_get or dcreg_place_descriptors returned); they receive the indices count, count + 1, .. */
int dcreg_places_add(dcreg_ctx *, int64_t n, const float *desc);
/* computes the descriptors of the call's clouds with the database's parameters and appends them on the device (no host round trip) */
int dcreg_places_add_clouds(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, dcreg_place_info *info);
int dcreg_places_add_clouds_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                   dcreg_place_info *info);
/* ... of the context's current source, in its input order (the copy dcreg_target_insert_source reads) */
int dcreg_places_add_source(dcreg_ctx *, dcreg_place_info *info);
/* entries [first, first + n) to desc_out (host): persistence for a caller */
int dcreg_places_get(dcreg_ctx *, int64_t first, int64_t n, float *desc_out);
/* n_queries host descriptors against the entries [first, last): idx, shift and dist hold n_queries * k results each (host memory) */
int dcreg_places_query(dcreg_ctx *, int n_queries, const float *desc, int64_t first, int64_t last, int k, int32_t *idx, int32_t *shift,
                       double *dist);
/* ... with the descriptors of the call's clouds (one query per cloud), computed with the database's parameters; info may be NULL */
int dcreg_places_query_clouds(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, int64_t first,
                              int64_t last, int k, int32_t *idx, int32_t *shift, double *dist, dcreg_place_info *info);
int dcreg_places_query_clouds_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats, int64_t first,
                                     int64_t last, int k, int32_t *idx, int32_t *shift, double *dist, dcreg_place_info *info);
/* ... with the descriptor of the context's current source (one query) */
int dcreg_places_query_source(dcreg_ctx *, int64_t first, int64_t last, int k, int32_t *idx, int32_t *shift, double *dist, dcreg_place_info *info);

/* ---------------- outlier removal: statistical and radius filters ----------------
 * PCL's StatisticalOutlierRemoval and RadiusOutlierRemoval on the device, with rules fixed tightly enough that the output is bitwise the
 * numpy reference of tests/outliers_ref.py (INTEGRATION.md lists where the statistical filter differs from PCL's).  For one cloud of n
 * points and the parameters mode, k, std_mul, radius, min_neighbors, search_radius:
 *   - used points: a point is used when x, y and z are all finite; the others are dropped and counted.  "Index" is the input index;
 *   - distances between used points are the float d2 that dcreg_knn computes; neighbours are ranked by the total order (d2, index);
 *   - a point is never its own neighbour, by index and not by distance: exact duplicates are neighbours at distance 0.  (With more than k
 *     duplicates of a point that point is not among its own k + 1 nearest, so "search k + 1 and drop the first" is wrong: the entry with
 *     the point's own index is dropped if it is there, otherwise the last.  The k distances that remain are the k smallest d2 to OTHER
 *     points either way, which is what the device keeps.)
 *   DCREG_OUTLIER_STATISTICAL (k in [1, 32], std_mul finite, search_radius finite and >= 0):
 *   - score m_i = (float)((sum_{j=1..k} (double)sqrtf(d2_ij)) / k), summed left to right over the k nearest others in ascending rank, with
 *     an IEEE float square root and an IEEE double division;
 *   - search_radius > 0: only neighbours with d2 < (float)(search_radius^2) count; a used point with fewer than k of them is SPARSE: it
 *     is dropped, counted in n_sparse, and takes no part in the statistics;
 *   - search_radius = 0: the search is unbounded.  A cloud with at most k used points has no statistics: all its used points are kept,
 *     every score is NaN, and mean, stddev and threshold are NaN;
 *   - tree sum T(a) of a length-n array: pad with +0.0 to the next power of two, replace the array by a[2j] + a[2j+1] until one value is
 *     left (numpy: while len(b) > 1: b = b[0::2] + b[1::2]).  Any reduction whose blocks are power-of-two sized and aligned reproduces
 *     this tree: the result does not depend on the launch configuration;
 *   - statistics over the n_stat points that are used and not sparse, every other position of the n contributing +0.0:
 *     mean = T((double)m_i) / n_stat; var = T(((double)m_i - mean)^2) / (n_stat - 1), or 0 for n_stat = 1; stddev = sqrt(var);
 *     threshold = mean + std_mul * stddev as one rounded multiply and one rounded add (no fused multiply-add).  n_stat = 0: all three NaN;
 *   - point i is kept iff (double)m_i <= threshold.
 *   DCREG_OUTLIER_RADIUS (radius finite and > 0, min_neighbors >= 1):
 *   - a used point is kept iff at least min_neighbors other used points have d2 < (float)(radius^2) - the comparison min_spacing uses in
 *     dcreg_target_insert.  No statistics (mean, stddev, threshold: NaN; n_sparse: 0), no order dependence; the count stops at min_neighbors.
 *   Output: the kept points in input order, each copied bit for bit, 3 floats per point; optionally (NULL: not wanted) a keep mask
 *   uint8[n] and the scores float[n] - statistical mode m_i, radius mode the neighbour count capped at min_neighbors as a float, NaN for
 *   unused and sparse points.
 * A call's result depends on the cloud and the parameters only - not on what else the context holds - and repeated calls are bitwise equal.
 * None of the filter calls changes the target, the source, neighbour states, loaded frames, the places database or the window index;
 * dcreg_set_source_outliers / dcreg_set_target_outliers change what dcreg_set_source / dcreg_set_target change, and
 * dcreg_target_remove_outliers what dcreg_target_crop changes.
 * An unbounded search of an isolated point walks the rings of the grid out to its k-th neighbour: a hundred points tens of metres from a
 * 1 M-point cloud take the call from 4 ms to a second; search_radius is the practical answer for clouds with far outliers.
 * DCREG_E_INVALID, and nothing is written: null parameters, an unknown mode, k outside [1, 32], a std_mul that is not finite, a
 * search_radius that is not finite or is negative, a radius that is not finite and > 0, min_neighbors < 1, stride < 3, n < 0, more than
 * 2^31 - 1 points, null buffers; DCREG_E_STATE: a linearisation in flight.  A failed allocation (DCREG_E_NOMEM) leaves the context as it
 * was.  Device memory: about 60 B per input point of scratch plus the index of the cloud, kept by the context for the next call. */
#define DCREG_OUTLIER_STATISTICAL 0
#define DCREG_OUTLIER_RADIUS 1
typedef struct dcreg_outlier_params {
    int mode;            /* DCREG_OUTLIER_STATISTICAL / DCREG_OUTLIER_RADIUS */
    int k;               /* statistical: neighbours per point (PCL setMeanK), 1 .. 32 */
    double std_mul;      /* statistical: PCL setStddevMulThresh */
    double search_radius;/* statistical: 0 = unbounded, > 0 = neighbours beyond it do not count (m) */
    double radius;       /* radius mode: PCL setRadiusSearch (m) */
    int min_neighbors;   /* radius mode: PCL setMinNeighborsInRadius, >= 1 */
    int reserved_;
} dcreg_outlier_params;
typedef struct dcreg_outlier_info {
    int64_t n_in;        /* points passed in (after the voxel block, where one runs first) */
    int64_t n_finite;    /* ... with three finite coordinates (used) */
    int64_t n_sparse;    /* ... of those, with fewer than k neighbours inside search_radius */
    int64_t n_out;       /* points kept */
    double mean, stddev, threshold;   /* statistical mode (NaN otherwise) */
} dcreg_outlier_info;
/* statistical, k = 8, std_mul = 2, search_radius = 0; radius = 0.5, min_neighbors = 3 */
int dcreg_default_outlier_params(dcreg_outlier_params *);
/* One cloud in (stride_floats floats per point, x y z first), the kept points out.  *n_out receives the number of kept points;
 * capacity_points = n is always enough; a smaller capacity that the output does not fit returns DCREG_E_INVALID with *n_out and info filled
 * (the size needed) and nothing written to out_xyz, keep_mask or scores.  info may be NULL.  Waits for the stream.
 * _device: d_xyz is read as dcreg_set_source_device reads a cloud; d_out_xyz, d_keep_mask and d_scores are device memory. */
int dcreg_outlier_filter(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_outlier_params *, float *out_xyz,
                         int64_t capacity_points, int64_t *n_out, uint8_t *keep_mask, float *scores, dcreg_outlier_info *info);
int dcreg_outlier_filter_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_outlier_params *,
                                float *d_out_xyz, int64_t capacity_points, int64_t *n_out, uint8_t *d_keep_mask, float *d_scores,
                                dcreg_outlier_info *info);
/* One cloud filtered and kept as the source / target; voxel != NULL runs the voxel pass first (voxel -> filter -> build), as the deskew
 * forms take a voxel block.  The context is left bitwise as dcreg_set_source / dcreg_set_target of the filtered cloud leaves it (the points
 * go from pass to build on the device).  A refused call - the filter's refusals, the voxel pass's, n <= 0, no point left - leaves the
 * context's source / target as it was.  vinfo and info may be NULL. */
int dcreg_set_source_outliers(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *voxel,
                              const dcreg_outlier_params *, dcreg_voxel_info *vinfo, dcreg_outlier_info *info);
int dcreg_set_source_outliers_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *voxel,
                                     const dcreg_outlier_params *, dcreg_voxel_info *vinfo, dcreg_outlier_info *info);
int dcreg_set_target_outliers(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *voxel,
                              const dcreg_outlier_params *, double search_radius_hint, dcreg_voxel_info *vinfo, dcreg_outlier_info *info);
int dcreg_set_target_outliers_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_voxel_params *voxel,
                                     const dcreg_outlier_params *, double search_radius_hint, dcreg_voxel_info *vinfo,
                                     dcreg_outlier_info *info);
/* Cleans the resident map in place: the filter over the map's points in index order, searched through the map's own index (on a map with
 * a window index the whole map's, as dcreg_knn), the survivors through the update path of dcreg_target_crop.  It carries the contract of
 * the map-update section above: later calls are bitwise dcreg_set_target of the cleaned cloud in index order; a call that changes the map
 * drops what dcreg_set_target drops; a call that removes nothing changes nothing (the neighbour states stay warm); a call that would
 * remove every point is refused (DCREG_E_INVALID); refusals leave everything as it was.  DCREG_E_STATE: no target. */
int dcreg_target_remove_outliers(dcreg_ctx *, const dcreg_outlier_params *, dcreg_outlier_info *info);

/* ---------------- keyframe store: submaps and map rebuilds from poses ----------------
 * The clouds a mapper registers are kept on the device by index, beside the map and the place database (which holds their descriptors: a
 * caller that adds keyframe and place in lockstep - dcreg_places_add_source, dcreg_keyframes_add_source - has one index for both).  A
 * SUBMAP is an ordered list of (keyframe id, pose) members: each member's points are moved by its pose on the device, the submap's points
 * are the concatenation of its members, optionally through the voxel pass.  Poses are arguments of every assembling call and are never
 * stored - the caller owns the pose graph, and its poses change.  Every output is bitwise the numpy reference of tests/keyframes_ref.py.
 *
 * Store.  A keyframe is a cloud of n >= 0 points, 3 floats each, stored bit for bit in input order.  Ids are 0, 1, 2, ... in the order
 * added; the clouds of one dcreg_keyframes_add_clouds call get consecutive ids from *first_id.  The store needs no target; it is not
 * dropped or changed by dcreg_set_target*, dcreg_set_source*, the map updates, the registration calls, the places calls or the filter
 * calls.  It is emptied only by dcreg_keyframes_reset and freed with the context; single keyframes cannot be removed (as for places).
 *
 * Add.  dcreg_keyframes_add_clouds takes clouds as dcreg_voxel_downsample takes them and has its cloud refusals (offsets, stride, null
 * buffers), plus dcreg_set_source's refusal of non-finite coordinates in ANY cloud of the call: raw sweeps go through the voxel or deskew
 * calls first, whose output is what this call takes with stride 3.  Empty clouds are accepted and become empty keyframes.  A refused call
 * or a failed allocation (DCREG_E_NOMEM) leaves the store as it was, bit for bit.  dcreg_keyframes_add_source adds the current source in
 * its INPUT order - the copy dcreg_target_insert_source reads - without a second upload.
 *
 * Member transform.  member_poses[12 m ..] = R[9] row-major, then t[3].  A stored point p becomes
 *     q_a = (float)(R[a][0] * (double)p_x + R[a][1] * (double)p_y + R[a][2] * (double)p_z + t[a]),
 * the sum evaluated left to right, every product and sum rounded to double, no contraction - the transform of dcreg_target_insert (an
 * identity pose therefore returns the stored values, a stored -0.0 as +0.0).  Poses must be finite; they are not checked for being
 * rotations, as in dcreg_target_insert.  A submap in a local frame (a candidate keyframe's own frame, or a frame near a vehicle far from
 * the origin) is the caller's pre-composed relative poses: the library composes nothing on the host, so the 12 numbers given fix the result.
 *
 * Submap.  Submap g has the members [member_offsets[g], member_offsets[g + 1]) (n_submaps + 1 offsets, from 0).  Its point sequence is
 * member after member in list order, each member's points in stored order.  An id may repeat within and across submaps; a submap may have
 * no members, and a member may be an empty keyframe.
 *
 * Output.  voxel == NULL: that sequence, 3 floats per point, submap after submap, submap g from out_offsets[g] (n_submaps + 1 entries);
 * vinfo: n_in = n_finite = n_out = the points written, n_voxels = 0.  voxel != NULL: bitwise dcreg_voxel_downsample of the n_submaps
 * sequences taken as n_clouds clouds - each submap keyed on its own, centroid sums in sequence order - so (out_xyz, out_offsets) is what
 * dcreg_register_pairs takes as targets with stride 3.  The capacity protocol is dcreg_voxel_downsample's: the member points in all are
 * always enough; a capacity the output does not fit returns DCREG_E_INVALID with out_offsets and vinfo filled and nothing written.  A
 * transformed coordinate that overflows float is non-finite, and what consumes it treats it as a non-finite input point: the voxel pass
 * drops it (counted in n_in - n_finite), the raw form writes it, the raw form of dcreg_set_target_keyframes refuses the call.
 *
 * dcreg_set_target_keyframes leaves the context bitwise as dcreg_set_target of the one-submap output of dcreg_keyframes_submaps with the
 * same arguments leaves it (with a voxel block: dcreg_set_target_voxel); the points go from the gather to the build on the device.  It
 * drops what dcreg_set_target drops; the store is untouched.  A refused call - the refusals below, no member, no point left, a non-finite
 * point in the raw form - leaves map and index as they were.
 *
 * Refusals.  DCREG_E_INVALID, nothing written: null arrays, negative counts, offsets that do not start at 0 or decrease, an id outside
 * [0, count), a non-finite pose, 2^31 - 1 or more member points in one call, the voxel pass's own refusals, an add that would take the
 * store to 2^32 points or more.  DCREG_E_STATE: a linearisation in flight (every call but _count); any call but _reset / _count before
 * the first _reset; _add_source without a source.  Every call that queues work waits for the stream before it returns.  A result depends on
 * the stored bits, the member lists, the poses and the voxel block only - not on the launch configuration, on what else the store or the
 * context holds, or on how many submaps share the call.
 *
 * Device memory: 12 B per stored point in one growing array whose capacity doubles - the new block is filled by a device-to-device copy
 * before the old one is released, so a growth peaks at old + new block, at most three times the bytes stored - and a host vector of int64
 * offsets.  Per call 104 B per non-empty member of scratch (output start, store offset, pose), uploaded in one copy; the raw form to host
 * memory stages its 12 B per point; the voxel form has the voxel pass's scratch. */
int dcreg_keyframes_reset(dcreg_ctx *);                       /* creates the store, or empties it and frees its points */
int64_t dcreg_keyframes_count(const dcreg_ctx *);             /* 0 before the first reset */
/* n_points[k] = the points of keyframe first + k, k < n; [first, first + n) must lie inside [0, count] */
int dcreg_keyframes_sizes(const dcreg_ctx *, int64_t first, int64_t n, int64_t *n_points);
/* first_id may be NULL.  _device: d_xyz is read as dcreg_voxel_downsample_device reads it */
int dcreg_keyframes_add_clouds(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats, int64_t *first_id);
int dcreg_keyframes_add_clouds_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                      int64_t *first_id);
int dcreg_keyframes_add_source(dcreg_ctx *, int64_t *id);    /* id may be NULL */
/* the stored points of one keyframe to host memory; DCREG_E_INVALID when capacity_points is below its size */
int dcreg_keyframes_get(dcreg_ctx *, int64_t id, float *xyz_out, int64_t capacity_points);
int dcreg_keyframes_submaps(dcreg_ctx *, int n_submaps, const int64_t *member_offsets, const int64_t *member_ids, const double *member_poses,
                            const dcreg_voxel_params *voxel, float *out_xyz, int64_t capacity_points, int64_t *out_offsets,
                            dcreg_voxel_info *vinfo);
/* d_out_xyz is device memory, written on the ctx's stream (the raw form writes it straight from the gather) */
int dcreg_keyframes_submaps_device(dcreg_ctx *, int n_submaps, const int64_t *member_offsets, const int64_t *member_ids,
                                   const double *member_poses, const dcreg_voxel_params *voxel, float *d_out_xyz, int64_t capacity_points,
                                   int64_t *out_offsets, dcreg_voxel_info *vinfo);
int dcreg_set_target_keyframes(dcreg_ctx *, int64_t n_members, const int64_t *member_ids, const double *member_poses,
                               const dcreg_voxel_params *voxel, double search_radius_hint, dcreg_voxel_info *vinfo);

/* ---------------- moving objects: visibility votes from keyframes ----------------
 * A map assembled from keyframes holds every car and pedestrian that moved while it was recorded, as a dense trail that the outlier
 * filters cannot remove.  The remedy is a range-image visibility check: a map point that other scans look THROUGH was not static.  The
 * keyframe store holds the scans, the caller the poses; every output is bitwise the numpy reference of tests/visibility_ref.py.
 *
 * Parameters (dcreg_visibility_params; the defaults of dcreg_default_visibility_params behind each):
 *   rows in [1, 256], cols in [1, 4096]                                          64, 1024
 *   elev_min < elev_max, both finite and inside [-pi/2, pi/2] (radians)          -pi/8, +pi/8
 *   0 <= min_range < max_range, finite (m)                                       0.5, 80
 *   margin_abs >= 0 (m), margin_rel >= 0, finite                                 0.2, 0.01
 *   window in [0, 3]                                                             1
 *   min_votes >= 1                                                               2
 *   min_ratio in [0, 1]                                                          0
 * Everything below is evaluated in double, left to right, every product and sum rounded, no contraction.
 *
 * Pixel of a sensor-frame point s.  rho2 = sx^2 + sy^2, r2 = rho2 + sz^2, r = sqrt(r2).  The point is USED iff r2 > 0 and
 * min_range^2 <= r2 < max_range^2 and, with
 *     az = atan2(sy, sx), plus 2 pi (6.283185307179586) when negative;   b = az * cols / 2 pi;   col = min(floor(b), cols - 1);
 *     el = atan2(sz, sqrt(rho2));   a = (elev_max - el) * rows / (elev_max - elev_min),
 * 0 <= a < rows; then row = floor(a): row 0 is at the top.  A point whose a or b lies within 1e-9 of an integer may fall on either side
 * (in or out at a = 0 and a = rows), as for the place descriptors: the device's atan2 is not the host's to the last bit.
 *
 * Range image of a keyframe.  Over its stored points, s = (double)p: image[row][col] = the minimum of (float)r over the used points of the
 * pixel, +inf for an empty pixel (rows x cols floats, row-major).  The minimum is an integer atomic minimum on the floats' bits (positive
 * values order as their bits do), so the image depends on neither the point order nor the launch shape.
 *
 * Vote of member (id, pose R, t; sensor -> map, 12 doubles as in the keyframe section) on a map-frame point q:
 *     d_a = (double)q_a - t[a];   s_a = R[0][a] * d_0 + R[1][a] * d_1 + R[2][a] * d_2      (the pose is not checked for being a rotation)
 * and the pixel of s as above; a point that is not used casts no vote.  m = the minimum of the member's image over the rows
 * row - window .. row + window that lie inside [0, rows) and the columns col - window .. col + window taken modulo cols.  m = +inf: no
 * vote.  Otherwise observed += 1, and through += 1 iff (double)m > r + (margin_abs + margin_rel * r).
 *
 * Decision.  Point i is REMOVED iff through_i >= min_votes and (double)through_i >= min_ratio * (double)observed_i.  The counts are
 * integers summed over the members: a result does not depend on the member order, on how the members are batched ("visibility_max_bytes"
 * of dcreg_set_option: the device bytes the range images of one batch may take, default 256 MiB, at least one image), or on what else
 * the context holds; a repeated member votes twice; an empty keyframe casts no vote.
 *
 * dcreg_visibility_filter takes one cloud in the map frame and has the shape of dcreg_outlier_filter: non-finite points are dropped and
 * counted (their counts are 0), the kept points are written in input order, bit for bit, and the optional outputs (NULL: not wanted) are
 * the keep mask uint8[n] and the counts int32 through[n], observed[n].  The capacity protocol is dcreg_outlier_filter's.
 * dcreg_target_remove_dynamic votes over the resident map's points (on a map with a window index the whole map's, as
 * dcreg_target_remove_outliers) and sends the survivors through the update path of dcreg_target_crop.  It carries the contract of the
 * map-update section: later calls are bitwise dcreg_set_target of the survivors in index order; a call that changes the map drops what
 * dcreg_set_target drops; a call that removes nothing changes nothing (the neighbour states stay warm); a call that would remove every
 * point is refused (DCREG_E_INVALID); refusals leave everything as it was.
 *
 * Refusals.  DCREG_E_INVALID, nothing written: null arrays, negative counts, an id outside [0, count), a non-finite pose, parameters
 * outside the ranges above, stride < 3, more than 2^31 - 1 points.  DCREG_E_STATE: a linearisation in flight; no store
 * (dcreg_keyframes_reset first); no target (the map form).  A failed allocation (DCREG_E_NOMEM) leaves the context as it was.  None of
 * the calls touches source, places, store, neighbour states or window index, except the map form as dcreg_target_crop does.  Every call
 * waits for the stream.  Device memory: the batch's images, 112 B per member, 8 B per point of counts and the filter's scratch. */
typedef struct dcreg_visibility_params {
    int rows, cols;                  /* the range image: elevation rows (row 0 at elev_max) x azimuth columns */
    double elev_min, elev_max;       /* radians */
    double min_range, max_range;     /* metres */
    double margin_abs, margin_rel;   /* a pixel sees through a point when its range exceeds r + margin_abs + margin_rel * r */
    int window, min_votes;
    double min_ratio;
} dcreg_visibility_params;
typedef struct dcreg_visibility_info {
    int64_t n_in;        /* points voted on */
    int64_t n_finite;    /* ... with three finite coordinates */
    int64_t n_observed;  /* ... with observed >= 1 */
    int64_t n_flagged;   /* ... removed by the decision */
    int64_t n_out;       /* points kept */
    int64_t n_members;   /* members of the call */
} dcreg_visibility_info;
int dcreg_default_visibility_params(dcreg_visibility_params *);
/* The range images of the keyframes ids[0 .. n), n x rows x cols floats to out (host memory; _device: device memory).  An id may repeat. */
int dcreg_keyframes_range_images(dcreg_ctx *, int64_t n, const int64_t *ids, const dcreg_visibility_params *, float *out);
int dcreg_keyframes_range_images_device(dcreg_ctx *, int64_t n, const int64_t *ids, const dcreg_visibility_params *, float *d_out);
/* *n_out receives the number of kept points; capacity_points = n is always enough; a smaller capacity that the output does not fit returns
 * DCREG_E_INVALID with *n_out and info filled and nothing written to out_xyz, keep_mask, through or observed.  info may be NULL.
 * _device: d_xyz is read as dcreg_set_source_device reads a cloud; the outputs are device memory. */
int dcreg_visibility_filter(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, int64_t n_members, const int64_t *member_ids,
                            const double *member_poses, const dcreg_visibility_params *, float *out_xyz, int64_t capacity_points,
                            int64_t *n_out, uint8_t *keep_mask, int32_t *through, int32_t *observed, dcreg_visibility_info *info);
int dcreg_visibility_filter_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, int64_t n_members,
                                   const int64_t *member_ids, const double *member_poses, const dcreg_visibility_params *, float *d_out_xyz,
                                   int64_t capacity_points, int64_t *n_out, uint8_t *d_keep_mask, int32_t *d_through, int32_t *d_observed,
                                   dcreg_visibility_info *info);
int dcreg_target_remove_dynamic(dcreg_ctx *, int64_t n_members, const int64_t *member_ids, const double *member_poses,
                                const dcreg_visibility_params *, dcreg_visibility_info *info);

/* ---------------- surface normals and curvature ----------------
 * pcl::NormalEstimation with setKSearch(k) on the device - what the reference's ICPContext::setTargetCloud(target, normal_nn) fills
 * targetNormals with - for one cloud or for the resident map, with a rule fixed tightly enough that the output is bitwise the numpy
 * reference of tests/normals_ref.py (INTEGRATION.md lists where it differs from PCL's arithmetic).  For one cloud of n points and the
 * parameters k (3 .. 32), search_radius (>= 0, 0 = unbounded), orient and viewpoint[3]:
 *   - used points: a point is used when x, y and z are all finite; the others get NaN in every output.  "Index" is the input index;
 *   - distances are the float d2 that dcreg_knn computes, (dx*dx + dy*dy) + dz*dz with every operation rounded to float; candidates are
 *     ranked by the total order (d2, index);
 *   - the neighbours of point i are the first k used points of the cloud in that order with d2 < bound.  The point itself is a candidate
 *     like any other, at d2 = 0 (PCL's NormalEstimation over its own input); among exact duplicates the index decides.
 *     bound = min((float)(search_radius^2), 3.0e38f) for search_radius > 0, and 3.0e38f - the bound of every unbounded search of this
 *     library - for search_radius = 0;
 *   - a used point with fewer than k such neighbours is SPARSE: NaN outputs, counted in n_sparse.  (With search_radius = 0 a cloud with
 *     fewer than k used points makes every used point sparse.)
 *   - covariance, all in double without contraction (every multiply and add rounds once): with the neighbours q_1 .. q_k in rank order,
 *     e_j = (double)q_j - (double)p_i per coordinate; s = e_1 + e_2 + ... summed left to right; m = s / k; d_j = e_j - m; the six unique
 *     C_ab = (sum_j d_ja * d_jb) / k, summed left to right, for xx, xy, xz, yy, yz, zz;
 *   - eigen-solve: cyclic Jacobi, exactly six sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the third index, from V = I:
 *       t = 0 if a_pq == 0, otherwise theta = (a_qq - a_pp) / (2 * a_pq) and t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta*theta + 1))
 *       (an overflowing theta gives t = 0 by IEEE arithmetic); c = 1 / sqrt(t*t + 1), a division and a square root; s = t * c;
 *       a_pp <- a_pp - t*a_pq; a_qq <- a_qq + t*a_pq; a_pq <- 0; a_rp <- c*a_rp - s*a_rq; a_rq <- s*a_rp(old) + c*a_rq;
 *       v_ip <- c*v_ip - s*v_iq; v_iq <- s*v_ip(old) + c*v_iq for i = 0, 1, 2.
 *     lambda is the diagonal.  The normal is the column of V at the smallest lambda (a tie: the lowest index), as computed - not
 *     renormalised (its length differs from 1 by rounding only);
 *   - trace = (lambda_0 + lambda_1) + lambda_2; curvature = |lambda_min| / trace, and 0 when trace == 0 (PCL's surface variation);
 *   - DCREG_NORMAL_ORIENT_VIEWPOINT (default, viewpoint (0,0,0) as PCL): the normal is negated when
 *     ((vx - (double)px)*nx + (vy - (double)py)*ny) + (vz - (double)pz)*nz < 0; a dot product of exactly 0 keeps the sign.
 *     DCREG_NORMAL_ORIENT_NONE leaves the solver's sign;
 *   - outputs per point, in input order: normal[3] = (float) of the doubles, curvature as a float, and optionally eigenvalues[3]: the
 *     three lambda ascending - through the exchanges (0,1), (1,2), (0,1), each swapping when the second is smaller - as floats;
 *   - info: n_in, n_finite, n_sparse and n_out = the points that received a normal (n_finite - n_sparse).
 * A point's result depends on the cloud and the parameters only: the index decides how fast the neighbours are found, never which.
 * Radius neighbourhoods (every point inside r, however many) are not offered: their sums would depend on the traversal order.
 * dcreg_normals reads one cloud as dcreg_set_source[_device] reads it; dcreg_target_normals covers the resident map's points in index
 * order (dcreg_target_get) and searches the map's own index - on a map with a window index the whole map's, as dcreg_knn.  Any of the
 * three outputs may be NULL (not wanted), but not all three.  Neither call changes the target, the source, neighbour states, the window
 * index, places or keyframes; both wait for the stream; repeated calls and calls on another context are bitwise equal.
 * An unbounded search of an isolated point walks the rings of the grid out to its k-th neighbour, as the outlier filter's does:
 * search_radius is the practical answer for clouds with far outliers.
 * DCREG_E_INVALID, before anything is queued: null context or parameters, k outside 3 .. 32, an unknown orient, a search_radius that is
 * not finite or is negative, a viewpoint that is not finite, stride < 3, n < 0, more than 2^31 - 1 points, a null cloud with n > 0, all
 * three outputs NULL, a capacity below the map's size.  DCREG_E_STATE: a linearisation in flight; no target (the map form).  A failed
 * allocation (DCREG_E_NOMEM) leaves the context as it was.  Device memory: the outlier filter's scratch for the cloud and its index
 * (the cloud form), and up to 28 B per point of outputs. */
#define DCREG_NORMAL_ORIENT_VIEWPOINT 0
#define DCREG_NORMAL_ORIENT_NONE 1
typedef struct dcreg_normal_params {
    int k;                 /* neighbours per point, the point itself among them (PCL setKSearch; the reference's normal_nn), 3 .. 32 */
    int orient;            /* DCREG_NORMAL_ORIENT_VIEWPOINT / DCREG_NORMAL_ORIENT_NONE */
    double search_radius;  /* 0 = unbounded, > 0 = neighbours beyond it do not count (m) */
    double viewpoint[3];   /* DCREG_NORMAL_ORIENT_VIEWPOINT: normals point to this side (PCL setViewPoint) */
    double reserved_[2];
} dcreg_normal_params;
typedef struct dcreg_normal_info {
    int64_t n_in;        /* points passed in / points of the map */
    int64_t n_finite;    /* ... with three finite coordinates (used) */
    int64_t n_sparse;    /* ... of those, with fewer than k neighbours inside the bound */
    int64_t n_out;       /* points that received a normal */
} dcreg_normal_info;
/* k = 5, DCREG_NORMAL_ORIENT_VIEWPOINT, search_radius = 0, viewpoint (0, 0, 0) */
int dcreg_default_normal_params(dcreg_normal_params *);
/* One cloud in (stride_floats floats per point, x y z first); normals_out 3 n floats, curvature_out n floats, eigenvalues_out 3 n floats
 * (host memory; _device: the cloud and the outputs are device memory).  info may be NULL. */
int dcreg_normals(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const dcreg_normal_params *, float *normals_out,
                  float *curvature_out, float *eigenvalues_out, dcreg_normal_info *info);
int dcreg_normals_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const dcreg_normal_params *, float *d_normals_out,
                         float *d_curvature_out, float *d_eigenvalues_out, dcreg_normal_info *info);
/* Many clouds in one call: cloud s = the points [offsets[s], offsets[s + 1]) of xyz (all clouds back to back, stride_floats floats per
 * point; offsets holds n_clouds + 1 entries, in points, starting at 0 - host memory in both forms).  The outputs are packed back to back
 * in input order, 3 floats per point of normals_out and 1 float per point of curvature_out (either may be NULL, not both; no eigenvalues
 * in this form); infos (may be NULL) receives one record per cloud.  Every value and every record is BITWISE what dcreg_normals returns
 * for that cloud alone with the same parameters - NaN for sparse and non-finite points included: a cloud's points never see another
 * cloud's.  Every cloud's finite points are indexed on their own, in cells chosen from its own bounds and density, all clouds in one
 * build (one upload, one sort per pass, one readback) and one kernel launch: the fixed cost of indexing a small cloud is paid once per
 * call, and neither the synchronises nor the launches grow with n_clouds.  A cloud with fewer than k finite points gets no index and
 * comes out all sparse, as in the single call.  n_clouds == 0 does nothing.  The refusals of dcreg_normals, and DCREG_E_INVALID for
 * offsets that do not start at 0 or decrease and for a call of 2^31 points or more - all before anything is queued. */
int dcreg_normals_clouds(dcreg_ctx *, int n_clouds, const float *xyz, const int64_t *offsets, int64_t stride_floats,
                         const dcreg_normal_params *, float *normals_out, float *curvature_out, dcreg_normal_info *infos);
int dcreg_normals_clouds_device(dcreg_ctx *, int n_clouds, const float *d_xyz, const int64_t *offsets, int64_t stride_floats,
                                const dcreg_normal_params *, float *d_normals_out, float *d_curvature_out, dcreg_normal_info *infos);
/* The resident map's points in index order; the outputs hold capacity_points points, at least the map's size. */
int dcreg_target_normals(dcreg_ctx *, const dcreg_normal_params *, float *normals_out, float *curvature_out, float *eigenvalues_out,
                         int64_t capacity_points, dcreg_normal_info *info);
int dcreg_target_normals_device(dcreg_ctx *, const dcreg_normal_params *, float *d_normals_out, float *d_curvature_out,
                                float *d_eigenvalues_out, int64_t capacity_points, dcreg_normal_info *info);

/* ---------------- kept normals and the 1-NN point-to-plane linearisation ----------------
 * The map can KEEP one normal per point on the device - float4 {nx, ny, nz, curvature} in index order (the order of dcreg_target_get) -
 * and a second linearisation registers against them: the correspondence stage of Open3D-style point-to-plane ICP, which is what the
 * reference fills targetNormals for (ICPContext::setTargetCloud(target, normal_nn); icp_test_runner.cpp:2944-2963, :2974-2981).  A
 * prior map fits its planes once; an iteration is then a 1-NN search, one 16-byte gather and a row.  The 6x6 system that comes out goes
 * through the solver seam below unchanged.
 *   dcreg_target_normals_keep   runs the map form of dcreg_target_normals into the member: bitwise what that call returns for the same
 *                               parameters (normal and curvature; a sparse point keeps NaN).  Nothing is downloaded; info may be NULL.
 *   dcreg_target_normals_set    takes the caller's normals, 3 floats first of stride_floats per point, in index order (curvature is
 *                               stored as NaN); n must equal the map's size.  Stored as given, not renormalised.
 *   A normal with any non-finite component means "this point has no normal".
 *   dcreg_target_normals_kept   1 while the member holds normals, else 0 (also for a null context);  _drop frees it.
 * Every call that changes the map's points or their index order drops the member: dcreg_set_target* in all its forms,
 * dcreg_target_insert*, dcreg_target_crop, dcreg_target_remove_outliers, dcreg_target_remove_dynamic, dcreg_set_target_keyframes
 * (the updates refit it instead under the option "normals_follow": see "kept normals that follow the map" below).
 * DCREG_E_INVALID, before anything is queued: null context, parameters or normals, the parameter refusals of dcreg_target_normals,
 * stride_floats < 3, n different from the map's size.  DCREG_E_STATE: a linearisation in flight; no target.  A failed allocation
 * (DCREG_E_NOMEM) leaves no kept normals.  16 B of device memory per map point.
 *
 * The rule of one linearisation (dcreg_linearize_normals; tests/normal_icp_ref.py states it in numpy).  Of the parameter block only
 * search_radius (R), weight_slope, weight_min and use_weight_derivative are read; parameterization must be DCREG_PARAM_SO3
 * (DCREG_E_INVALID otherwise).  Every operation rounds once (no contraction).  For each source point p (floats, widened to double):
 *   - q = R p + t as dcreg_linearize transforms a point: per coordinate ((R_a0*px + R_a1*py) + R_a2*pz) + t_a in double, stored as float;
 *   - candidates are ranked by the total order (d2, index) with the float d2 that dcreg_knn computes, (dx*dx + dy*dy) + dz*dz, every
 *     operation rounded to float; j is the first map point in that order (dcreg_knn with k = 1).  Flag 0 (radius gate) unless
 *     (double)d2 < R*R (icp_test_runner.cpp:2951); a d2 equal to R*R stays out.  A point that passes counts in n_pt;
 *   - n = the kept normal of j, widened to double.  Flag 2 when j has no normal;
 *   - e = (double)q - (double)t_j per coordinate; r = (nx*ex + ny*ey) + nz*ez;
 *   - s = 1 - weight_slope*|r|, and 0 when that is negative; ds = -weight_slope*(r > 0 ? 1 : -1) when use_weight_derivative and
 *     0 < s < 1, else 0.  Flag 4 unless s > weight_min (the weight and its gate are dcreg_linearize's);
 *   - m = R^T n, component k = (R_0k*nx + R_1k*ny) + R_2k*nz; w = s + r*ds; A = w * [p x m, m] with
 *     p x m = (py*m2 - pz*m1, pz*m0 - px*m2, px*m1 - py*m0): the right-perturbation row; b = -(s*r), in double (this engine has no
 *     float store of the coefficients).  Flag 1: the point is effective and its row is [A0..A5, b, r];
 *   - the sums, in dcreg_lin_out: H = sum A A^T, g = sum A b, sum_r2, sum_b2 = sum b^2 and n_eff over the effective points, n_pt.
 * The sums are added in a fixed order (no floating-point atomics): a result depends on the clouds, the normals, the pose and the
 * parameters only - not on earlier calls (each source point remembers where its last nearest neighbour sits and starts the next search
 * bounded by that point's distance, inclusive: a speed device only), not on the context, and not on whether the map is searched through
 * its window index.  Nothing of dcreg_linearize's neighbour states is read or written.
 * DCREG_E_INVALID: null arguments, a non-finite pose, a search_radius that is not finite and > 0, a parameterization other than SO3.
 * DCREG_E_STATE: no target, no source, no kept normals, a linearisation in flight.  Waits for the stream. */
int dcreg_target_normals_keep(dcreg_ctx *, const dcreg_normal_params *, dcreg_normal_info *info);
int dcreg_target_normals_set(dcreg_ctx *, const float *normals, int64_t n, int64_t stride_floats);
int dcreg_target_normals_set_device(dcreg_ctx *, const float *d_normals, int64_t n, int64_t stride_floats);
int dcreg_target_normals_kept(const dcreg_ctx *);
int dcreg_target_normals_drop(dcreg_ctx *);
int dcreg_linearize_normals(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *, dcreg_lin_out *);

/* ---------------- kept normals that follow the map ----------------
 * dcreg_set_option("normals_follow", 1) makes the map updates - dcreg_target_insert, _insert_device, _insert_source, dcreg_target_crop,
 * dcreg_target_remove_outliers, dcreg_target_remove_dynamic - UPDATE the kept normals instead of dropping them, so that a keyframe loop
 * (dcreg_set_source + dcreg_icp_run_normals + dcreg_target_insert_source, a crop every few keyframes) never pays for the whole map's
 * normals again.  Default 0: every update drops them, as stated above.  The option is read at the time of the update.  It applies only
 * while normals are kept AND they came from dcreg_target_normals_keep: the context remembers that call's parameter block and refits
 * with it.  Normals given by dcreg_target_normals_set have no rule to refit with and are dropped as before; dcreg_set_target* in all
 * its forms and dcreg_set_target_keyframes always drop (the map is a new one).
 *   Contract.  After a followed update dcreg_target_normals_get returns, bit for bit, what a fresh context with the same options returns
 *   after dcreg_set_target(M') + dcreg_target_normals_keep(params), M' = dcreg_target_get of the updated map; a sparse point keeps NaN.
 *   Everything built on the kept normals is therefore bitwise the fresh context's too: dcreg_linearize_normals, dcreg_icp_run_normals,
 *   dcreg_register_frames_normals, dcreg_icp_run_trials_normals.  The result does not depend on the sequence of updates, on
 *   "map_update", on whether an update merged into the grid or re-derived it (dcreg_map_update::rebuilt), or on whether the window
 *   index was active.  Only the points whose neighbourhood can have changed are computed: a point is refitted when an added or removed
 *   point may lie within the distance of its k-th neighbour (within the search bound for a sparse point) - a conservative test on the
 *   cells of the grid, never an approximation; past a share of the map everything is recomputed, with the same bits.
 *   An update that changes nothing (an insert whose points were all thinned away, a crop that keeps everything) leaves normals and info
 *   as they were; a refused update leaves the normals bitwise as they were.  If following runs out of memory after the map has changed,
 *   the update stands and its return code is unchanged: the normals are dropped (dcreg_target_normals_kept 0, followed 0).  The start
 *   positions of the next searches and the warm slots of the batched form are invalidated by every update exactly as without the option
 *   (positions in the sorted array move).  Memory: 4 B more per map point beside the 16 B of a kept normal - 20 B in all - from
 *   dcreg_target_normals_keep on, with the option or without; a removal holds a second copy of both arrays until the next one reuses it.
 *   dcreg_target_normals_get[_device]   the kept normals in index order, 4 floats per point: nx ny nz curvature (NaN where the point has
 *                                       none).  What a caller persists with a map.  DCREG_E_STATE: no kept normals, a linearisation in
 *                                       flight.  DCREG_E_INVALID: null context or buffer, capacity_points below the map's size.  Waits
 *                                       for the stream.
 *   dcreg_target_normals_follow_info    what the last update that changed the map did (all zero after dcreg_set_target* in any of its forms: a new map has had no update yet): n_target = the map's size after it, n_refit =
 *                                       points whose normal it computed (added points included), n_carried = points whose stored normal
 *                                       was moved over unchanged, followed = 0 not followed (the normals were dropped, or no update
 *                                       yet), 1 incremental, 2 followed by a full recompute.  n_refit + n_carried == n_target when
 *                                       followed.  DCREG_E_INVALID: null context or info. */
typedef struct dcreg_normals_follow_info {
    int64_t n_target, n_refit, n_carried;
    int followed;
    int reserved_;
} dcreg_normals_follow_info;
int dcreg_target_normals_get(dcreg_ctx *, float *out, int64_t capacity_points);
int dcreg_target_normals_get_device(dcreg_ctx *, float *d_out, int64_t capacity_points);
int dcreg_target_normals_follow_info(const dcreg_ctx *, dcreg_normals_follow_info *info);

/* ---------------- kept source normals and the plane-to-plane (GICP) linearisation ----------------
 * Generalized-ICP (Segal, Haehnel, Thrun 2009) weighs a correspondence by the covariances of both surfaces.  With the plane-regularised
 * covariance of that paper (fast_gicp's PLANE mode) - eigenvalues (1, 1, eps) around the normal - a covariance is a function of its
 * normal, C = I - (1 - eps) n n^T, so both sides' covariances and their sum at a pose are formed from the two normals in registers:
 * the map keeps its normals (above), the SOURCE keeps its own beside its points, and nothing else is stored.  The whitened residual
 * L^-1 e (Sigma = L L^T) turns one correspondence into three point-to-plane rows whose pseudo-normals are the rows of L^-1; the 6x6
 * system goes through the solver seam below unchanged.
 *   dcreg_source_normals_keep   runs dcreg_normals on the context's source points: bitwise what that call returns for the source's
 *                               points in their original order (normal and curvature; a sparse point keeps NaN).  info may be NULL.
 *   dcreg_source_normals_set    takes the caller's normals, 3 floats first of stride_floats per point, in the source's original order
 *                               (curvature is stored as NaN); n must equal the source's size.  Stored as given, not renormalised.
 *   A normal with any non-finite component means "this point has no normal".
 *   dcreg_source_normals_get    4 floats per point (nx ny nz curvature) in the source's original order.
 *   dcreg_source_normals_kept   1 while the member holds normals, else 0 (also for a null context);  _drop frees it.
 * Every call that replaces the context's source points drops the member: dcreg_set_source* in all its forms (plain, _device, _voxel,
 * _outliers, _deskew, _deskew_path).  The batched calls (dcreg_register_frames*, dcreg_icp_run_trials*, dcreg_register_pairs), which
 * leave the context's own source as it was, leave the member as it was.  Nothing follows anything: the source normals are not updated.
 * DCREG_E_INVALID, before anything is queued: null context, parameters, normals or output, the parameter refusals of dcreg_normals,
 * stride_floats < 3, n different from the source's size, a capacity below it.  DCREG_E_STATE: a linearisation in flight; no source;
 * _get without kept source normals.  A failed allocation (DCREG_E_NOMEM) leaves no kept source normals.  16 B of device memory per
 * source point.
 *
 * The rule of one linearisation (dcreg_linearize_gicp; tests/gicp_ref.py states it in numpy).  eps = the option "gicp_epsilon" at the
 * time of the call, c = 1 - eps.  Of the parameter block only search_radius (R) is read - the second engine's weight and its gate do
 * not apply; parameterization must be DCREG_PARAM_SO3 (DCREG_E_INVALID otherwise).  Every operation rounds once in double (no
 * contraction).  For each source point p (floats, widened to double):
 *   - transform, nearest point j and radius gate exactly as dcreg_linearize_normals: q stored as float, j the first map point in
 *     (float d2, index) order, flag 0 unless (double)d2 < R*R.  A point that passes counts in n_pt;
 *   - n = the kept normal of j, flag 2 when it has none; m = the kept normal of p, flag 3 when it has none (in this order);
 *   - u = R m, component a = (R_a0*mx + R_a1*my) + R_a2*mz;  S_ab = d_ab - c*(n_a*n_b + u_a*u_b) with d_ab = 2 on the diagonal and
 *     0 off it, for the six entries of the lower triangle: the covariance C_map + R C_src R^T of the pair;
 *   - the Cholesky factor, in this order: l00 = sqrt(S00); l10 = S10/l00; l20 = S20/l00; l11 = sqrt(S11 - l10*l10);
 *     l21 = (S21 - l20*l10)/l11; l22 = sqrt((S22 - l20*l20) - l21*l21).  Flag 5 (not positive definite) unless each of the three
 *     radicands is > 0 - possible only with caller-given normals that are not unit length;
 *   - W = L^-1: w00 = 1/l00; w11 = 1/l11; w22 = 1/l22; w10 = -(l10*w00)*w11; w21 = -(l21*w11)*w22; w20 = -(l20*w00 + l21*w10)*w22.
 *     The pseudo-normals are its rows: a_0 = (w00, 0, 0), a_1 = (w10, w11, 0), a_2 = (w20, w21, w22) - the zeros are multiplied and
 *     added below like any other value;
 *   - e = (double)q - (double)t_j per coordinate.  For k = 0, 1, 2: r_k = (a_kx*ex + a_ky*ey) + a_kz*ez; m_k = R^T a_k, component
 *     i = (R_0i*a_kx + R_1i*a_ky) + R_2i*a_kz; row k = [p x m_k, m_k, -r_k, r_k] with p x m = (py*m2 - pz*m1, pz*m0 - px*m2,
 *     px*m1 - py*m0): the second engine's row with weight 1, a right perturbation as dcreg_boxplus applies it.  Flag 1;
 *   - the sums, in dcreg_lin_out, over the THREE rows of every flag-1 point: H = sum A A^T, g = sum A b; sum_r2 and sum_b2 are both
 *     the sum of the squared Mahalanobis distances e^T S^-1 e.  n_eff counts the flag-1 POINTS (not rows), n_pt the points with flag != 0.
 * The sums are added in a fixed order (no floating-point atomics): a result depends on the clouds, both sets of normals, the pose,
 * R and eps only - not on earlier calls, not on the context, not on the window index.  The search starts from the warm bound that
 * dcreg_linearize_normals keeps per source point and leaves its own there: both look for the same nearest point, so calls of the two
 * may interleave on one context and neither moves a bit of the other.  Nothing of dcreg_linearize's neighbour states is read or written.
 * DCREG_E_INVALID: null arguments, a non-finite pose, a search_radius that is not finite and > 0, a parameterization other than SO3.
 * DCREG_E_STATE: no target, no source, no kept normals, no kept source normals, a linearisation in flight.  Waits for the stream. */
int dcreg_source_normals_keep(dcreg_ctx *, const dcreg_normal_params *, dcreg_normal_info *info);
int dcreg_source_normals_set(dcreg_ctx *, const float *normals, int64_t n, int64_t stride_floats);
int dcreg_source_normals_set_device(dcreg_ctx *, const float *d_normals, int64_t n, int64_t stride_floats);
int dcreg_source_normals_get(dcreg_ctx *, float *out, int64_t capacity_points);
int dcreg_source_normals_get_device(dcreg_ctx *, float *d_out, int64_t capacity_points);
int dcreg_source_normals_kept(const dcreg_ctx *);
int dcreg_source_normals_drop(dcreg_ctx *);
int dcreg_linearize_gicp(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *, dcreg_lin_out *);

/* ---------------- robust kernels (second and third engine) ----------------
 * dcreg_linearize_normals weights a correspondence by the reference's s = 1 - weight_slope*|r| alone, dcreg_linearize_gicp by nothing:
 * a wrong correspondence inside the radius gate - a parked car that has moved, the part of a loop-closure pair that does not overlap -
 * enters nearly or entirely in full.  The option "robust_kernel" turns each row of those two linearisations into a row of iteratively
 * reweighted least squares: it is multiplied by k = sqrt(rho'(r) / r) of the chosen kernel rho at the correspondence's residual, so that
 * H and g are the kernel's weighted sums.  k is a constant of the iteration: no derivative of k enters the row.
 *
 * The rule.  kind = "robust_kernel", c = "robust_scale" (second engine) or "gicp_robust_scale" (third engine) at the time of the
 * linearisation; c2 = c * c, formed once on the host in double.  Every operation rounds once in double (no contraction); division
 * and square root are IEEE double.  factor(kind, u2):
 *   - DCREG_ROBUST_HUBER:          u = sqrt(u2); k = 1 if u <= 1, else k = sqrt(1 / u);
 *   - DCREG_ROBUST_CAUCHY:         k = 1 / sqrt(1 + u2);
 *   - DCREG_ROBUST_GEMAN_MCCLURE:  k = 1 / (1 + u2).
 * dcreg_linearize_normals: flags, r, s, ds and w exactly as without a kernel - the gates do not change, so n_eff and n_pt at a pose
 * do not change.  For a flag-1 point with the row [A0..A5, b, r]: u2 = (r * r) / c2; k = factor(kind, u2); the row becomes
 * [k*A0, .., k*A5, k*b, r] - each of the seven products one more rounding on the value of the rule above.  Slot 7 stays r: sum_r2,
 * and with it the rmse, keeps its geometric meaning; sum_b2 is the sum of the scaled b squared.
 * dcreg_linearize_gicp: with the three residuals r_0, r_1, r_2 of a flag-1 point (r_k as the rule above forms it):
 * m2 = (r_0*r_0 + r_1*r_1) + r_2*r_2 (the squared Mahalanobis distance); u2 = m2 / c2; ONE k = factor(kind, u2) per point.  Slots
 * 0..6 of all three rows are multiplied by k; slot 7 stays r_k.
 * DCREG_ROBUST_NONE: nothing is multiplied - every call returns the bytes it returned before the option existed.
 *
 * Every form of the two engines follows the three options without a new entry point: dcreg_linearize_normals / _gicp,
 * dcreg_icp_run_normals / _gicp, dcreg_icp_run_trials_normals / _gicp, dcreg_register_frames_normals / _gicp,
 * dcreg_register_pairs_normals / _gicp and the *_batch_begin calls of dcreg_debug.h.  The engines' host steps, logs, covariance,
 * aborts and convergence test are untouched; H_upper of a log or a record is the SCALED Hessian (the kernel's weights are in it).
 * The batched forms stay bitwise their serial sequence - the one run on a context with the same three option values.  The debug
 * dumps (dcreg_debug.h) keep their layout: `row` is the scaled row, and r (and s) beside it are enough to check k.
 * The FIRST engine (dcreg_linearize, dcreg_icp_run, dcreg_register_frames, dcreg_register_pairs, ...), the Euler form and the
 * sharded forms do not read these options: their weight is the reference's.  Not provided: redescending kernels (Tukey), scales
 * estimated from the data (MAD), graduated non-convexity, a scale per pair in the pairs form.
 * The default scales (0.1 m, 1.0) are starting values that nobody has tuned: a scale near the noise of a good correspondence leaves
 * the inliers at k close to 1. */
#define DCREG_ROBUST_NONE 0
#define DCREG_ROBUST_HUBER 1
#define DCREG_ROBUST_CAUCHY 2
#define DCREG_ROBUST_GEMAN_MCCLURE 3

/* ---------------- kept voxel distributions and the voxel-distribution linearisation (fourth engine) ----------------
 * The second and third engine find every point's match with an exact 1-NN search at every linearisation.  Voxelised GICP and NDT (Koide
 * et al. 2021; Magnusson 2009) do not search: the map is summarised ONCE as one Gaussian per voxel, and a transformed source point's
 * correspondence is the voxel it falls into - a constant-time lookup, nothing walked, nothing kept between calls.  The map side needs no
 * normals, and the correspondence basin is a voxel edge instead of a search radius: the cheap, wide-basin stage that a GICP or 1-NN run
 * follows.  It is density-hungry and centimetre-grade, not a replacement for those engines.
 *
 * The rule of the kept voxel map (dcreg_target_voxels_keep; tests/voxels_ref.py states it in numpy).  The map's points are taken in index
 * order (the order of dcreg_target_get).  Every operation is in double and rounds once (no contraction).
 *   - the voxel of a point: v_a = floor((double)p_a / leaf) per axis - the voxel pass's rule with one leaf for all axes.  A voxel's
 *     members are its points in ascending index; n is their count;
 *   - a voxel with n < min_points is not kept and counts in n_small;
 *   - mean: s_a = the left-to-right sum of (double)p_a; mu_a = s_a / n;
 *   - covariance, a second pass over the same points: d_j = (double)p_j - mu; the six entries C_ab = (sum_j d_ja * d_jb) / n, summed left
 *     to right, in the order xx, xy, xz, yy, yz, zz;
 *   - eigen-solve: exactly the cyclic Jacobi of the normals rule (six sweeps; "surface normals and curvature" above).  It leaves
 *     lambda_0..2 (the diagonal) and V (columns);
 *   - normalised clamp (fast_gicp's NORMALIZED_MIN_EIG): lmax = the largest lambda.  Unless lmax > 0 and all three lambda are finite the
 *     voxel is not kept and counts in n_degenerate (coincident points are the usual case).  l_k = lambda_k / lmax, replaced by epsilon
 *     when l_k < epsilon.  C'_ab = ((V_a0*l_0)*V_b0 + (V_a1*l_1)*V_b1) + (V_a2*l_2)*V_b2 for the lower triangle (a >= b): xx = C'_00,
 *     xy = C'_10, xz = C'_20, yy = C'_11, yz = C'_21, zz = C'_22;
 *   - the kept record: (float)mu[3], (float)C'[6] in that order, n.  48 bytes, padded so that a lookup is three 16-byte loads.  The floats
 *     are widened to double at use: that is part of the rule.
 * dcreg_target_voxels_get returns the kept voxels in ascending (v_z, v_y, v_x) order: absolute voxel coordinates (3 per voxel), counts,
 * means (3) and covariances (6).  dcreg_target_voxels_kept: the number of kept voxels, 0 without a member (also for a null context);
 * _drop frees the member.  A keep that keeps no voxel succeeds, fills info and leaves no member.
 * A voxel's record depends on its own points and the three parameters only - not on the launch shape, the lookup structure or other
 * voxels.  One lane reduces one voxel (that fixes the summation order): a call pays for its fullest voxel.  The lookup structure is an
 * open-addressing table of 64-bit keys (the voxel relative to the map's minimum voxel, 21 bits per axis) with linear probing, at most
 * half full; a query outside the map's voxel box answers "none" without reading it.  Device memory: 56 B per kept voxel (record and key)
 * and 12 B per table slot - the power of two at or above twice the kept voxels - 80 to 104 B per kept voxel in all; a keep also uses
 * 48 B of scratch per occupied voxel and the voxel pass's scratch per map point.
 * Every call that changes the map's points drops the member: dcreg_set_target* in all its forms, dcreg_target_insert*,
 * dcreg_target_crop, dcreg_target_remove_outliers, dcreg_target_remove_dynamic and dcreg_set_target_keyframes - unless the option
 * "voxels_follow" makes the updates refit it ("kept voxel map that follows the map" below).
 * DCREG_E_INVALID, before anything is queued: null context, parameters or outputs; a leaf that is not finite and > 0; epsilon outside
 * [1e-6, 1]; min_points < 2; a capacity_voxels below the kept voxels; and, once the points' voxels are known and before anything is kept,
 * a map that spans 2^21 or more voxels on an axis or has a voxel coordinate of magnitude 2^62 or more (the voxel pass's limits).
 * DCREG_E_STATE: no target, a linearisation in flight, _get without a member.  A failed allocation (DCREG_E_NOMEM) leaves no member.
 *
 * The rule of one linearisation (dcreg_linearize_voxels).  Of the parameter block only parameterization is read (DCREG_PARAM_SO3, else
 * DCREG_E_INVALID); there is no radius gate - a point is at most a voxel diagonal from its mean.  Options, read at every call:
 * "voxels_source_cov" = 0 (default) point-to-distribution (any value but 0 or 1: DCREG_E_INVALID, the old value stays), 1 distribution-to-distribution with the source's plane covariance from its
 * kept normals (dcreg_source_normals_keep / _set) and eps = "gicp_epsilon" as the third engine reads it, c = 1 - eps; "robust_kernel" and
 * "gicp_robust_scale" exactly as dcreg_linearize_gicp applies them (one k per point from the squared Mahalanobis distance, slots 0..6
 * of all three rows scaled, slot 7 left; kernel 0 multiplies nothing).  For each source point p (floats, widened to double):
 *   - q is formed as every engine forms it (stored as float);
 *   - v_a = floor((double)q_a / leaf) with the member's leaf.  Flag 0 when no kept voxel has these coordinates; otherwise the point
 *     counts in n_pt;
 *   - mode 1 only: m = the point's kept source normal, flag 3 when it has none; u = R m, summed as dcreg_linearize_gicp sums it;
 *   - S_ab = C'_ab (the record's floats, widened) in mode 0; S_ab = C'_ab + (d_ab - c*(u_a*u_b)) in mode 1, d_ab = 1 on the diagonal
 *     and 0 off it, for the six entries of the lower triangle;
 *   - the Cholesky factor and W = L^-1 by the third engine's formulas in its order.  Flag 5 unless the three radicands are > 0;
 *   - e = (double)q - (double)mu per coordinate (mu: the record's floats); the three rows as dcreg_linearize_gicp forms them from W, e
 *     and p, scaled by the robust kernel's k where one is on.  Flag 1;
 *   - the sums are the third engine's: three rows per flag-1 point, n_eff counts points, sum_r2 and sum_b2 are both the Mahalanobis sum
 *     (sum_b2 of the scaled rows with a kernel on), added in a fixed order (no floating-point atomics).
 * A result depends on the source, the kept records, the pose and the options only.  The call neither reads nor writes warm words,
 * neighbour states, the window index or the map's kept normals: it may be interleaved with every other engine's calls without moving a
 * bit on either side.  DCREG_E_INVALID: null arguments, a non-finite pose, a parameterization other than SO3.  DCREG_E_STATE: no target,
 * no source, no kept voxels, in mode 1 no kept source normals, a linearisation in flight.  Waits for the stream.
 *
 * Neighbour-voxel correspondences.  Option "voxels_neighbors" = S, S = 1 (default), 7 or 27 (any other value: DCREG_E_INVALID, the old
 * value stays), read at every call with the options above: a point is matched to the kept voxels of a stencil around its own, S
 * correspondences per point with three rows each.  With S = 1 every byte is the rule above.  Everything not named here is the rule above:
 *   - q and v are formed as above.  The stencil is a fixed list of integer offsets o_j, j = 0..S-1.  S = 7: (0,0,0), (+1,0,0), (-1,0,0),
 *     (0,+1,0), (0,-1,0), (0,0,+1), (0,0,-1).  S = 27: (0,0,0) first, then the other 26 offsets of the 3 x 3 x 3 block in ascending
 *     (dz, dy, dx);
 *   - correspondence j is the kept voxel at u = v + o_j, the sum formed in double before the box test: a u outside the map's voxel box
 *     answers "none" without reading the table (so the key is never formed from a negative difference), and a v that is not finite
 *     gives no correspondence at all;
 *   - every correspondence has its own flag: 0 no kept voxel at u, 3 (mode 1) the point has no source normal - every found voxel of that
 *     point gets flag 3 - 5 not positive definite, 1 effective.  S_ab, its Cholesky factor, W, e = (double)q - (double)mu_j and the
 *     three rows are formed per correspondence, exactly as above, from that voxel's record;
 *   - mode 1: the source normal m and u = R m are the point's own, read and formed once, not per neighbour;
 *   - with a robust kernel on there is one factor k_j per correspondence, from that correspondence's own squared Mahalanobis distance,
 *     applied to slots 0..6 of its three rows;
 *   - the sums are over all rows of all flag-1 correspondences, in the fixed order (point, j, row k) within a lane - pass 3 j + k of the
 *     wave's accumulation - and without floating-point atomics.  n_pt counts the points with at least one flag != 0, n_eff the points
 *     with at least one flag 1: both count points, not rows or correspondences.
 * The correspondences are not weighted: every effective one adds its full Mahalanobis distance.  A neighbour voxel's thin Gaussian then
 * pulls as hard as the point's own, so S > 1 is meant to run in mode 1 or under a robust kernel (DESIGN.md section 24 has the figures).
 * The batched forms - many trials of the own source, many frames, many scan pairs with a voxel map per target - are
 * dcreg_icp_run_trials_voxels, dcreg_register_frames_voxels and dcreg_register_pairs_voxels below (the engine is density-hungry on
 * scan-sized targets: DESIGN.md sections 21 to 23).
 * Not provided: correspondences weighted by the voxel's point count, sharded / Euler forms, a caller-supplied voxel map, the runner's
 * YAML. */
typedef struct dcreg_voxel_map_params {
    double leaf;      /* voxel edge, metres (default 1.0) */
    double epsilon;   /* floor of the normalised eigenvalues (default 1e-3) */
    int min_points;   /* a voxel with fewer points is not kept (default 6) */
    int reserved_;
} dcreg_voxel_map_params;
typedef struct dcreg_voxel_map_info {
    int64_t n_points, n_voxels, n_small, n_degenerate, n_kept;
} dcreg_voxel_map_info;
int dcreg_default_voxel_map_params(dcreg_voxel_map_params *);      /* leaf 1.0, epsilon 1e-3, min_points 6 */
int dcreg_target_voxels_keep(dcreg_ctx *, const dcreg_voxel_map_params *, dcreg_voxel_map_info *info /* may be NULL */);
int dcreg_target_voxels_get(dcreg_ctx *, int64_t *coords /*3V*/, int32_t *count /*V*/, float *mean /*3V*/, float *cov /*6V*/,
                            int64_t capacity_voxels);
int dcreg_target_voxels_kept(const dcreg_ctx *);   /* number of kept voxels, 0 without a member */
int dcreg_target_voxels_drop(dcreg_ctx *);
int dcreg_linearize_voxels(dcreg_ctx *, const double R[9], const double t[3], const dcreg_lin_params *, dcreg_lin_out *);

/* ---------------- kept voxel map that follows the map ----------------
 * dcreg_set_option("voxels_follow", 1) makes the map updates - dcreg_target_insert, _insert_device, _insert_source, dcreg_target_crop,
 * dcreg_target_remove_outliers, dcreg_target_remove_dynamic - UPDATE the kept voxel map instead of dropping it, so that a keyframe loop
 * (dcreg_set_source + dcreg_icp_run_voxels + dcreg_target_insert_source, a crop every few keyframes) never sorts the whole map again.
 * Default 0: every update drops the member, as stated above.  The option is read at the time of the update.  It applies only while a
 * member exists (dcreg_target_voxels_kept() > 0): the context remembers the parameter block (leaf, epsilon, min_points) of the
 * dcreg_target_voxels_keep that made it and refits with it.  dcreg_set_target* in all its forms and dcreg_set_target_keyframes always
 * drop (the map is a new one).
 *   Contract.  After a followed update dcreg_target_voxels_get returns, bit for bit, what a fresh context returns after
 *   dcreg_set_target(M') + dcreg_target_voxels_keep(params), M' = dcreg_target_get of the updated map: coordinates, counts, means and
 *   covariances in ascending (v_z, v_y, v_x) order, and dcreg_target_voxels_kept agrees.  Every dcreg_linearize_voxels dump and sum
 *   agrees too, at "voxels_neighbors" 1, 7 and 27 and in both "voxels_source_cov" modes; dcreg_icp_run_voxels,
 *   dcreg_icp_run_trials_voxels and dcreg_register_frames_voxels are therefore bitwise the fresh context's.  The result does not depend
 *   on the sequence of updates, on "map_update", on whether an update merged into the grid or re-derived it
 *   (dcreg_map_update::rebuilt), on whether the window index was active, or on whether the update ran incrementally or as a full keep.
 *   A voxel's record is a function of its points in index order, so a voxel that holds an added or a removed point ("touched") is
 *   reduced again from ALL of its points; the records of every other voxel are moved over unchanged.
 *   An update that changes nothing (an insert whose points were all thinned away, a crop that keeps everything) leaves the member and
 *   the info as they were; a refused update leaves the member bitwise as it was.  If the follow leaves no kept voxel the member goes,
 *   exactly as a keep that keeps nothing leaves none.  The follow may fail after the map has changed - out of memory, an updated map
 *   that spans 2^21 or more voxels on an axis, a voxel coordinate of magnitude 2^62 or more: the keep's own refusals.  The update then
 *   stands with its return code unchanged, and the voxel map is dropped (dcreg_target_voxels_kept 0, followed 0).
 *   Memory while a followed update runs: a second copy of the records, keys and table (56 B per kept voxel, 12 B per slot; it stays
 *   until the next update reuses it), 20 B per kept voxel of merge scratch, the touched set (8 B per slot, the power of two at or above
 *   twice the changed points), 8 B per point of the updated map (the voxel pass's own scratch, as a keep sizes it), and for the
 *   gathered subset - the points of the touched voxels - 16 B per point plus the voxel pass's scratch per point and 48 B per voxel.
 *   dcreg_target_voxels_follow_info     what the last update that changed the map did (all zero after dcreg_set_target* in any of its
 *                                       forms: a new map has had no update yet): n_target = the map's size after it; n_touched = the
 *                                       distinct voxels that hold an added or removed point; n_refit = voxels reduced again (the
 *                                       touched voxels still occupied after the update; every occupied voxel when followed is 2);
 *                                       n_carried = kept records moved over unchanged; n_kept = kept voxels after the update
 *                                       (n_kept - n_carried = the refitted voxels that ended up kept); followed = 0 not followed
 *                                       (the member was dropped, or no update yet), 1 incremental, 2 followed by the full keep.
 *                                       DCREG_E_INVALID: null context or info. */
typedef struct dcreg_voxels_follow_info {
    int64_t n_target, n_touched, n_refit, n_carried, n_kept;
    int followed;
    int reserved_;
} dcreg_voxels_follow_info;
int dcreg_target_voxels_follow_info(const dcreg_ctx *, dcreg_voxels_follow_info *info);

/* ---------------- solver seam (host only, no device needed) ---------------- */
/* Config + ICPParameters subset (utils.hpp:82-171) */
typedef struct dcreg_config {
    double search_radius;
    int max_iterations;
    double CONVERGENCE_THRESH_ROT, CONVERGENCE_THRESH_TRANS;
    double DEGENERACY_THRES_COND, DEGENERACY_THRES_EIG;
    double KAPPA_TARGET, PCG_TOLERANCE;
    int PCG_MAX_ITER;
    double STD_REG_GAMMA, ADAPTIVE_REG_ALPHA;
    int use_weight_derivative;  /* additive key: icp_test_runner.cpp:1691 as a switch */
    int always_compute_schur;   /* additive key: fill Schur/diag numbers for every method (paper traces) */
    int euler_exact_jacobian;   /* additive key, dcreg_icp_run_euler only: 0 (default) = the reference's row (DCREG_PARAM_EULER),
                                   1 = the exact derivative (DCREG_PARAM_EULER_EXACT) */
    int reserved_cfg_;
    double gt_matrix[16];       /* row-major */
} dcreg_config;

/* DegeneracyAnalysisResult (utils.hpp:427-448) */
typedef struct dcreg_analysis {
    int isDegenerate;
    int degenerate_mask[6];
    double cond_schur_rot, cond_schur_trans;
    double cond_diag_rot, cond_diag_trans;
    double cond_full;
    double cond_full_sub_rot, cond_full_sub_trans;
    double eigenvalues_full[6];   /* ascending */
    double eigenvectors_full[36]; /* row-major, column i <-> eigenvalue i */
    double singular_values[6];    /* descending */
    double lambda_schur_rot[3], lambda_schur_trans[3];
    double lambda_sub_rot[3], lambda_sub_trans[3];
    double schur_V_rot[9], schur_V_trans[9];
    double aligned_V_rot[9], aligned_V_trans[9];
    int rot_indices[3], trans_indices[3];
    double P_preconditioner[36];
    double W_adaptive[36];
    int pcg_iterations;
} dcreg_analysis;

void dcreg_default_config(dcreg_config *);
int dcreg_analyze_degeneracy(const double H[36], int detection, int handling, const dcreg_config *, dcreg_analysis *);
int dcreg_solve_degenerate_system(const double H[36], const double g[6], int handling, const dcreg_config *,
                                  dcreg_analysis *, double x[6]);
void dcreg_unpack_hessian(const double H_upper[21], double H[36]);
void dcreg_boxplus(const double R[9], const double t[3], const double dx[6], double R_out[9], double t_out[3]);
void dcreg_pose6d_to_matrix(double roll, double pitch, double yaw, double x, double y, double z, double T[16]);
void dcreg_pose_error(const double gt[16], const double T[16], double *trans_m, double *rot_deg);

/* ---------------- engine seam ---------------- */
/* IterationLogData (utils.hpp:174-249) */
typedef struct dcreg_iter_log {
    int iter_count;
    int64_t effective_points, corr_pt_count;
    double rmse, fitness, objective_value;
    double gradient[6];
    double update_dx[6];
    double transform_matrix[16];
    double trans_error_vs_gt, rot_error_vs_gt;
    double iter_time_ms;
    double H_upper[21];
    dcreg_analysis analysis;
} dcreg_iter_log;

typedef struct dcreg_icp_result {
    int converged;
    int iterations;
    int status;        /* 0 ok, 1 n_eff<10 abort (:1847), 2 non-finite dx abort (:1942), 3 bad input (:1635) */
    double R[9], t[3];
    double icp_cov[36];
    double time_ms;
} dcreg_icp_result;

int dcreg_icp_run(dcreg_ctx *, const double R0[9], const double t0[3], int detection, int handling,
                  const dcreg_config *, dcreg_iter_log *log, int log_capacity, dcreg_icp_result *);

/* The loop of dcreg_icp_run with dcreg_linearize_normals as its linearisation (the map's kept normals: dcreg_target_normals_keep / _set
 * first, DCREG_E_STATE without them): the same aborts (n_eff < 10, a non-finite step), fitness n_pt / N_src, rmse, convergence test, log
 * records, covariance and status codes, the same host step.  One pose per call; dcreg_register_frames_normals and
 * dcreg_icp_run_trials_normals (below) run many registrations in one call, dcreg_register_pairs_normals many pairs, each against a
 * target of its own.  There is no sharded / RCCL form and no Euler form of this engine. */
int dcreg_icp_run_normals(dcreg_ctx *, const double R0[9], const double t0[3], int detection, int handling,
                          const dcreg_config *, dcreg_iter_log *log, int log_capacity, dcreg_icp_result *);

/* The same loop with dcreg_linearize_gicp as its linearisation (kept map normals AND kept source normals first, DCREG_E_STATE without
 * either): one waited launch per iteration, the same aborts, fitness, convergence test, log records, covariance and status codes, the
 * same host step.  rmse keeps its formula sqrt(sum_r2 / n_eff): here the RMS Mahalanobis distance per effective point (three whitened
 * residuals each), not a distance in metres.  Of the configuration's linearisation parameters only search_radius is read.  One pose per
 * call; dcreg_register_frames_gicp and dcreg_icp_run_trials_gicp (below) run many registrations in one call, dcreg_register_pairs_gicp
 * many pairs, each against a target of its own.  No sharded / RCCL or Euler form of this engine. */
int dcreg_icp_run_gicp(dcreg_ctx *, const double R0[9], const double t0[3], int detection, int handling,
                       const dcreg_config *, dcreg_iter_log *log, int log_capacity, dcreg_icp_result *);

/* The same loop with dcreg_linearize_voxels as its linearisation (dcreg_target_voxels_keep first, DCREG_E_STATE without it; with
 * "voxels_source_cov" = 1 kept source normals too; "voxels_neighbors" is read once when the call starts): one waited launch per iteration, the same aborts, fitness, convergence test, log
 * records, covariance and status codes, the same host step.  rmse is the RMS Mahalanobis distance per effective point, as for
 * dcreg_icp_run_gicp.  Of the configuration's linearisation parameters none is read.  One pose per call (many at once:
 * dcreg_icp_run_trials_voxels, dcreg_register_frames_voxels); no sharded / RCCL or Euler form of this engine. */
int dcreg_icp_run_voxels(dcreg_ctx *, const double R0[9], const double t0[3], int detection, int handling,
                         const dcreg_config *, dcreg_iter_log *log, int log_capacity, dcreg_icp_result *);

/* n independent scan pairs at once: one host thread per ctx (each ctx owns its clouds, index, stream), every thread runs
 * dcreg_icp_run.  One 100 k-point linearisation fills well under half of an MI355X and the device idles during each host
 * step, so independent pairs interleave: 4 pairs in flight give ~3.3x the one-pair iteration rate.  R0 = n x 9,
 * t0 = n x 3; results[i].status etc. as for dcreg_icp_run; returns the first non-OK code of any pair (all pairs still run
 * to completion).  Logs are not collected in this mode. */
int dcreg_icp_run_many(int n, dcreg_ctx *const *ctxs, const double *R0, const double *t0, int detection, int handling,
                       const dcreg_config *, dcreg_icp_result *results);

/* Point sharding of ONE scan pair over several devices: the ctx holds the whole target and THIS rank's slice
 * of the source; after every linearisation `reduce` must replace row[32] (21 H, 6 g, sum r^2, sum b^2, n_eff, n_pt, pad) by
 * the sum over all ranks, added in rank order so that every rank obtains bitwise the same totals (e.g. an all_gather over
 * RCCL + ordered sum; return 0 on success).  Every rank then takes the identical host step: no broadcast is needed.
 * n_source_total = points of the whole source cloud (fitness, :1856).  reduce == NULL: plain dcreg_icp_run. */
typedef int (*dcreg_reduce_fn)(double row[32], void *user);
int dcreg_icp_run_sharded(dcreg_ctx *, const double R0[9], const double t0[3], int detection, int handling,
                          const dcreg_config *, int64_t n_source_total, dcreg_reduce_fn reduce, void *reduce_user,
                          dcreg_iter_log *log, int log_capacity, dcreg_icp_result *);

/* The same with the exchange done natively: ONE ncclAllGather (RCCL over xGMI) of the 32-double rows per iteration on the
 * ctx's stream, rows added in rank order, inside the C++ engine loop (no callback).  Set-up: rank 0 obtains 128 opaque bytes
 * from dcreg_comm_unique_id and hands them to every rank by any means (the Python launcher broadcasts them with
 * torch.distributed); every rank then calls dcreg_comm_init(ctx, id, rank, world) - collectively, like ncclCommInitRank - and
 * dcreg_icp_run_sharded_rccl.  dcreg_comm_allgather_sum is the exchange step on its own.  RCCL is dlopen'ed on first use. */
int dcreg_comm_unique_id(void *id128);
int dcreg_comm_init(dcreg_ctx *, const void *id128, int rank, int world);
int dcreg_comm_destroy(dcreg_ctx *);
int dcreg_comm_allgather_sum(dcreg_ctx *, double row[32]);
int dcreg_icp_run_sharded_rccl(dcreg_ctx *, const double R0[9], const double t0[3], int detection, int handling,
                               const dcreg_config *, int64_t n_source_total, dcreg_iter_log *log, int log_capacity,
                               dcreg_icp_result *);

/* The second engine of the reference (selected by Config::use_so3_parameterization == false, icp_test_runner.cpp:443-458):
 * state = Pose6D {roll, pitch, yaw, x, y, z}, the Jacobian of :2299-2346 with the float-stored weighted normal and no weight
 * derivative - literally, coefficient permutation included (enum dcreg_parameterization above; dcreg_config::euler_exact_jacobian
 * selects the exact derivative instead) -, additive update (:2633-2638), convergence on |d rmse| < 1e-4 && |d fitness| < 1e-4
 * (:2679-2687), covariance mapped through the Euler->Lie Jacobian (:2695-2738).  pose6d = {roll, pitch, yaw, x, y, z};
 * final_pose6d receives the optimised pose (may be NULL).  The 6x6 analysis / handling step goes through the solver
 * seam above (the reference inlines a copy of it in this engine).  No committed trace of the reference exercises this
 * engine: parity is pinned on the shared correspondence steps only. */
int dcreg_icp_run_euler(dcreg_ctx *, const double pose6d[6], int detection, int handling, const dcreg_config *,
                        dcreg_iter_log *log, int log_capacity, dcreg_icp_result *, double final_pose6d[6]);

/* TestResult subset per trial (utils.hpp:253-303) */
typedef struct dcreg_trial_result {
    int converged, iterations, status;
    double time_ms;
    double trans_error_m, rot_error_deg;
    double final_rmse, final_fitness;
    int64_t corr_num;
    double final_transform[16];
    double H_upper[21];
    int degenerate_mask[6];
} dcreg_trial_result;

/* n_trials independent ICP runs of the same cloud pair from different initial poses (the num_runs loop of runMethod) as a
 * continuously refilled batch: up to 256 trials are in flight, every iteration of a group of them is ONE batched launch, and
 * a trial that ends hands its slot to the next one in line at once.  Each trial is bitwise the single run (dcreg_icp_run) of
 * its pose. */
int dcreg_icp_run_trials(dcreg_ctx *, int n_trials, const double *R0_9, const double *t0_3, int detection,
                         int handling, const dcreg_config *, dcreg_trial_result *results);

/* Many frames registered against the context's map in one call (placing a recorded drive on a prior map from odometry guesses,
 * multi-LiDAR rigs, loop-closure candidates, relocalisation): frame f = the points [frame_offsets[f], frame_offsets[f + 1]) of xyz
 * (HOST memory, all frames back to back, stride_floats floats per point, x y z first; frame_offsets holds n_frames + 1 entries, in
 * points, starting at 0), started from its own pose R0_9[9f..], t0_3[3f..].  The frames are uploaded in one copy and run as
 * dcreg_icp_run_trials runs trials - `slots` registrations in flight (0 = 256), every iteration of a group of them ONE batched launch in
 * which each pose reads its own frame - and results[f] is bitwise what dcreg_set_source(frame f) + dcreg_icp_run(R0, t0) give on this
 * context: final_transform, iterations, converged, status, final_rmse, final_fitness (of the frame's own point count), corr_num, H_upper
 * and degenerate_mask (time_ms: the call's time over the frames).  trans_error_m / rot_error_deg are taken against cfg->gt_matrix, as for
 * trials.  Like the other batched launches the frames search the whole map's index (never the window index of dcreg_roi_info: it is
 * invisible in the results).  An empty frame gets status 3 (as a trial with no source), the others run; n_frames == 0 does nothing.
 * DCREG_E_INVALID, and nothing runs: offsets that do not start at 0 or decrease, non-finite coordinates in any frame; DCREG_E_STATE: no
 * target.  The context's own source, its neighbour state and its reserved warm states are left as they were. */
int dcreg_register_frames(dcreg_ctx *, int n_frames, const float *xyz, const int64_t *frame_offsets, int64_t stride_floats,
                          const double *R0_9, const double *t0_3, int detection, int handling, const dcreg_config *, int slots,
                          dcreg_trial_result *results);

/* The same two calls for the second engine (dcreg_icp_run_normals: 1-NN rows against the map's kept normals).  Arguments, argument
 * rules, slots, record fields and amortised time_ms are those of dcreg_register_frames / dcreg_icp_run_trials: offsets start at 0 and do
 * not decrease, non-finite coordinates are refused (DCREG_E_INVALID, nothing runs), an empty frame gets status 3, n_frames == 0 /
 * n_trials == 0 does nothing, errors are taken against cfg->gt_matrix.  Every iteration of a group of registrations is ONE batched
 * launch (dcreg_debug.h: dcreg_normals_batch_begin) on the whole map's index, and results[f] is bitwise what dcreg_set_source(frame f) +
 * dcreg_icp_run_normals(R0 f, t0 f) give on a context with the same map, normals and options - final_transform, iterations, converged,
 * status (1: n_eff < 10, 2: a non-finite step), final_rmse, final_fitness (of the frame's own point count), corr_num, H_upper and
 * degenerate_mask; for trials, dcreg_icp_run_normals of the context's own source from each pose.  DCREG_E_STATE: no target, or no kept
 * normals (dcreg_target_normals_keep / _set first; every change of the map's points drops them) - results are then left untouched.  The
 * context's own source, the warm positions of dcreg_linearize_normals, the first engine's own and reserved states, the window index and
 * the kept normals are left as they were (dcreg_register_frames_normals replaces the frames a dcreg_register_frames call left on the
 * device, and the other way round).  Not available for this engine: the sharded / RCCL forms, the Euler form. */
int dcreg_register_frames_normals(dcreg_ctx *, int n_frames, const float *xyz, const int64_t *frame_offsets, int64_t stride_floats,
                                  const double *R0_9, const double *t0_3, int detection, int handling, const dcreg_config *, int slots,
                                  dcreg_trial_result *results);
int dcreg_icp_run_trials_normals(dcreg_ctx *, int n_trials, const double *R0_9, const double *t0_3, int detection, int handling,
                                 const dcreg_config *, dcreg_trial_result *results);

/* ... and for the third engine (dcreg_icp_run_gicp: plane-to-plane rows from the map's kept normals and each frame's own).  Arguments,
 * argument rules, slots, record fields and amortised time_ms as above.  frame_normals: the rule every frame's own normals are estimated
 * with - all frames in one batched pass (dcreg_normals_clouds' build and kernel over the loaded frames), kept beside the frames' points
 * for the call; its refusals are those of dcreg_normals (DCREG_E_INVALID, before anything is queued).  Every iteration of a group of
 * registrations is ONE batched launch (dcreg_debug.h: dcreg_gicp_batch_begin), and results[f] is bitwise what dcreg_set_source(frame f) +
 * dcreg_source_normals_keep(frame_normals) + dcreg_icp_run_gicp(R0 f, t0 f) give on a context with the same map, kept map normals and
 * options ("gicp_epsilon" among them); for trials, dcreg_icp_run_gicp of the context's own source and its kept source normals from each
 * pose.  An empty frame gets status 3; a frame with fewer than k points runs and ends with status 1 (none of its points has a normal:
 * n_eff = 0).  DCREG_E_STATE: no target, no kept map normals, or - the trials form - no kept source normals; results are then left
 * untouched.  The context's own source and its kept normals, the warm positions of the single-pose 1-NN launches, the first engine's
 * states, the window index and the map's kept normals are left as they were. */
int dcreg_register_frames_gicp(dcreg_ctx *, int n_frames, const float *xyz, const int64_t *frame_offsets, int64_t stride_floats,
                               const dcreg_normal_params *frame_normals, const double *R0_9, const double *t0_3, int detection,
                               int handling, const dcreg_config *, int slots, dcreg_trial_result *results);
int dcreg_icp_run_trials_gicp(dcreg_ctx *, int n_trials, const double *R0_9, const double *t0_3, int detection, int handling,
                              const dcreg_config *, dcreg_trial_result *results);

/* ... and for the fourth engine (dcreg_icp_run_voxels: rows against the map's kept voxel distributions - the cheap stage with the wide
 * basin, for many candidates at once: relocalisation hypotheses, loop-closure candidates, a recorded drive on a prior map, Monte-Carlo
 * starts).  Arguments, argument rules, slots, record fields and amortised time_ms are those of dcreg_register_frames /
 * dcreg_icp_run_trials: offsets start at 0 and do not decrease, stride_floats >= 3, non-finite coordinates are refused (DCREG_E_INVALID,
 * nothing runs), an empty frame gets status 3, n_frames == 0 / n_trials == 0 does nothing, errors are taken against cfg->gt_matrix.
 * Every iteration of a group of registrations is ONE batched launch (dcreg_debug.h: dcreg_voxels_batch_begin), and results[f] is bitwise
 * what dcreg_set_source(frame f) [+ dcreg_source_normals_keep(frame_normals) in mode 1] + dcreg_icp_run_voxels(R0 f, t0 f) give on a
 * context with the same map, kept voxels and options - final_transform, iterations, converged, status (1: n_eff < 10, 2: a non-finite
 * step), final_rmse, final_fitness (of the frame's own point count), corr_num, H_upper and degenerate_mask; for trials,
 * dcreg_icp_run_voxels of the context's own source from each pose.  A frame with fewer than 10 effective points (points that fall into a kept
 * voxel) ends with status 1.
 * "voxels_source_cov" and "voxels_neighbors" are read once when the call starts.  Mode 0: frame_normals is not read and may be NULL, no normals pass runs, and
 * the map needs no kept normals.  Mode 1, frames form: frame_normals is checked as dcreg_register_frames_gicp checks it (DCREG_E_INVALID,
 * before the empty call returns), and all frames' normals are then estimated in one batched pass behind the load
 * (dcreg_frames_normals_keep); a frame with fewer than k points has no normals and ends with status 1.  Mode 1, trials form: no kept
 * source normals is DCREG_E_STATE.  "gicp_epsilon", "robust_kernel" and "gicp_robust_scale" are read at every launch, as by the
 * single-pose call.
 * DCREG_E_STATE, results untouched: no target, no kept voxels (dcreg_target_voxels_keep first; every change of the map's points drops
 * them), a linearisation in flight.  The context's own source and its kept normals, every warm and neighbour state of the other engines,
 * the window index, the map's kept normals and the kept voxels are left as they were (the frames form replaces the frames a previous
 * dcreg_register_frames* call left on the device, and their kept normals, as between the other engines).  Scan pairs, each against
 * a voxel map of its own target: dcreg_register_pairs_voxels below.  Not provided: the sharded / RCCL forms, the Euler form. */
int dcreg_register_frames_voxels(dcreg_ctx *, int n_frames, const float *xyz, const int64_t *frame_offsets, int64_t stride_floats,
                                 const dcreg_normal_params *frame_normals, const double *R0_9, const double *t0_3, int detection,
                                 int handling, const dcreg_config *, int slots, dcreg_trial_result *results);
int dcreg_icp_run_trials_voxels(dcreg_ctx *, int n_trials, const double *R0_9, const double *t0_3, int detection, int handling,
                                const dcreg_config *, dcreg_trial_result *results);

/* Many scan pairs registered in one call, each against a target of its own (loop-closure candidates against their submaps, scan-to-scan
 * odometry of a recorded drive, multi-session alignment, accuracy evaluation over a dataset of pairs): pair p = source points
 * [src_offsets[p], src_offsets[p + 1]) of src_xyz against target points [tgt_offsets[p], tgt_offsets[p + 1]) of tgt_xyz, started from
 * R0_9[9p..], t0_3[3p..].  Both buffers in HOST memory, clouds back to back, stride_floats floats per point (x y z first); each offset
 * array holds n_pairs + 1 entries, in points, starting at 0.  The targets are indexed in build batches (option "pairs_max_bytes"; their
 * cell tables budgeted per target by "pair_max_table_entries"), every batch with one upload, one bounds pass and a fixed number of sorts
 * and synchronises whatever its size, for the radius cfg->search_radius; the pairs of a batch then run as dcreg_register_frames runs
 * frames, each pose reading its own source and its own target.  results[p] is bitwise what a context with the same options gives for
 * dcreg_set_target(target p, cfg->search_radius) + dcreg_set_source(source p) + dcreg_icp_run(R0 p, t0 p) - the fields
 * dcreg_register_frames promises, errors against cfg->gt_matrix.  An empty source or target: status 3, the other pairs run; n_pairs == 0
 * does nothing.  DCREG_E_INVALID, and nothing runs: offsets that do not start at 0 or decrease, non-finite coordinates in any cloud;
 * DCREG_E_STATE: a linearisation in flight.  Needs no target on the context, and leaves its target, source, neighbour states, reserved
 * warm states, frames and window index as they were. */
int dcreg_register_pairs(dcreg_ctx *, int n_pairs, const float *src_xyz, const int64_t *src_offsets, const float *tgt_xyz,
                         const int64_t *tgt_offsets, int64_t stride_floats, const double *R0_9, const double *t0_3, int detection,
                         int handling, const dcreg_config *, int slots, dcreg_trial_result *results);

/* dcreg_register_pairs for the second engine (dcreg_icp_run_normals: 1-NN rows against kept normals) and the third (dcreg_icp_run_gicp:
 * plane-to-plane rows).  Arguments, offset rules, build batches ("pairs_max_bytes", "pair_max_table_entries"; a batch is counted with 32
 * more bytes per target point: its kept normals and the scratch of their estimation), slots, record fields and amortised time_ms are
 * those of dcreg_register_pairs.  target_normals: the rule every target's normals are estimated with, all targets of a build batch in ONE
 * launch over the grids the batch already has, kept beside them for the batch; source_normals (the GICP form): the rule of the sources'
 * own normals, estimated once per call for all sources in one batched pass.  Every iteration of a group of pairs is ONE batched launch
 * (dcreg_debug.h: dcreg_pairs_normals_batch_begin / dcreg_pairs_gicp_batch_begin), each pose reading its own source, its own target and
 * that target's normals.  results[p] is bitwise what a context with the same options ("gicp_epsilon" among them, read as the single call
 * reads it) gives for dcreg_set_target(target p, cfg->search_radius) + dcreg_target_normals_keep(target_normals) + dcreg_set_source(source
 * p) [+ dcreg_source_normals_keep(source_normals)] + dcreg_icp_run_normals / dcreg_icp_run_gicp(R0 p, t0 p): final_transform, iterations,
 * converged, status, final_rmse, final_fitness, corr_num, H_upper and degenerate_mask; errors against cfg->gt_matrix.  An empty source or
 * target: status 3, the other pairs run; n_pairs == 0 does nothing.  A target with fewer than k points has no normals (all NaN), and so
 * has, in the GICP form, a source with fewer than k points: the pair runs - as the serial sequence does - and ends after one launch with
 * status 1, iterations 1 and n_eff = 0.  DCREG_E_INVALID, before anything is queued: the refusals of dcreg_register_pairs, and those of
 * dcreg_normals for either parameter block (checked before the n_pairs == 0 return); DCREG_E_STATE: a linearisation or a batched 1-NN
 * launch in flight.  The calls need no target on the context and leave alone its target, kept map normals, source, kept source normals,
 * the warm positions of the single-pose 1-NN launches, the first engine's states and reserved warm states, the loaded frames with their
 * kept normals and the window index; they replace the pairs' sources a dcreg_register_pairs* call left on the device, and size the warm
 * slots of the batched 1-NN launches (dcreg_debug.h: dcreg_normals_reserve_slots) for their own sources, as dcreg_register_frames_normals does for its frames. */
int dcreg_register_pairs_normals(dcreg_ctx *, int n_pairs, const float *src_xyz, const int64_t *src_offsets, const float *tgt_xyz,
                                 const int64_t *tgt_offsets, int64_t stride_floats, const dcreg_normal_params *target_normals,
                                 const double *R0_9, const double *t0_3, int detection, int handling, const dcreg_config *, int slots,
                                 dcreg_trial_result *results);
int dcreg_register_pairs_gicp(dcreg_ctx *, int n_pairs, const float *src_xyz, const int64_t *src_offsets, const float *tgt_xyz,
                              const int64_t *tgt_offsets, int64_t stride_floats, const dcreg_normal_params *target_normals,
                              const dcreg_normal_params *source_normals, const double *R0_9, const double *t0_3, int detection,
                              int handling, const dcreg_config *, int slots, dcreg_trial_result *results);

/* dcreg_register_pairs for the fourth engine (dcreg_icp_run_voxels: rows against per-voxel Gaussians): the cheap stage with the wide
 * basin for many candidates at once, each against its own submap - loop-closure and relocalisation candidates from the place search,
 * whose starts may lie outside the 1-NN engines' search radius.  Arguments, offset rules, build batches under "pairs_max_bytes", slots,
 * record fields and amortised time_ms are those of dcreg_register_pairs.  The engine needs no index on the target side: a build batch
 * uploads and packs its targets and keeps ONE voxel map per target by the rule target_voxels, all maps of the batch in one pass (one
 * sort - two where target and voxel bits exceed 64 -, a fixed number of launches and synchronises whatever the number of targets); no
 * cell table, no adaptation pass and no normals pass runs, and a batch is counted with what this build allocates (dcreg_debug.h:
 * dcreg_pairs_plan_voxels), "pair_max_table_entries" is not read.  Every iteration of a group of pairs is ONE batched launch
 * (dcreg_debug.h: dcreg_pairs_voxels_batch_begin), each pose reading its own source and its own target's voxel map.
 * results[p] is bitwise what a context with the same options gives for dcreg_set_target(target p, any radius) +
 * dcreg_target_voxels_keep(target_voxels) + dcreg_set_source(source p) [+ dcreg_source_normals_keep(source_normals) in mode 1] +
 * dcreg_icp_run_voxels(R0 p, t0 p): final_transform, iterations, converged, status, final_rmse, final_fitness, corr_num, H_upper and
 * degenerate_mask; errors against cfg->gt_matrix.  cfg->search_radius is not read by this engine.
 * "voxels_source_cov" and "voxels_neighbors" are read once when the call starts; "gicp_epsilon", "robust_kernel" and "gicp_robust_scale" at every launch, as in
 * the frames form.  Mode 0: source_normals is not read and may be NULL, no normals pass runs.  Mode 1: source_normals is checked as
 * dcreg_register_pairs_gicp checks it, and all sources' normals are estimated once per call in one batched pass; a source with fewer
 * than k points has no normals and ends with status 1.
 * An empty source or target: status 3, the other pairs run.  A target that keeps no voxel (every voxel below min_points or degenerate)
 * also gives status 3 - the one departure from the serial sequence, where dcreg_icp_run_voxels refuses with DCREG_E_STATE.  n_pairs == 0
 * does nothing, after the parameter checks.
 * DCREG_E_INVALID, nothing runs, results untouched: the refusals of dcreg_register_pairs; those of dcreg_target_voxels_keep for
 * target_voxels (a leaf that is not finite and > 0, epsilon outside [1e-6, 1], min_points < 2, a null block) and, in mode 1, those of
 * dcreg_normals for source_normals, both checked before the n_pairs == 0 return; any target, in any build batch, that spans 2^21 or more
 * voxels on an axis or has a voxel coordinate of magnitude 2^62 or more (the targets of later batches are checked on the host from their
 * coordinate-wise bounds, the first batch's by its own build, before any pair runs).  DCREG_E_STATE: a linearisation or a batched launch
 * in flight.
 * The call needs no target on the context and leaves alone its target, kept voxels, kept normals, source, kept source normals, every
 * warm and neighbour state, the loaded frames with their normals and the window index; it replaces the pairs' sources (and their kept
 * normals) a previous dcreg_register_pairs* call left on the device and the voxel batch of a previous call of its own. */
int dcreg_register_pairs_voxels(dcreg_ctx *, int n_pairs, const float *src_xyz, const int64_t *src_offsets, const float *tgt_xyz,
                                const int64_t *tgt_offsets, int64_t stride_floats, const dcreg_voxel_map_params *target_voxels,
                                const dcreg_normal_params *source_normals, const double *R0_9, const double *t0_3, int detection,
                                int handling, const dcreg_config *, int slots, dcreg_trial_result *results);

/* Initial pose of Monte-Carlo trial k (the reference has no RNG: its num_runs loop, icp_test_runner.cpp:339-349, repeats one
 * deterministic run; the seeded perturbation is this build's definition, shared by the runner and dcreg_amd/montecarlo.py):
 * k == 0 -> the base pose; k >= 1 -> base + U(-amp, amp) per degree of freedom from MT19937(low 32 bits of seed + k),
 * 53-bit doubles, drawn in the order x y z roll pitch yaw.  base = {x, y, z [m], roll, pitch, yaw [rad]}; T row-major 4x4
 * = Pose6D2Matrix (utils.hpp:452-460); pose_xyzrpy (may be NULL) receives the perturbed six numbers. */
int dcreg_trial_pose(const double base_xyzrpy[6], uint64_t seed, int64_t k, double trans_amp, double rot_amp_rad, double T[16],
                     double pose_xyzrpy[6]);

/* The Monte-Carlo experiment of one rank: trials k = first_trial + j * trial_stride, j = 0 .. n_trials - 1 (rank r of w: first_trial
 * = r, stride = w), initial poses from dcreg_trial_pose, run as dcreg_icp_run_trials does with `slots` trials in flight (0 = 256).
 * results[j] belongs to trial first_trial + j * trial_stride. */
int dcreg_icp_run_montecarlo(dcreg_ctx *, const double base_xyzrpy[6], uint64_t seed, int64_t first_trial, int64_t trial_stride,
                             int64_t n_trials, double trans_amp, double rot_amp_rad, int detection, int handling,
                             const dcreg_config *, int slots, dcreg_trial_result *results);

/* The Monte-Carlo experiment (BASELINE configs[4]; runMethod's num_runs loop + updateStatistics / finalizeStatistics,
 * icp_test_runner.cpp:331-390, 604-664) as ONE job over the ranks of the ctx's communicator (dcreg_comm_init; without one: a job of one
 * rank): this rank runs trials k = rank, rank + world, ... (dcreg_icp_run_montecarlo), the fixed-size trial records of all ranks are
 * gathered with ONE ncclAllGather (RCCL over xGMI) on the ctx's stream, and EVERY rank receives all n_trials records ordered by trial
 * and the method's statistics - no host-side collective, no Python.  A record is DCREG_TRIAL_RECORD_DOUBLES doubles:
 *   [0] converged [1] iterations [2] time_ms [3] trans_error_m [4] rot_error_deg [5] final_rmse [6] final_fitness [7] corr_num
 *   [8] status [9] trial index [10..25] final transform, row-major [26..46] last Hessian, upper triangle [47..52] degenerate mask.
 * records: [n_trials * DCREG_TRIAL_RECORD_DOUBLES] or NULL; stats may be NULL. */
#define DCREG_TRIAL_RECORD_DOUBLES 64
typedef struct dcreg_method_stats {        /* MethodStatistics, utils.hpp:305-330 */
    int64_t total_runs, converged_runs;
    double success_rate;
    double mean_trans_error, std_trans_error, min_trans_error, max_trans_error;     /* population std (:660-662) */
    double mean_rot_error, std_rot_error, min_rot_error, max_rot_error;
    double mean_time_ms, std_time_ms;
    double mean_iterations, mean_rmse, mean_fitness;
    int64_t corr_num;              /* correspondences of all final iterations */
    int64_t iterations_total;      /* ICP iterations of all trials */
    int ranks_seen;                /* ranks that contributed at least one record (= the communicator's size when every rank did) */
    int world;
} dcreg_method_stats;
int dcreg_montecarlo_job(dcreg_ctx *, const double base_xyzrpy[6], uint64_t seed, int64_t n_trials, double trans_amp, double rot_amp_rad,
                         int detection, int handling, const dcreg_config *, int slots, double *records, dcreg_method_stats *stats);
/* the gather on its own: count doubles of this rank -> recv[world * count], rank-major, on every rank; rank / size of the communicator */
int dcreg_comm_allgather(dcreg_ctx *, const double *send, double *recv, int64_t count);
int dcreg_comm_info(const dcreg_ctx *, int *rank, int *world);

/* host threads the batched engines may use for the per-trial 6x6 steps (OpenMP; the reference hard-codes 8, :1714).  Launchers
 * that pin OMP_NUM_THREADS=1 (torch.distributed.run) should set this to the CPUs the rank really owns.  Whatever is set, the engines
 * never use more threads than the process can keep busy - min(affinity mask, cgroup CPU quota): OpenMP's default inside a container is
 * the machine's hardware thread count. */
int dcreg_set_host_threads(int n);
int dcreg_get_host_threads(void);

/* calculatePointToPointError (utils.hpp:538-589): aligned = T * source (float), both directions on the GPU.
 *   T       row-major 4x4; the bottom row is ignored (the reference's affine transform ignores it).  T must be a RIGID motion: a non-finite
 *           entry in its top three rows, or a rotation block that is not a rotation (an element of |R^T R - I| above 1e-6, or det(R) <= 0 -
 *           the rule of the deskew calls), is refused with DCREG_E_INVALID before anything is queued.  No source or no target: DCREG_E_STATE.
 *   forward (rmse, fitness, valid, and the forward half of chamfer): every T * p (double arithmetic, float store) against the map, as the
 *           reference does it - valid and fitness are the reference's exactly, rmse and the forward mean are double sums of the same float
 *           terms in another order.  A point counts as valid when (double)sqrtf(d2) < error_threshold, strictly: a threshold <= 0 counts
 *           none (rmse = fitness = 0), +inf counts all.
 *   backward (the other half of chamfer): the reference builds a second tree over the aligned cloud.  Here the map points are moved by
 *           T^-1 = (R^T, -R^T t) into the body frame and searched in a grid over the source - the same nearest neighbours because a rigid
 *           motion preserves distances; that is why T must be one.  The two differ only in where the float rounding happens (T^-1 q in
 *           the body frame here, T p in the map frame there).  A nearest-neighbour distance is 1-Lipschitz in either point set, so against
 *           the mean taken in exact arithmetic
 *               |backward mean here - exact|      <= sqrt(3) * 2^-24 * B + 2^-21 * mean,
 *               |backward mean reference - exact| <= sqrt(3) * 2^-24 * G + 2^-21 * mean,
 *           with B (G) the largest absolute body-frame (map-frame) coordinate among the moved points and the cloud they are searched in;
 *           the second term covers the float d2 arithmetic and sqrtf.  chamfer differs from the reference by at most half the sum of the
 *           two.  (A rotation block at the edge of the 1e-6 rule adds up to 1e-6 * the distances involved.)
 *   Results are deterministic: the same clouds and T give the same bits. */
int dcreg_p2p_error(dcreg_ctx *, const double T[16], double error_threshold, double *rmse, double *fitness,
                    double *chamfer, int64_t *valid_correspondences);

/* ---------------- FPFH descriptors and feature-space matching ----------------
 * The first two stages of a correspondence-based global alignment (PCL FPFHEstimation with setKSearch + a nearest-neighbour search in
 * feature space; Open3D compute_fpfh_feature + correspondences): 33 floats per point, and for every row of one descriptor set its best
 * and second-best row of another.  The pose from the correspondences (RANSAC, a graph method) is the caller's.  Both rules are fixed
 * tightly enough that the output is bitwise the numpy reference of tests/fpfh_ref.py, with ONE freedom, stated below (atan2).
 *
 * The descriptor rule.  For a cloud of n points, one normal per point (3 floats, normals_stride floats apart) and the parameters k
 * (3 .. 32, the point itself among the neighbours) and search_radius (>= 0, 0 = unbounded):
 *   - used points: a point is used when its three coordinates AND its three normal components are all finite.  Unused points are neither
 *     queries nor candidates and get NaN in all 33 outputs;
 *   - neighbours: candidates are ranked by (d2, input index) with dcreg_knn's float d2; the neighbours of a point are the first k used
 *     points with d2 < bound, bound = min((float)(search_radius^2), 3.0e38f) for search_radius > 0 and 3.0e38f for search_radius = 0 (the
 *     normals' bound).  A point with fewer than k candidates inside the bound keeps the m it has, 1 <= m <= k (unlike the normals this is
 *     not sparse-or-nothing);
 *   - pair features: for the point p and each neighbour q with d2 > 0, in rank order, everything in double, every operation rounded
 *     once, a dot product evaluated as (x + y) + z:
 *       d = q - p; f4 = sqrt(d.d); a pair with f4 == 0 is skipped;
 *       a1 = (n_p.d) / f4; a2 = (n_q.d) / f4;
 *       if |a1| < |a2|: n1 = n_q, n2 = n_p, d = -d, phi = -a2; otherwise n1 = n_p, n2 = n_q, phi = a1;
 *       v = d x n1; vn = sqrt(v.v); a pair with vn == 0 is skipped; v = v / vn per coordinate;
 *       w = n1 x v; alpha = v.n2; theta = atan2(w.n2, n1.n2);
 *   - bins, each min(max(floor(.), 0), 10): of t = 11 * ((theta + pi) / (2 * pi)), of 11 * ((alpha + 1) * 0.5), of 11 * ((phi + 1) * 0.5);
 *   - SPFH: c[33] integer counts, theta in 0 .. 10, alpha in 11 .. 21, phi in 22 .. 32; as a double s_b = (double)c_b * (100.0 /
 *     (double)(m - 1)).  A point with m < 2 or with no counted pair has no SPFH;
 *   - FPFH: F_b = sum_j (1.0 / (double)d2_j) * s_b(q_j) over the neighbours in rank order, skipping every j with d2_j == 0 and every j
 *     whose q_j has no SPFH; summed left to right, starting from the first term;
 *   - normalisation, each block of 11 on its own: S = the block's sum, left to right; out_b = (float)(F_b * (100.0 / S)).  A point whose
 *     three S are not all > 0 is EMPTY: NaN in all 33 outputs, counted in n_empty;
 *   - info: n_in, n_used, n_empty and n_out = n_used - n_empty.
 * A point's result depends on the cloud, the normals and the parameters only - never on the index, the launch or the context's other
 * state.  The ONE operation that is not bit-reproducible between numpy and the device is atan2: it matters only where t falls within
 * rounding of an interior bin edge of theta (t = 1 .. 10; the clamped outer edges are harmless), and there the device's bin may be
 * either neighbour's.  Everything else is bitwise; the reference flags the points with such a pair ("edge-near": |t - round(t)| < 1e-9).
 * The descriptor changes when a normal flips its sign: orient the normals of clouds that are to be matched consistently.
 *
 * dcreg_fpfh reads one cloud as dcreg_normals reads it.  normals == NULL: the call estimates them first with normal_params (the rule
 * of dcreg_normals, bitwise) on the same per-cloud index - a sparse point has no normal and is then unused - and returns them in
 * normals_out (3 n floats) when that is not NULL; the cloud is indexed a second time only when some finite point got no normal.  With
 * normals given, normal_params and normals_out are ignored and may be NULL.  dcreg_target_fpfh computes the resident map's descriptors
 * in index order (dcreg_target_get) from the kept normals of dcreg_target_normals_keep / _set through the map's own index (a map whose
 * kept normals are not all finite is indexed once more without those points).  fpfh_out holds 33 n floats (33 capacity_points).
 * Neither call changes the target, the source, warm states, kept normals, places or keyframes; both wait for the stream; repeated
 * calls and calls on another context are bitwise equal.
 * DCREG_E_INVALID, before anything is queued: null context or parameters, k outside 3 .. 32, a search_radius that is not finite or is
 * negative, stride < 3, normals_stride < 3, n < 0, more than 2^31 - 1 points, a null cloud with n > 0, a null output, both normals and
 * normal_params NULL, the refusals of dcreg_normals for normal_params when it is read, a capacity below the map's size.  DCREG_E_STATE:
 * a linearisation in flight; no target or no kept normals (the map form).  Device memory: the outlier filter's scratch for the cloud
 * and its index (the cloud form), 8 k bytes per point for the neighbour lists (position and d2), 48 bytes per point for the counts and
 * 132 for the output - kept as scratch of the context, as the outlier pass's, and reused by the next call.  A refused call zeroes *info. */
typedef struct dcreg_fpfh_params {
    int k;                 /* neighbours per point, the point itself among them (PCL setKSearch), 3 .. 32 */
    int reserved0_;
    double search_radius;  /* 0 = unbounded, > 0 = neighbours beyond it do not count (m) */
    double reserved_[2];
} dcreg_fpfh_params;
typedef struct dcreg_fpfh_info {
    int64_t n_in;        /* points passed in / points of the map */
    int64_t n_used;      /* ... with finite coordinates and a finite normal */
    int64_t n_empty;     /* ... of those, without a descriptor (a block's sum is not > 0) */
    int64_t n_out;       /* points that received a descriptor */
} dcreg_fpfh_info;
#define DCREG_FPFH_DIM 33
/* k = 16, search_radius = 0 */
int dcreg_default_fpfh_params(dcreg_fpfh_params *);
int dcreg_fpfh(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const float *normals, int64_t normals_stride_floats,
               const dcreg_normal_params *, const dcreg_fpfh_params *, float *fpfh_out, float *normals_out, dcreg_fpfh_info *info);
int dcreg_fpfh_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const float *d_normals, int64_t normals_stride_floats,
                      const dcreg_normal_params *, const dcreg_fpfh_params *, float *d_fpfh_out, float *d_normals_out, dcreg_fpfh_info *info);
int dcreg_target_fpfh(dcreg_ctx *, const dcreg_fpfh_params *, float *fpfh_out, int64_t capacity_points, dcreg_fpfh_info *info);
int dcreg_target_fpfh_device(dcreg_ctx *, const dcreg_fpfh_params *, float *d_fpfh_out, int64_t capacity_points, dcreg_fpfh_info *info);

/* ---------------- FPFH over a radius support ----------------
 * The same descriptor with PCL's other neighbourhood (FPFHEstimation with setRadiusSearch): EVERY used point within `radius` is a
 * neighbour, a few hundred per point at the usual five leaves.  With m unbounded there is no rank-ordered list to sum over, so both
 * sums of this rule are INTEGERS: no order of summation is part of it, and the output is bitwise the numpy reference of
 * tests/fpfh_radius_ref.py with the one freedom of the rule above (atan2 at an interior bin edge of theta, the same "edge-near" flags).
 * Unchanged from the rule above: the used points, dcreg_knn's float d2 = (dx*dx + dy*dy) + dz*dz with every operation rounded to float,
 * the pair features in double and the three bins.  Parameters: radius, finite and > 0, with R2 = (float)(radius * radius) > 0 and
 * < 3.0e38f; max_neighbors in 2 .. 65535.
 *   1. neighbours of a used point i: every used point j with d2_ij < R2 (strict), the point itself and exact duplicates included;
 *      m_i is their number;
 *   2. a point with m_i > max_neighbors is CROWDED: it has no SPFH and it is EMPTY, counted in n_crowded as well as in n_empty (its
 *      walk stops where the count passes the cap: it is reported with m = max_neighbors + 1);
 *   3. counts: for every neighbour with d2 > 0 the pair features and bins of the rule above; pairs with f4 == 0 or vn == 0 are skipped;
 *      c_b(i), b = 0 .. 32, are integer counts;
 *   4. a point has an SPFH when 2 <= m_i <= max_neighbors and at least one pair was counted;
 *   5. quantised SPFH: q_b(i) = (c_b(i) << 16) / (m_i - 1), integer floor.  c_b <= m - 1, so q_b <= 65536 and each block of 11 sums to
 *      at most 65536;
 *   6. weight: w_ij = min((uint64) floor(((double)R2 / (double)d2_ij) * 16384.0), 2^30) - one IEEE double division, a multiply by a
 *      power of two; 16384 <= w <= 2^30, and pairs closer than radius / 256 share the clamped weight;
 *   7. FPFH: F_b(i) = sum of w_ij * q_b(j) over the neighbours j with d2_ij > 0 and an SPFH, in uint64.  F_b <= m * 2^30 * 2^16 <=
 *      65535 * 2^46 < 2^62, and a block's sum S_t has the same bound because a block of q sums to at most 65536: nothing wraps.
 *      That bound is why max_neighbors ends at 65535;
 *   8. normalisation: out_b = (float)((double)F_b * (100.0 / (double)S_t)), uint64 to double rounding to nearest even.  A point with
 *      any S_t == 0 is EMPTY: NaN in all 33 outputs;
 *   9. info: n_in, n_used, n_empty, n_crowded, n_out = n_used - n_empty, m_max and m_sum = the maximum and the sum of m over the used
 *      points (a crowded point with max_neighbors + 1).  m_sum / n_used is what a caller tunes the radius by.
 * The calls take the arguments of dcreg_fpfh / dcreg_target_fpfh with this parameter block and follow their text above: normals == NULL
 * estimates them with normal_params under the k-rule of dcreg_normals, the map form reads the kept normals through the map's own index
 * (whole or window), nothing else in the context changes, both wait for the stream, repeated calls and other contexts give the same bits.
 * DCREG_E_INVALID, before anything is queued: null context or parameters, a radius that is not finite or not > 0 or whose R2 leaves
 * (0, 3.0e38), max_neighbors outside 2 .. 65535, stride < 3, normals_stride < 3, n < 0, more than 2^31 - 1 points, a null cloud with
 * n > 0, a null output, both normals and normal_params NULL, the refusals of dcreg_normals for normal_params when it is read, a capacity
 * below the map's size.  DCREG_E_STATE: a linearisation in flight; no target or no kept normals (the map form).  Device memory does not
 * depend on the radius: the outlier filter's scratch for the cloud and its index (the cloud form), 276 bytes per used point for the
 * quantised SPFH and the counts, 132 per point for the output - kept as scratch of the context and reused by the next call. */
typedef struct dcreg_fpfh_radius_params {
    double radius;         /* the support: neighbours are the used points with d2 < (float)(radius * radius) (PCL setRadiusSearch) */
    int max_neighbors;     /* a point with more neighbours is crowded and gets no descriptor, 2 .. 65535 */
    int reserved0_;
    double reserved_[2];
} dcreg_fpfh_radius_params;
typedef struct dcreg_fpfh_radius_info {
    int64_t n_in;        /* points passed in / points of the map */
    int64_t n_used;      /* ... with finite coordinates and a finite normal */
    int64_t n_empty;     /* ... of those, without a descriptor (crowded, or a block's sum is 0) */
    int64_t n_crowded;   /* ... of those, with more than max_neighbors neighbours */
    int64_t n_out;       /* points that received a descriptor */
    int64_t m_max;       /* the largest m of a used point */
    int64_t m_sum;       /* the sum of m over the used points */
    int64_t reserved_;
} dcreg_fpfh_radius_info;
/* radius = 1.0, max_neighbors = 65535 */
int dcreg_default_fpfh_radius_params(dcreg_fpfh_radius_params *);
int dcreg_fpfh_radius(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const float *normals, int64_t normals_stride_floats,
                      const dcreg_normal_params *, const dcreg_fpfh_radius_params *, float *fpfh_out, float *normals_out,
                      dcreg_fpfh_radius_info *info);
int dcreg_fpfh_radius_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const float *d_normals,
                             int64_t normals_stride_floats, const dcreg_normal_params *, const dcreg_fpfh_radius_params *, float *d_fpfh_out,
                             float *d_normals_out, dcreg_fpfh_radius_info *info);
int dcreg_target_fpfh_radius(dcreg_ctx *, const dcreg_fpfh_radius_params *, float *fpfh_out, int64_t capacity_points, dcreg_fpfh_radius_info *info);
int dcreg_target_fpfh_radius_device(dcreg_ctx *, const dcreg_fpfh_radius_params *, float *d_fpfh_out, int64_t capacity_points,
                                    dcreg_fpfh_radius_info *info);

/* The matching rule.  a: n_a rows, b: n_b rows, 33 floats each, stride_a / stride_b floats apart (>= 33):
 *   - a row with any non-finite value is neither a query nor a candidate; as a query it returns index -1 and NaN distances;
 *   - D(i, j) = sum_{c = 0 .. 32} ((double)a_ic - (double)b_jc)^2, left to right, the multiply and the add rounded separately;
 *   - candidates are ranked by (D, j); idx_out / d_out (n_a int32 / n_a doubles) receive the best, idx2_out / d2nd_out the second-best
 *     (either pair may be NULL); with fewer than two valid candidates the missing places get -1 and +inf;
 *   - mutual_out (n_a bytes, may be NULL): 1 when the best row of a for b[idx_i], under the same rule with the roles swapped, is i;
 *   - info: n_a_valid, n_b_valid, n_mutual (0 when mutual_out is NULL).
 * Every distance is computed in the order above whatever the launch: the result does not depend on how the candidates are split over
 * blocks ("feature_match_split": rows of b per block column, 0 = chosen from the sizes; a test option).  No ratio test and no distance
 * filter: the caller has both distances.  n_a == 0 does nothing; n_b == 0 returns -1 / +inf for every valid query.
 * DCREG_E_INVALID, before anything is queued: null context, null a with n_a > 0, null b with n_b > 0, null idx_out or d_out, a stride
 * below 33, a negative count or more than 2^31 - 1 rows; DCREG_E_STATE: a linearisation in flight.  Touches nothing else in the context.
 * Device memory: both descriptor sets (the host form), 24 bytes per query and candidate split, and the results. */
typedef struct dcreg_match_info {
    int64_t n_a_valid, n_b_valid, n_mutual;
    int64_t reserved_;
} dcreg_match_info;
int dcreg_feature_match(dcreg_ctx *, const float *a, int64_t n_a, int64_t stride_a, const float *b, int64_t n_b, int64_t stride_b,
                        int32_t *idx_out, double *d_out, int32_t *idx2_out, double *d2nd_out, uint8_t *mutual_out, dcreg_match_info *info);
int dcreg_feature_match_device(dcreg_ctx *, const float *d_a, int64_t n_a, int64_t stride_a, const float *d_b, int64_t n_b, int64_t stride_b,
                               int32_t *d_idx_out, double *d_d_out, int32_t *d_idx2_out, double *d_d2nd_out, uint8_t *d_mutual_out,
                               dcreg_match_info *info);

/* ---------------- Pose from correspondences ----------------
 * The stage behind dcreg_feature_match: from point pairs (a[corr_a[m]], b[corr_b[m]]), most of them wrong, the rigid pose q ~ R p + t
 * that most of them agree on, by seeded RANSAC over three-pair hypotheses (Open3D registration_ransac_based_on_correspondence, PCL
 * SampleConsensusPrerejective without its verification against the cloud).  The call knows nothing of descriptors: two clouds and two
 * index arrays.  The best n_best hypotheses come back as 4x4 poses that every T0 / T0s argument of the engines takes as they are.
 * Everything is in double, every operation is rounded once, a dot product is (x + y) + z, and no operation of the rule is a library
 * function whose last bit is free: the output is BITWISE the numpy reference of tests/align_ref.py, with no stated freedom.
 *
 * 1. Used pairs.  Pair m is used when 0 <= corr_a[m] < n_a, 0 <= corr_b[m] < n_b and the six coordinates are finite; the others are
 *    skipped (n_pairs - n_used), which makes dcreg_feature_match's -1 entries harmless.  The used pairs are numbered u = 0 .. M_u - 1
 *    in ascending m; p_u, q_u are their points widened to double.  With M_u < 3 the call returns DCREG_OK with n_returned = 0.
 * 2. Draws (splitmix64, integers mod 2^64).  x(k) = mix(seed + k * 0x9E3779B97F4A7C15) with mix(z): z = (z ^ z >> 30) *
 *    0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.  Hypothesis h = 0 .. H - 1 takes the used pairs
 *    u_j = ((x(3 h + j + 1) >> 32) * M_u) >> 32, j = 0, 1, 2.  Two equal u_j: the hypothesis is DEGENERATE (counted, not drawn again).
 * 3. Pre-rejection (edge_similarity s > 0).  For the edges (i, j) = (0, 1), (1, 2), (2, 0): g = p_i - p_j, la = sqrt((g_x g_x + g_y g_y)
 *    + g_z g_z), lb likewise from q.  The hypothesis is REJECTED unless la >= s * lb and lb >= s * la on all three edges.
 * 4. Pose (a triad; the least-squares fit is step 7).  u = p_1 - p_0, v = p_2 - p_0, w = u x v (w_x = u_y v_z - u_z v_y, cyclic: two
 *    products, one subtraction).  DEGENERATE if w.w <= 1e-4 * ((u.u) * (v.v)); the same test on the q side (both sides are computed).
 *    e1 = u / sqrt(u.u), e3 = w / sqrt(w.w) (per coordinate), e2 = e3 x e1; f1, f2, f3 the same from q.  R_rc = (f1_r e1_c + f2_r e2_c)
 *    + f3_r e3_c.  c_p = ((p_0 + p_1) + p_2) / 3.0 per coordinate, c_q likewise; t_r = c_q_r - ((R_r0 c_p_x + R_r1 c_p_y) + R_r2 c_p_z).
 * 5. Score, over ALL used pairs: r_r = (((R_r0 p_x + R_r1 p_y) + R_r2 p_z) + t_r) - q_r; e2 = (r_x r_x + r_y r_y) + r_z r_z; the pair
 *    is an inlier when e2 <= dd, dd = d * d (d = inlier_distance).  count = the number of inliers; cost = the sum over the inliers of
 *    (uint64) floor((e2 / dd) * 1048576.0).  Both are integers: no order of summation is part of the rule.
 * 6. Rank: (count descending, cost ascending, h ascending) over the n_scored = H - n_degenerate - n_rejected hypotheses; the first
 *    n_returned = min(n_best, n_scored) are returned, best first.  The records behind them are zero.
 * 7. Refinement, for every returned record on its own, refine_iterations times: the inliers of the current pose (step 5's test) in
 *    ascending u; fewer than three: stop (`refined` counts the steps taken).  With n of them: c_p = (sum p) / n per coordinate, the sum
 *    from 0.0 left to right, c_q likewise; S_ab = sum (p_a - c_p_a) * (q_b - c_q_b) from 0.0 left to right, the product rounded, then
 *    added.  Horn's matrix: N00 = (Sxx + Syy) + Szz, N11 = (Sxx - Syy) - Szz, N22 = (Syy - Sxx) - Szz, N33 = (Szz - Sxx) - Syy,
 *    N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx, N12 = Sxy + Syx, N13 = Szx + Sxz, N23 = Syz + Szy, symmetric.  V = I.  Eight
 *    cyclic Jacobi sweeps over (0,1), (0,2), (0,3), (1,2), (1,3), (2,3); one rotation of (p, q), as for the normals' 3x3: t = 0 if
 *    N_pq == 0, otherwise theta = (N_qq - N_pp) / (2.0 * N_pq), t = (theta >= 0 ? 1.0 : -1.0) / (|theta| + sqrt(theta * theta + 1.0));
 *    c = 1.0 / sqrt(t * t + 1.0); s = t * c; N_pp -= t * N_pq; N_qq += t * N_pq; N_pq = 0; for the two other rows r (ascending):
 *    N_rp' = c * N_rp - s * N_rq, N_rq' = s * N_rp + c * N_rq (and their mirror images); for the four rows k of V: V_kp' = c * V_kp -
 *    s * V_kq, V_kq' = s * V_kp + c * V_kq.  The column of V under the largest diagonal entry (the lowest index among equals) is
 *    (w, x, y, z); negated if w < 0; divided by sqrt(((w w + x x) + y y) + z z).  With the nine products xx .. wz:
 *      R00 = 1.0 - 2.0 * (yy + zz)   R01 = 2.0 * (xy - wz)         R02 = 2.0 * (xz + wy)
 *      R10 = 2.0 * (xy + wz)         R11 = 1.0 - 2.0 * (xx + zz)   R12 = 2.0 * (yz - wx)
 *      R20 = 2.0 * (xz - wy)         R21 = 2.0 * (yz + wx)         R22 = 1.0 - 2.0 * (xx + yy)
 *    and t from c_p, c_q as in step 4.  After the iterations: n_inliers and rmse = sqrt((sum e2) / n_inliers) over the inliers of the
 *    final pose in ascending u, the sum from 0.0 (0.0 without an inlier), and for record 0 the mask: inlier_mask_out[m] = 1 for the
 *    correspondences m of those inliers, 0 for every other one of the n_pairs (all 0 when nothing is returned).
 * `count` and `cost` are the unrefined hypothesis's (the ranking key); T, n_inliers and rmse the refined pose's.  `pairs` are the
 * correspondence numbers m of u_0, u_1, u_2.
 *
 * Steps 1 to 6 run on the device, step 7 on the host from the used pairs (28 bytes each, downloaded once).  The call touches nothing
 * else in the context and waits for the stream; repeated calls and calls on another context are bitwise equal; no result depends on
 * how the scorer splits the pairs over blocks ("align_score_split": used pairs per block column, 0 = chosen from the sizes; a test option).
 * DCREG_E_INVALID, before anything is queued: null context, parameters or records; n_hypotheses outside 1 .. 2^24; n_best outside
 * 1 .. 32; refine_iterations outside 0 .. 8; an inlier_distance that is not finite or not > 0; an edge_similarity outside [0, 1) or not
 * finite; a stride below 3; a negative count; more than 2^31 - 1 points or pairs; a null cloud with a positive point count; a null index
 * array with n_pairs > 0.  DCREG_E_STATE: a linearisation in flight.  Device memory: the clouds and index arrays (the host form),
 * 36 bytes per correspondence, 32 bytes per hypothesis (the survivors' keys, unsorted and sorted) - kept as scratch of the context. */
typedef struct dcreg_align_params {
    int64_t n_hypotheses;      /* H, 1 .. 2^24 */
    uint64_t seed;
    double inlier_distance;    /* d > 0, metres */
    double edge_similarity;    /* s in [0, 1): 0 = no pre-rejection; Open3D's edge-length checker uses 0.9 */
    int n_best;                /* T, 1 .. 32 records returned */
    int refine_iterations;     /* 0 .. 8 */
    double reserved_[2];
} dcreg_align_params;
typedef struct dcreg_align_record {   /* one per returned hypothesis, best first */
    double T[16];              /* row-major 4x4, bottom row 0 0 0 1: q ~ R p + t; feeds every T0 argument as it is */
    int64_t hypothesis;        /* h */
    int32_t pairs[3];          /* the three correspondence numbers m it was drawn from */
    int32_t count;             /* inliers of the unrefined hypothesis (the ranking key) */
    uint64_t cost;             /* its integer cost (ranking key) */
    int32_t n_inliers;         /* inliers of T, after refinement */
    int32_t refined;           /* refinement steps actually taken */
    double rmse;               /* over the inliers of T */
} dcreg_align_record;
typedef struct dcreg_align_info {
    int64_t n_pairs, n_used, n_drawn, n_degenerate, n_rejected, n_scored, n_returned;
    int64_t reserved_;
} dcreg_align_info;
/* H = 100000, seed = 0, d = 0.5, s = 0.9, T = 1, refine = 3 */
int dcreg_default_align_params(dcreg_align_params *);
int dcreg_align_correspondences(dcreg_ctx *, const float *a_xyz, int64_t n_a, int64_t stride_a, const float *b_xyz, int64_t n_b,
                                int64_t stride_b, const int32_t *corr_a, const int32_t *corr_b, int64_t n_pairs, const dcreg_align_params *,
                                dcreg_align_record *records_out, uint8_t *inlier_mask_out, dcreg_align_info *info);
int dcreg_align_correspondences_device(dcreg_ctx *, const float *d_a_xyz, int64_t n_a, int64_t stride_a, const float *d_b_xyz, int64_t n_b,
                                       int64_t stride_b, const int32_t *d_corr_a, const int32_t *d_corr_b, int64_t n_pairs,
                                       const dcreg_align_params *, dcreg_align_record *records_out, uint8_t *d_inlier_mask_out,
                                       dcreg_align_info *info);

/* ---------------- Consensus pose from a compatibility graph ----------------
 * The same stage as the call above, for inlier shares a three-pair sampler does not survive (an all-inlier draw has the probability of
 * the share cubed): a rigid motion keeps lengths, so two right pairs (p_i, q_i), (p_j, q_j) have |p_i - p_j| ~ |q_i - q_j|, the right
 * pairs form a clique in that compatibility graph, and second-order counts - the compatible neighbours two compatible pairs share -
 * make the clique stand out (SC2-PCR, the graph stage of TEASER).  The same clouds and index arrays go in, records with 4x4 poses come
 * out.  Arithmetic as above: double, every operation rounded once, a dot product is (x + y) + z, nothing contracted; every quantity of
 * the graph is a bit or an integer.  The output is BITWISE the numpy reference of tests/consensus_ref.py, with no stated freedom.
 *
 * 1. Used pairs: step 1 of the rule above, unchanged - the same test, u = 0 .. M_u - 1 in ascending m, p_u and q_u widened to double.
 *    With M_u < 3 the call returns DCREG_OK with nothing returned and an all-zero mask.
 * 2. Compatibility.  For u != v: g = p_u - p_v, la = sqrt((g_x g_x + g_y g_y) + g_z g_z), lb likewise from q (the squares make both
 *    symmetric bitwise).  C(u, v) = 1 when corr_a[m_u] != corr_a[m_v] and corr_b[m_u] != corr_b[m_v] and la >= min_length and
 *    lb >= min_length and fabs(la - lb) <= compat_distance; C(u, u) = 0.  deg(u) = the number of ones in row u.
 * 3. Second-order counts and weights.  S(u, v) = C(u, v) * |{x : C(u, x) and C(v, x)}|; w(u) = sum over v of S(u, v).  With
 *    M_u <= 32768, w < 2^31.  Integers: no order is part of the rule.
 * 4. Seeds and their sets.  The seeds are the first min(n_seeds, M_u) used pairs in the order (w descending, u ascending); a seed's
 *    rank r is its place there.  For seed s: S_max = max over v of S(s, v); the candidates are the v with C(s, v) = 1, S(s, v) >= 1
 *    and 2 * S(s, v) >= S_max; the members are s and the first min(consensus_size - 1, candidates) candidates in the order (S(s, v)
 *    descending, v ascending).  A seed with fewer than three members is SKIPPED: counted, and no further seed is taken in its place.
 * 5. Pose of a set: the fit of step 7 above - centroids, S_ab, Horn's N, eight Jacobi sweeps, quaternion, R, t - over the members in
 *    ascending u, once.
 * 6. Score, over ALL used pairs: step 5 above with d = inlier_distance - the integer count and the integer cost.
 * 7. Rank: (count descending, cost ascending, r ascending) over the n_scored seeds not skipped; the first n_returned = min(n_best,
 *    n_scored) are returned, best first, each refined refine_iterations times exactly as step 7 above refines a record; n_inliers,
 *    rmse and record 0's inlier_mask_out as there.  The records behind them are zero.
 * `count` and `cost` are the set's unrefined pose's (the ranking key); T, n_inliers and rmse the refined pose's.
 *
 * Optional outputs, each may be null (host pointers in the host form, device pointers in the device form):
 *   members_out [n_best x consensus_size] int32: the correspondence numbers m of the members of each returned record in ascending u,
 *               padded with -1 (rows behind the returned ones are all -1)
 *   degree_out  [n_pairs] uint32: deg of every used pair, 0 at unused pairs
 *   weight_out  [n_pairs] uint32: w likewise.  The weights are a product in their own right: a pair without a compatible neighbour
 *               that shares one has w = 0, so a caller can keep the pairs with w > 0 and give those to dcreg_align_correspondences,
 *               whose sampler then draws from a far higher inlier share.
 * Steps 1 to 4 and 6 run on the device; the host fits the seeds' poses from their member lists (at most 1024 x 64 indices, OpenMP over
 * the seeds), uploads 12 doubles per seed, ranks the at most 1024 scores and refines the returned records.  The graph is a bit matrix
 * of M_u^2 / 8 bytes (128 MiB at the cap) and one uint16 row of counts per seed, kept as scratch of the context.  The call touches
 * nothing else in the context and waits for the stream; repeated calls and calls on another context are bitwise equal.
 * DCREG_E_INVALID, before anything is queued: what dcreg_align_correspondences lists for its context, records, clouds, index arrays,
 * strides and counts; n_pairs > 32768; a compat_distance or inlier_distance that is not finite or not > 0; a min_length that is not
 * finite or < 0; n_seeds outside 1 .. 1024; consensus_size outside 3 .. 64; n_best outside 1 .. 32; refine_iterations outside 0 .. 8.
 * DCREG_E_STATE: a linearisation in flight. */
typedef struct dcreg_consensus_params {
    double compat_distance;    /* > 0, metres: two pairs are compatible when their lengths differ by no more */
    double min_length;         /* >= 0, metres: pairs closer than this on either side say nothing about each other */
    double inlier_distance;    /* d > 0, metres */
    int n_seeds;               /* 1 .. 1024 */
    int consensus_size;        /* 3 .. 64 members of a set, the seed among them */
    int n_best;                /* 1 .. 32 records returned */
    int refine_iterations;     /* 0 .. 8 */
    double reserved_[2];
} dcreg_consensus_params;
typedef struct dcreg_consensus_record {   /* one per returned seed, best first */
    double T[16];              /* row-major 4x4, bottom row 0 0 0 1: q ~ R p + t; feeds every T0 argument as it is */
    int32_t seed;              /* the correspondence number m of the seed s */
    int32_t seed_rank;         /* r */
    int32_t weight;            /* w(s) */
    int32_t n_members;
    int32_t count;             /* inliers of the set's pose (the ranking key) */
    uint64_t cost;             /* the set's pose's integer cost (ranking key) */
    int32_t n_inliers;         /* inliers of T, after refinement */
    int32_t refined;           /* refinement steps actually taken */
    double rmse;              /* over the inliers of T */
} dcreg_consensus_record;
typedef struct dcreg_consensus_info {
    int64_t n_pairs, n_used, n_edges, max_degree, n_seeds, n_skipped, n_scored, n_returned;
    int64_t reserved_;
} dcreg_consensus_info;
#define DCREG_CONSENSUS_MAX_PAIRS 32768
/* compat_distance = 0.5, min_length = 1.0, d = 0.5, n_seeds = 64, consensus_size = 16, n_best = 1, refine = 3 */
int dcreg_default_consensus_params(dcreg_consensus_params *);
int dcreg_consensus_correspondences(dcreg_ctx *, const float *a_xyz, int64_t n_a, int64_t stride_a, const float *b_xyz, int64_t n_b,
                                    int64_t stride_b, const int32_t *corr_a, const int32_t *corr_b, int64_t n_pairs,
                                    const dcreg_consensus_params *, dcreg_consensus_record *records_out, uint8_t *inlier_mask_out,
                                    int32_t *members_out, uint32_t *degree_out, uint32_t *weight_out, dcreg_consensus_info *info);
int dcreg_consensus_correspondences_device(dcreg_ctx *, const float *d_a_xyz, int64_t n_a, int64_t stride_a, const float *d_b_xyz,
                                           int64_t n_b, int64_t stride_b, const int32_t *d_corr_a, const int32_t *d_corr_b, int64_t n_pairs,
                                           const dcreg_consensus_params *, dcreg_consensus_record *records_out, uint8_t *d_inlier_mask_out,
                                           int32_t *d_members_out, uint32_t *d_degree_out, uint32_t *d_weight_out,
                                           dcreg_consensus_info *info);

/* ---------------- Verification of candidate poses against the map ----------------
 * The stage behind the two calls above (PCL SampleConsensusPrerejective's scoring against the cloud, Open3D evaluate_registration): P
 * candidate poses of ONE cloud are scored against the resident map in one launch - per pose the number of cloud points with a map point
 * strictly inside the inlier distance, and an integer cost of their distances.  The poses of dcreg_align_correspondences,
 * dcreg_consensus_correspondences, a register_frames result or a place-recognition guess go in as they are; the best of the ranked
 * records feed every T0 / T0s argument of the engines.  Counts and costs are integers: the records are BITWISE the numpy reference of
 * tests/verify_ref.py and do not depend on how the work is split over blocks or launches.
 *
 * Inputs: the poses T_k, k = 0 .. P - 1 (row-major 4x4 at T + k * pose_stride_doubles; the bottom row is ignored), a cloud, and
 * d = inlier_distance, s = point_stride, rank_by, detail_pose.
 * 1. Points.  The resident form takes the source as dcreg_set_source* holds it, original indices i = 0 .. n - 1 (all finite).  The
 *    cloud forms take n rows of a caller's cloud; row i is USED when its three coordinates are finite.  Row i is SELECTED when
 *    i % s == 0 - the stride is taken on the original index, before the finiteness test.  n_scored = the selected used points.
 * 2. Transform (the engines' body_to_global): per coordinate a, ((R_a0 * px + R_a1 * py) + R_a2 * pz) + t_a in double, every operation
 *    rounded once, nothing contracted; the result is stored as float32.  A transformed point with a non-finite coordinate is not an
 *    inlier of that pose.
 * 3. Nearest map point: d2 = (dx * dx + dy * dy) + dz * dz in float32, as dcreg_knn computes it; j = the map point of the smallest
 *    (d2, original index) over the WHOLE resident map (the call makes the whole map's index the active one, as the metrics do).
 * 4. Inlier iff (double)d2 < dd, dd = d * d in double - STRICT, the search's convention, not the `<=` of the align rule.  Its term:
 *    e = (uint64) floor(((double)d2 / dd) * 1048576.0), at most 2^20 - 1.
 * 5. Sums: count_k = the inliers, cost_k = the sum of their e, score_k = cost_k + (n_scored - count_k) * 1048576 - an MSAC score:
 *    every outlier pays the full 2^20.  Integers all three: no order of summation is part of the rule.
 * 6. Derived: fitness_k = (double)count_k / (double)n_scored (0.0 when n_scored is 0); rmse_k = sqrt((((double)cost_k / 1048576.0) * dd)
 *    / (double)count_k) (0.0 when count_k is 0).  rmse_k is the FLOOR-QUANTISED value: its square lies at most dd * 2^-20 below the mean
 *    of the inliers' float d2 (each term loses less than one unit of 2^-20 dd), and never above it but for the rounding of these four
 *    double operations.
 * 7. Rank.  rank_by = 0: (count descending, cost ascending, k ascending) - the key of the align and consensus records.  rank_by = 1:
 *    (score ascending, count descending, k ascending).  All P records come back, best first, each with its input index k in `pose`.
 * 8. Detail of one pose: detail_pose = an input index k, or -1 for none.  mask_out[i] = 1 where point i is an inlier of that pose, 0
 *    elsewhere (rows that are not selected or not used included); nn_out[i] = j for an inlier, -1 elsewhere - n entries each, in the
 *    cloud's original order.  Either may be null; both are left alone when detail_pose is -1.
 *
 * dcreg_verify_poses scores the resident source.  dcreg_verify_poses_cloud / _cloud_device score a caller's cloud (xyz, n,
 * stride_floats) in host / device memory - the device form also takes device pointers for mask_out and nn_out - and neither read nor
 * change the resident source.  With pose_stride_doubles = 22 the T of an array of dcreg_align_record or dcreg_consensus_record - 176
 * bytes each - is read in place.  The calls wait for the stream, keep nothing from one call to the next but scratch memory, touch no
 * warm state, no kept normals or voxels and no source ordering; the whole map's index becomes the active one.  One launch scores all
 * poses: block (x, k) takes 256 selected points at pose k; with s > 1 the selected points are compacted first.  "verify_poses_per_launch"
 * (0 = all; a test option) splits the poses over several launches; no result depends on it.
 * DCREG_E_INVALID, before anything is queued and with records, detail outputs and info untouched: a null context, parameters or records;
 * n_poses outside 0 .. 65535 (0 returns DCREG_OK with a zero info); a null T with n_poses > 0; pose_stride_doubles < 16; an
 * inlier_distance that is not finite or not > 0; point_stride < 1; rank_by outside 0 and 1; detail_pose outside -1 .. n_poses - 1; a
 * cloud stride below 3, a negative n, more than 2^31 - 1 points, a null cloud with n > 0; a pose with a non-finite entry in its top
 * three rows or whose rotation block is no rotation (|R^T R - I| > 1e-6 in an entry, or det <= 0: the rule of dcreg_p2p_error) - the
 * message names the pose's index.  DCREG_E_STATE: a linearisation in flight; no map; the resident form without a source. */
typedef struct dcreg_verify_params {
    double inlier_distance;    /* d > 0, metres */
    int64_t point_stride;      /* s >= 1: every s-th point of the cloud, by original index */
    int32_t rank_by;           /* 0: (count desc, cost asc, k asc); 1: (score asc, count desc, k asc) */
    int32_t detail_pose;       /* the input index whose mask / nn are written, -1: none */
    double reserved_[2];
} dcreg_verify_params;
typedef struct dcreg_verify_record {   /* one per pose, best first */
    int32_t pose;              /* k: the input index */
    int32_t count;             /* inliers */
    uint64_t cost;             /* sum of the inliers' terms */
    uint64_t score;            /* cost + (n_scored - count) * 2^20 */
    double fitness;            /* count / n_scored */
    double rmse;               /* floor-quantised, see step 6 */
} dcreg_verify_record;
typedef struct dcreg_verify_info {
    int64_t n_poses, n_points, n_scored, best_pose;   /* best_pose: records_out[0].pose (0 in the zero info of a call without poses) */
    int64_t reserved_[2];
} dcreg_verify_info;
#define DCREG_VERIFY_MAX_POSES 65535
/* d = 0.5, stride 1, rank_by 0, detail_pose -1 */
int dcreg_default_verify_params(dcreg_verify_params *);
int dcreg_verify_poses(dcreg_ctx *, const double *T, int64_t n_poses, int64_t pose_stride_doubles, const dcreg_verify_params *,
                       dcreg_verify_record *records_out, uint8_t *mask_out, int32_t *nn_out, dcreg_verify_info *info);
int dcreg_verify_poses_cloud(dcreg_ctx *, const float *xyz, int64_t n, int64_t stride_floats, const double *T, int64_t n_poses,
                             int64_t pose_stride_doubles, const dcreg_verify_params *, dcreg_verify_record *records_out, uint8_t *mask_out,
                             int32_t *nn_out, dcreg_verify_info *info);
int dcreg_verify_poses_cloud_device(dcreg_ctx *, const float *d_xyz, int64_t n, int64_t stride_floats, const double *T, int64_t n_poses,
                                    int64_t pose_stride_doubles, const dcreg_verify_params *, dcreg_verify_record *records_out,
                                    uint8_t *d_mask_out, int32_t *d_nn_out, dcreg_verify_info *info);

size_t dcreg_sizeof(const char *struct_name);
const char *dcreg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DCREG_H */
