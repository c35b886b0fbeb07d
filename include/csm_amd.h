/*
 * csm_amd.h — C-ABI of the MI355X-native correlative scan matcher.
 *
 * Drop-in boundary for Cartographer's scan-matching hot path
 * (reference: juwangvsu/cartographer-1). Every entry point below replaces a
 * reference interface, cited as file:line relative to the reference root.
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Return codes: CSM_OK (0) = matched / success, CSM_NO_MATCH (1) = the search
 * completed without a score above min_score (the reference's `false` /
 * nullptr), negative = error. The reference aborts via glog CHECK on invariant
 * violations; the C++ shim (include/cartographer_amd/scan_matching.h) turns
 * negative codes into aborts to keep those semantics.
 *
 * Threading: matcher handles are re-entrant for concurrent match calls (the
 * reference calls const Match methods concurrently from ThreadPool workers,
 * constraint_builder_2d.cc:100-111). A single Match / MatchFullSubmap call
 * (csm_fast2d_match*, csm_fast3d_match*) takes a call context from a pool on
 * the matcher's context for its duration: its own HIP stream and scratch,
 * the matcher's device pyramid shared read-only, so concurrent callers'
 * searches overlap on the GPU. Calls that name a context (batches, RTCSM,
 * filters, refinement) serialise on that context's stream; use one context
 * per calling thread to run those concurrently. Destroying a handle while a
 * call uses it is the caller's error, as in the reference.
 */
#ifndef CSM_AMD_H_
#define CSM_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSM_OK 0
#define CSM_NO_MATCH 1
#define CSM_EINVAL (-1)
#define CSM_EHIP (-2)
#define CSM_ENOMEM (-3)
#define CSM_ERANGE (-4) /* input exceeds the device path's index limits */

/* mapping/2d/map_limits.h:40-96 (resolution, max corner, CellLimits
 * xy_index.h:34-45). Cell (x, y) lives at flat index x + y * num_x_cells
 * (grid_2d.h:113-116); x counts down from max_y, y down from max_x
 * (map_limits.h:69-75). */
typedef struct csm_map_limits {
  double resolution;
  double max_x, max_y;
  int32_t num_x_cells, num_y_cells;
} csm_map_limits;

/* transform::Rigid2d (transform/rigid_transform.h:33-86): translation and an
 * unnormalized rotation angle. */
typedef struct csm_pose2d {
  double x, y, theta;
} csm_pose2d;

/* proto::FastCorrelativeScanMatcherOptions2D
 * (proto/scan_matching/fast_correlative_scan_matcher_options_2d.proto:19-30). */
typedef struct csm_fast2d_options {
  double linear_search_window;
  double angular_search_window;
  int32_t branch_and_bound_depth;
  /* Device-side search pyramid depth (>= branch_and_bound_depth, <= 12). The
   * branch and bound is exact, so extra coarse levels change only the work
   * done, never the result (DESIGN.md "Search"). 0 = automatic. */
  int32_t search_depth;
} csm_fast2d_options;

/* proto::RealTimeCorrelativeScanMatcherOptions
 * (proto/scan_matching/real_time_correlative_scan_matcher_options.proto:19-31). */
typedef struct csm_rt_options {
  double linear_search_window;
  double angular_search_window;
  double translation_delta_cost_weight;
  double rotation_delta_cost_weight;
} csm_rt_options;

typedef struct csm_context csm_context;   /* device, stream, scratch */
typedef struct csm_fast2d csm_fast2d;     /* one submap's device pyramid */
typedef struct csm_scan_set csm_scan_set; /* device-resident node clouds */

/* ---- context -------------------------------------------------------------- */
int csm_context_create(int32_t device, csm_context** out);
void csm_context_destroy(csm_context* ctx);
/* hipStream_t the context launches on (as void*), for event timing. */
void* csm_context_stream(csm_context* ctx);

/* Kernel timing, accumulated with HIP events on the context stream while
 * enabled: the candidate-scoring (search) kernel's total device milliseconds,
 * launches and algorithmic bytes (candidates scored x points x 1 B). */
typedef struct csm_timing {
  double search_kernel_ms;
  int64_t search_launches;
  double search_lookups;   /* candidates scored x points */
  double search_candidates;
  double other_kernel_ms;
  /* 3D: RTCSM3D scoring kernel time and lookups (candidates x points);
   * FastCSM3D search kernel time, launches and pyramid lookups. */
  double rt3d_kernel_ms;
  double rt3d_lookups;
  double fast3d_kernel_ms;
  int64_t fast3d_launches;
  double fast3d_lookups;
  /* Search health, accumulated while timing is enabled: pairs whose batch
   * search returned an error status (< 0), and the largest DFS stack depth
   * (entries) any workgroup reached (2D and 3D). */
  int64_t search_errors;
  int64_t stack_high_water;
  /* 2D searches whose maximum was reached by more than one leaf (the
   * reference's pick among them is restored, DESIGN.md §2 "Ties"), and those
   * of them picked by walking the reference's order on the device because
   * more than 4096 leaves tied (CSM_TIE_WALK; counted whether or not timing
   * is enabled). */
  int64_t tied_pairs;
  /* Named ties_unresolved before round 5 (same slot, same layout). */
  int64_t ties_walked;
  /* Pairs (2D and 3D) whose pick needed the whole lowest-resolution list
   * ordered (CSM_TIE_TOPLIST). 3D: pairs whose best sum was reached by more
   * than one leaf passing the low-resolution check, and those of them picked
   * by the ordered walk (more than 4096 such leaves). */
  int64_t ties_toplist;
  int64_t tied_pairs_3d;
  int64_t ties_walked_3d; /* named ties_unresolved_3d before round 5 */
} csm_timing;
void csm_context_enable_timing(csm_context* ctx, int32_t enable);
void csm_context_get_timing(csm_context* ctx, csm_timing* out);
void csm_context_reset_timing(csm_context* ctx);
/* Per pyramid level: candidates scored and scoring batches (v2 kernel),
 * accumulated while timing is enabled. Returns the number of levels written. */
int32_t csm_context_level_stats(csm_context* ctx, double* candidates, double* batches,
                                int32_t max_levels);

/* ---- FastCorrelativeScanMatcher2D ------------------------------------------
 * csm_fast2d_create replaces the constructor
 *   FastCorrelativeScanMatcher2D(const Grid2D&, const Options2D&)
 *   (fast_correlative_scan_matcher_2d.h:114-116, .cc:188-194)
 * and builds the PrecomputationGridStack2D (.cc:171-186) on the device.
 * `cells` are the grid's uint16 correspondence-cost values
 * (Grid2D::correspondence_cost_cells, grid_2d.h:97-99); min/max cc are
 * Grid2D::GetMin/MaxCorrespondenceCost (grid_2d.h:61-67). The cells are copied:
 * the caller may free them on return. */
int csm_fast2d_create(csm_context* ctx, const csm_map_limits* limits,
                      const uint16_t* cells, float min_correspondence_cost,
                      float max_correspondence_cost,
                      const csm_fast2d_options* options, csm_fast2d** out);
void csm_fast2d_destroy(csm_fast2d* m);

/* bool Match(const Rigid2d& initial_pose_estimate, const PointCloud&,
 *            float min_score, float* score, Rigid2d* pose_estimate) const
 *   (fast_correlative_scan_matcher_2d.h:127-129, .cc:198-208).
 * points: n x (x, y, z) floats (sensor::RangefinderPoint, point_cloud.h). */
int csm_fast2d_match(const csm_fast2d* m, const csm_pose2d* initial,
                     const float* points_xyz, int32_t n, float min_score,
                     float* score, csm_pose2d* pose);

/* bool MatchFullSubmap(const PointCloud&, float min_score, float* score,
 *                      Rigid2d* pose_estimate) const
 *   (fast_correlative_scan_matcher_2d.h:135-136, .cc:210-225). */
int csm_fast2d_match_full_submap(const csm_fast2d* m, const float* points_xyz,
                                 int32_t n, float min_score, float* score,
                                 csm_pose2d* pose);

/* Device bytes a matcher holds (its pyramid planes and cost grid), for a
 * caller's cache budget (the drop-in builders' matcher_cache_bytes; the
 * reference keeps every matcher until DeleteScanMatcher,
 * constraint_builder_2d.cc:165-186, :307-316). */
int64_t csm_fast2d_device_bytes(const csm_fast2d* m);

/* Test-visible: copies PrecomputationGrid2D level `level` (uint8 wide grid,
 * fast_correlative_scan_matcher_2d.h:49-93) to host. */
int csm_fast2d_read_level(const csm_fast2d* m, int32_t level, uint8_t* out,
                          int64_t capacity, int32_t* wide_nx, int32_t* wide_ny);

/* Test-visible: the search plane of level `level` as the v4/v5 kernels load
 * it (raw bytes, polyphase storage order), and its layout in layout8:
 * [0] entry bytes (0: the node chain reaches no plane at this level, 4: quad,
 * 16: hex), [1] quad_w, [2] quad_h, [3] quad_pws, [4] quad_pph, [5] quad_bias,
 * [6] cshift, [7] plane bytes. out == NULL: the layout only. */
int csm_fast2d_read_plane(const csm_fast2d* m, int32_t level, uint8_t* out,
                          int64_t capacity, int32_t* layout8);

/* ---- Batched constraint search (the throughput path) ----------------------
 * Replaces the per-pair Tasks ConstraintBuilder2D schedules
 * (constraint_builder_2d.cc:77-137, ComputeConstraint :188-277): a set of
 * node clouds lives on the device once; each pair names a submap handle and a
 * node; results come back in pair order. */
int csm_scan_set_create(csm_context* ctx, const float* points_xyz,
                        const int64_t* offsets, int32_t num_scans,
                        csm_scan_set** out);
void csm_scan_set_destroy(csm_scan_set* s);
/* Appends num_scans clouds (offsets[0] == 0, as for create) to a live set:
 * the earlier scans keep their indices, device copies and cached rotation
 * tables, and the first new scan gets index *first_index. Lets a builder keep
 * one set across flushes (TrajectoryNode::Data clouds are immutable, so a
 * node's cloud is uploaded once, not once per flush). */
int csm_scan_set_append(csm_scan_set* s, const float* points_xyz,
                        const int64_t* offsets, int32_t num_scans,
                        int32_t* first_index);
/* Scans and points currently held (for a caller's cache limit). */
int csm_scan_set_size(const csm_scan_set* s, int32_t* num_scans, int64_t* num_points);

typedef struct csm_pair2d {
  int32_t submap;      /* index into the submaps[] array */
  int32_t scan;        /* index into the scan set */
  int32_t full_submap; /* 1 = MatchFullSubmap, 0 = Match(initial) */
  float min_score;
  csm_pose2d initial;  /* used when full_submap == 0 */
} csm_pair2d;

/* How a result was picked among exactly tied maxima (csm_result2d.tie;
 * DESIGN.md §2 "Exactly tied maxima"). The reference returns the first
 * maximal leaf its depth-first search visits
 * (fast_correlative_scan_matcher_2d.cc:276-312, :331-332, :344-376):
 *   NONE       one leaf reaches the maximum;
 *   ANCESTORS  several do, all under one highest-scoring lowest-resolution
 *              candidate: the pick follows the children's visiting order;
 *   TOPLIST    two distinct lowest-resolution candidates share the highest
 *              score: the pair's whole lowest-resolution list was scored and
 *              ordered with std::sort's introsort to find the first;
 *   WALK       more tied leaves than the collect pass records (4096): the
 *              device walks the reference's visiting order itself, from the
 *              sorted lowest-resolution list down to the first leaf at the
 *              maximum (any number of tied leaves).
 * Every branch returns the reference's leaf; none falls back to another. */
#define CSM_TIE_NONE 0
#define CSM_TIE_ANCESTORS 1
#define CSM_TIE_TOPLIST 2
#define CSM_TIE_WALK 3
/* Round-4 name of code 3 (before the walk resolved every such pair, it marked
 * them unresolved); kept so that callers written against it still compile. */
#define CSM_TIE_UNRESOLVED CSM_TIE_WALK

typedef struct csm_result2d {
  int32_t status;      /* CSM_OK, CSM_NO_MATCH or a negative error */
  float score;
  csm_pose2d pose;
  int32_t tie;         /* CSM_TIE_* (CSM_OK results only) */
  int32_t reserved;
} csm_result2d;

/* The submap handles may come from any context on ctx's device (e.g. one
 * whose stream builds the next batch's pyramids while ctx searches); the
 * scan set is ctx's. */
int csm_fast2d_match_batch(csm_context* ctx, csm_fast2d* const* submaps,
                           int32_t num_submaps, const csm_scan_set* scans,
                           const csm_pair2d* pairs, int64_t num_pairs,
                           csm_result2d* results);

/* ---- RealTimeCorrelativeScanMatcher2D --------------------------------------
 * double Match(const Rigid2d& initial_pose_estimate, const PointCloud&,
 *              const Grid2D&, Rigid2d* pose_estimate) const
 *   (real_time_correlative_scan_matcher_2d.h:66-68, .cc:117-149), for a
 * ProbabilityGrid. Returns CSM_OK and writes the best candidate's score. */
int csm_rt2d_match(csm_context* ctx, const csm_rt_options* options,
                   const csm_map_limits* limits, const uint16_t* cells,
                   float min_correspondence_cost, float max_correspondence_cost,
                   const csm_pose2d* initial, const float* points_xyz,
                   int32_t n, double* score, csm_pose2d* pose);

/* The same Match() for a TSDF2D grid (GridType::TSDF,
 * real_time_correlative_scan_matcher_2d.cc:38-59 and :162-167): the grid
 * crosses as its two uint16 arrays, correspondence_cost_cells() (TSD values,
 * tsdf_2d.cc:73-79) and weight_cells_ (tsdf_2d.cc:81-87), both x-fastest
 * num_x_cells * num_y_cells, plus the TSDValueConverter parameters
 * (truncation distance = max TSD, max weight; tsd_value_converter.cc:22-33).
 * Candidate score = sum((trunc - |tsd|) / trunc * weight) / sum(weight), 0 when
 * no point lands on a weighted cell; outside the limits a point reads
 * (-trunc, 0). */
int csm_rt2d_match_tsdf(csm_context* ctx, const csm_rt_options* options,
                        const csm_map_limits* limits, const uint16_t* tsd_cells,
                        const uint16_t* weight_cells, float truncation_distance,
                        float max_weight, const csm_pose2d* initial,
                        const float* points_xyz, int32_t n, double* score,
                        csm_pose2d* pose);

/* ---- correlative_scan_matcher_2d.h: search-space helpers ---------------------
 * The free functions and SearchParameters of correlative_scan_matcher_2d.h
 * (:35-68, .cc:27-127), host-side, with the reference's float/double
 * arithmetic (the device path computes the same values internally). */
typedef struct csm_linear_bounds {
  int32_t min_x, max_x, min_y, max_y;  /* inclusive pixel offsets */
} csm_linear_bounds;

typedef struct csm_search_parameters {
  int32_t num_angular_perturbations;
  double angular_perturbation_step_size;
  double resolution;
  int32_t num_scans;
  /* linear_bounds start as +-num_linear_perturbations for every scan. */
  int32_t num_linear_perturbations;
} csm_search_parameters;

/* SearchParameters(linear_search_window, angular_search_window, point_cloud,
 * resolution) (correlative_scan_matcher_2d.cc:27-52). */
int csm_search_parameters_init(double linear_search_window, double angular_search_window,
                               const float* points_xyz, int32_t n, double resolution,
                               csm_search_parameters* out);
/* SearchParameters(num_linear_perturbations, num_angular_perturbations,
 * angular_perturbation_step_size, resolution) — "for testing" (:54-66). */
int csm_search_parameters_init_for_testing(int32_t num_linear_perturbations,
                                           int32_t num_angular_perturbations,
                                           double angular_perturbation_step_size,
                                           double resolution, csm_search_parameters* out);
/* SearchParameters::ShrinkToFit (:68-91): bounds (num_scans entries) are
 * tightened in place against discrete scans (num_scans * points_per_scan
 * (x, y) cell indices, scan-major) and the grid's cell limits. */
int csm_search_parameters_shrink_to_fit(const csm_search_parameters* sp,
                                        const int32_t* discrete_xy, int32_t points_per_scan,
                                        int32_t num_x_cells, int32_t num_y_cells,
                                        csm_linear_bounds* bounds);
/* GenerateRotatedScans (:93-108): out_xyz holds num_scans * n points. */
int csm_generate_rotated_scans(const float* points_xyz, int32_t n,
                               const csm_search_parameters* sp, float* out_xyz);
/* DiscretizeScans (:110-127): num_scans rotated clouds of n points each
 * (scan-major), translated by (initial_x, initial_y) in float and turned
 * into cell indices by MapLimits::GetCellIndex; out_xy receives
 * num_scans * n (x, y) pairs. */
int csm_discretize_scans(const csm_map_limits* limits, const float* rotated_xyz, int32_t n,
                         int32_t num_scans, float initial_x, float initial_y, int32_t* out_xy);

/* Candidate2D (correlative_scan_matcher_2d.h:71-98): score is filled in by
 * ScoreCandidates. */
typedef struct csm_candidate2d {
  int32_t scan_index, x_index_offset, y_index_offset;
  float score;
} csm_candidate2d;

/* RealTimeCorrelativeScanMatcher2D::ScoreCandidates(grid, discrete_scans,
 * search_parameters, candidates*) (real_time_correlative_scan_matcher_2d.h:
 * 75-78, .cc:151-176; visible for testing): every candidate's score =
 * mean probability of its discrete scan shifted by its offsets, times
 * exp(-(hypot(x, y) * w_t + |orientation| * w_r)^2) with the candidate's
 * x, y, orientation from the search parameters. discrete_xy as
 * csm_discretize_scans writes it. */
int csm_rt2d_score_candidates(csm_context* ctx, const csm_rt_options* options,
                              const csm_map_limits* limits, const uint16_t* cells,
                              float min_correspondence_cost, float max_correspondence_cost,
                              const int32_t* discrete_xy, int32_t num_scans,
                              int32_t points_per_scan, const csm_search_parameters* sp,
                              csm_candidate2d* candidates, int64_t num_candidates);
/* The same over a TSDF2D (grid arrays as csm_rt2d_match_tsdf). */
int csm_rt2d_score_candidates_tsdf(csm_context* ctx, const csm_rt_options* options,
                                   const csm_map_limits* limits, const uint16_t* tsd_cells,
                                   const uint16_t* weight_cells, float truncation_distance,
                                   float max_weight, const int32_t* discrete_xy,
                                   int32_t num_scans, int32_t points_per_scan,
                                   const csm_search_parameters* sp,
                                   csm_candidate2d* candidates, int64_t num_candidates);

/* ---- 3D: HybridGrid ----------------------------------------------------------
 * A HybridGrid (mapping/3d/hybrid_grid.h:463-545) crosses the boundary as the
 * list its iterator / ToProto yields (hybrid_grid.h:530-541): cell indices
 * (x, y, z) and uint16 probability values. The device keeps a dense brick
 * over the known cells' bounding box; outside it the value is 0 (unknown,
 * probability kMinProbability), as DynamicGrid::value returns for cells never
 * set (:260-279). `grid_size` is DynamicGrid::grid_size() of the source grid
 * (FastCorrelativeScanMatcher3D's width_in_voxels, .cc:120); 0 = derive it from
 * the indices with DynamicGrid's growth rule (128 << k, indices in
 * [-size/2, size/2)). The cells are copied. */
typedef struct csm_hybrid_grid csm_hybrid_grid;
typedef struct csm_intensity_grid csm_intensity_grid; /* below: device-resident IntensityHybridGrid */
int csm_hybrid_grid_create(csm_context* ctx, float resolution, const int32_t* xyz_indices,
                           const uint16_t* values, int64_t count, int32_t grid_size,
                           csm_hybrid_grid** out);
/* `num` grids in one call, each as csm_hybrid_grid_create builds it (the
 * same bricks and values), with one upload and one launch per build step for
 * all of them: for a caller that builds many submaps' grids at once (the
 * constraint builder's matcher construction, constraint_builder_3d.cc:
 * 170-198). grid_sizes may be NULL (every grid derives its size). */
int csm_hybrid_grid_create_batch(csm_context* ctx, int32_t num, const float* resolutions,
                                 const int32_t* const* xyz_indices, const uint16_t* const* values,
                                 const int64_t* counts, const int32_t* grid_sizes,
                                 csm_hybrid_grid** out);
void csm_hybrid_grid_destroy(csm_hybrid_grid* g);
/* Bounding box origin / extent of the device brick and the grid size. */
int csm_hybrid_grid_info(const csm_hybrid_grid* g, int32_t* origin3, int32_t* dims3,
                         int32_t* grid_size);
/* Test-visible lookups on the device grid, with the kernels' own code:
 * HybridGrid::GetProbability at n cell indices (hybrid_grid.h:496-499; unknown
 * cells give kMinProbability), and InterpolatedProbabilityGrid::
 * GetInterpolatedValue at n points (interpolated_grid.h:48-105, the
 * CeresScanMatcher3D cost's interpolation). */
int csm_hybrid_grid_get_probability(const csm_hybrid_grid* g, const int32_t* xyz_indices, int64_t n,
                                    float* out);
int csm_hybrid_grid_interpolate(const csm_hybrid_grid* g, const double* xyz, int64_t n,
                                double* out);

/* transform::Rigid3d: translation and rotation quaternion (w, x, y, z). */
typedef struct csm_pose3d {
  double t[3];
  double q[4];
} csm_pose3d;

/* ---- RealTimeCorrelativeScanMatcher3D ----------------------------------------
 * float Match(const Rigid3d& initial_pose_estimate, const PointCloud&,
 *             const HybridGrid&, Rigid3d* pose_estimate) const
 *   (real_time_correlative_scan_matcher_3d.h:47-50, .cc:34-54). */
int csm_rt3d_match(csm_context* ctx, const csm_rt_options* options, const csm_hybrid_grid* grid,
                   const csm_pose3d* initial, const float* points_xyz, int32_t n, float* score,
                   csm_pose3d* pose);

/* The search window Match uses (GenerateExhaustiveSearchTransforms, :55-95):
 * (2L+1)^3 translations and (2A+1)^3 rotations for this cloud and grid
 * resolution. Candidate index = t * num_rotations + r. */
int csm_rt3d_window(const csm_rt_options* options, float resolution, const float* points_xyz,
                    int32_t n, int32_t* num_translations, int32_t* num_rotations);

/* Test-visible: ScoreCandidate (:97-113, score after the exp penalty) of
 * every translation for each of `num_rotations` rotation indices of the
 * window, computed by the same kernel as Match; scores[k * num_translations
 * + t] for rotations[k]. */
int csm_rt3d_score_rotations(csm_context* ctx, const csm_rt_options* options,
                             const csm_hybrid_grid* grid, const csm_pose3d* initial,
                             const float* points_xyz, int32_t n, const int32_t* rotations,
                             int32_t num_rotations, float* scores);

/* ---- FastCorrelativeScanMatcher3D --------------------------------------------
 * proto::FastCorrelativeScanMatcherOptions3D
 * (proto/scan_matching/fast_correlative_scan_matcher_options_3d.proto). */
typedef struct csm_fast3d_options {
  int32_t branch_and_bound_depth;
  int32_t full_resolution_depth;
  double min_rotational_score;
  double min_low_resolution_score;
  double linear_xy_search_window;
  double linear_z_search_window;
  double angular_search_window;
} csm_fast3d_options;

typedef struct csm_fast3d csm_fast3d;

/* FastCorrelativeScanMatcher3D(const HybridGrid&, const HybridGrid* low_res,
 *   const Eigen::VectorXf* histogram, const Options3D&)
 *   (fast_correlative_scan_matcher_3d.h:75-79, .cc:112-123). The pyramid
 * (PrecomputationGridStack3D, .cc:57-77) is built on the device from
 * `high_resolution`; the histogram is copied. As in the reference (which keeps
 * raw pointers, .h:149-150) `low_resolution` must outlive the matcher. */
int csm_fast3d_create(csm_context* ctx, const csm_hybrid_grid* high_resolution,
                      const csm_hybrid_grid* low_resolution, const float* histogram,
                      int32_t histogram_size, const csm_fast3d_options* options,
                      csm_fast3d** out);
/* `count` FastCorrelativeScanMatcher3D constructions in one call (a sweep
 * that builds many submaps' matchers at once, e.g. ConstraintBuilder3D's
 * DispatchScanMatcherConstruction for every submap of a loaded map,
 * constraint_builder_3d.cc:170-198): out[i] is what csm_fast3d_create(ctx,
 * high[i], low[i], histograms[i], histogram_sizes[i], options) returns, with
 * each pyramid level built for all of them in one launch. On error no
 * matcher is returned. count <= 65535. */
int csm_fast3d_create_batch(csm_context* ctx, int32_t count,
                            const csm_hybrid_grid* const* high_resolution,
                            const csm_hybrid_grid* const* low_resolution,
                            const float* const* histograms, const int32_t* histogram_sizes,
                            const csm_fast3d_options* options, csm_fast3d** out);
void csm_fast3d_destroy(csm_fast3d* m);
/* Device bytes of the matcher's pyramid (levels and octet planes), and of a
 * HybridGrid's bricks (as csm_fast2d_device_bytes). */
int64_t csm_fast3d_device_bytes(const csm_fast3d* m);
int64_t csm_hybrid_grid_device_bytes(const csm_hybrid_grid* g);
/* Test-visible: copies pyramid level `level` (dense brick, x fastest);
 * level < csm_fast3d_search_levels, which counts the levels above
 * branch_and_bound_depth that only the device search roots at. */
int csm_fast3d_read_level(const csm_fast3d* m, int32_t level, uint8_t* out, int64_t capacity,
                          int32_t* origin3, int32_t* dims3);
int32_t csm_fast3d_search_levels(const csm_fast3d* m);
/* Test-visible: the octet brick of level `level` < search_levels - 1 as the
 * search loads it (one uint64 per cell, x fastest), its box and the child
 * offset H (oct_h). out == NULL: the box and H only. */
int csm_fast3d_read_octets(const csm_fast3d* m, int32_t level, uint64_t* out, int64_t capacity,
                           int32_t* origin3, int32_t* dims3, int32_t* oct_h);

/* The parts of TrajectoryNode::Data the matcher reads (trajectory_node.h):
 * high/low resolution point clouds, the rotational histogram and the
 * gravity alignment (w, x, y, z). */
typedef struct csm_node3d {
  const float* high_resolution_xyz;
  int32_t num_high_resolution;
  const float* low_resolution_xyz;
  int32_t num_low_resolution;
  const float* histogram;
  int32_t histogram_size;
  double gravity_alignment[4];
} csm_node3d;

/* FastCorrelativeScanMatcher3D::Result (fast_correlative_scan_matcher_3d.h:68-73). */
typedef struct csm_result3d {
  int32_t status; /* CSM_OK, CSM_NO_MATCH (the reference's nullptr) or error */
  float score;
  csm_pose3d pose;
  float rotational_score;
  float low_resolution_score;
  int32_t tie;    /* CSM_TIE_*: how the pick among exactly tied leaves was made */
  int32_t reserved;
} csm_result3d;

/* std::unique_ptr<Result> Match(const Rigid3d& global_node_pose,
 *   const Rigid3d& global_submap_pose, const TrajectoryNode::Data&, float min_score)
 *   (fast_correlative_scan_matcher_3d.h:89-92, .cc:127-143). */
int csm_fast3d_match(const csm_fast3d* m, const csm_pose3d* global_node_pose,
                     const csm_pose3d* global_submap_pose, const csm_node3d* node,
                     float min_score, csm_result3d* result);
/* std::unique_ptr<Result> MatchFullSubmap(const Quaterniond& global_node_rotation,
 *   const Quaterniond& global_submap_rotation, const TrajectoryNode::Data&, float)
 *   (fast_correlative_scan_matcher_3d.h:98-101, .cc:145-170). Rotations (w,x,y,z). */
int csm_fast3d_match_full_submap(const csm_fast3d* m, const double* global_node_rotation,
                                 const double* global_submap_rotation, const csm_node3d* node,
                                 float min_score, csm_result3d* result);

/* Batched 3D constraint search (ConstraintBuilder3D tasks,
 * constraint_builder_3d.cc:200-305): results in pair order. For full_submap
 * pairs only the rotations of the two poses are used. */
typedef struct csm_pair3d {
  int32_t submap;
  int32_t node;
  int32_t full_submap;
  float min_score;
  csm_pose3d node_pose;
  csm_pose3d submap_pose;
} csm_pair3d;

int csm_fast3d_match_batch(csm_context* ctx, csm_fast3d* const* submaps, int32_t num_submaps,
                           const csm_node3d* nodes, int32_t num_nodes, const csm_pair3d* pairs,
                           int64_t num_pairs, csm_result3d* results);

/* Test-visible: the batch search's rotational stage on raw inputs
 * (RotationalScanMatcher::Match, rotational_scan_matcher.cc:119-185, and the
 * min_rotational_score filter of GenerateDiscreteScans,
 * fast_correlative_scan_matcher_3d.cc:258-270), through the two kernels the
 * batch launches. Record p scores the 2 * window + 1 angles
 * yaw0 + (k - window) * step (float arithmetic), k = 0..2 * window, of the
 * `size` buckets at histograms[node_histogram] against those at
 * histograms[submap_histogram]; records may share histograms. */
typedef struct csm_rot_pair3d {
  int32_t node_histogram;   /* float offsets into `histograms` */
  int32_t submap_histogram;
  int32_t size;             /* 0..512 buckets */
  int32_t window;           /* 0..32768 */
  float step, yaw0;
  double min_score;         /* yaw k is kept unless (double)score_k < min_score */
} csm_rot_pair3d;

/* scores: every record's scores, record after record (sum of 2 * window + 1
 * floats). ranges[2 * p], ranges[2 * p + 1]: offset and count of record p's
 * kept yaws in kept_k / kept_scores (capacity: as `scores`), k increasing
 * within a record; the records' ranges tile [0, *num_kept) in no fixed order.
 * CSM_EINVAL: a null pointer, a size, window or histogram offset out of
 * range, a non-finite step, yaw0 or min_score; CSM_ERANGE: more than 65535
 * records or 2^31 - 1 scores. Waits for the stream. */
int csm_rotational_scores_batch(csm_context* ctx, const float* histograms, int64_t num_floats,
                                const csm_rot_pair3d* pairs, int32_t num_pairs, float* scores,
                                int32_t* ranges, int32_t* kept_k, float* kept_scores,
                                int64_t* num_kept);

/* Test-visible: the discrete scans (GenerateDiscreteScans,
 * fast_correlative_scan_matcher_3d.cc:246-295) that csm_fast3d_match_batch
 * searches for the pair (m, node) with these poses, through the batch's own
 * pair preparation, rotational stage and yaw build (the host patches of
 * undecided roundings included). One record per kept yaw, k increasing:
 * the scan's rotation q and GetPoseFromCandidate's normalized rotation n
 * (both w, x, y, z) and its translation t, as the search kernels read them. */
typedef struct csm_discrete_scan3d {
  int32_t k;               /* angle index: angle = (k - angular_window) * angular_step */
  float rotational_score;
  float q[4];
  float n[4];
  float t[3];
} csm_discrete_scan3d;

/* status: the pair's status as csm_result3d.status reports it (CSM_OK, or the
 * error that keeps the batch from searching the pair); *count: kept yaws, of
 * which min(*count, capacity) are written to `scans` (may be NULL with
 * capacity 0). yaw0: the initial angle of the rotational match. */
int csm_fast3d_discrete_scans(csm_context* ctx, csm_fast3d* m, const csm_node3d* node,
                              const csm_pair3d* pair, csm_discrete_scan3d* scans,
                              int32_t capacity, int32_t* count, int32_t* angular_window,
                              float* angular_step, float* yaw0, int32_t* status);

/* ---- CeresScanMatcher2D refinement ------------------------------------------
 * ConstraintBuilder2D::ComputeConstraint refines every accepted match with
 * CeresScanMatcher2D::Match(target_translation = match translation,
 * initial = match, filtered cloud, submap grid) (constraint_builder_2d.cc:
 * 245-249; ceres_scan_matcher_2d.cc:64-105). csm_ceres2d_refine_batch runs
 * that refinement for n (submap, scan) items on the device, over the submaps'
 * csm_fast2d handles (their correspondence-cost grids) and a scan set.
 * Ceres is not part of this library: the solver restates Ceres 1.13's
 * trust-region Levenberg-Marquardt (the version scripts/install_ceres.sh:20
 * pins), pinned by the reference's ceres_scan_matcher_2d_test.cc.
 * iterations (may be NULL) receives the iterations each item ran. */
typedef struct csm_ceres2d_options {
  /* proto::CeresScanMatcherOptions2D (pose_graph.lua:30-39 defaults 20, 10, 1;
   * ceres_solver_options.max_num_iterations = 10). */
  double occupied_space_weight;
  double translation_weight;
  double rotation_weight;
  int32_t max_num_iterations;
  /* ceres_solver_options.use_nonmonotonic_steps (pose_graph.lua:35: true). */
  int32_t use_nonmonotonic_steps;
} csm_ceres2d_options;

typedef struct csm_refine2d {
  int32_t submap;  /* index into submaps[] */
  int32_t scan;    /* index into the scan set */
  csm_pose2d initial;
  double target_x, target_y;
} csm_refine2d;

int csm_ceres2d_refine_batch(csm_context* ctx, csm_fast2d* const* submaps, int32_t num_submaps,
                             const csm_scan_set* scans, const csm_refine2d* items, int64_t n,
                             const csm_ceres2d_options* options, csm_pose2d* out,
                             int32_t* iterations);

/* The submaps may be TSDF handles (csm_fast2d_create_tsdf,
 * csm_fast2d_create_from_tsdf_grid), and one call may mix both kinds: a TSDF
 * item's first residual block is TSDFMatchCostFunction2D
 * (tsdf_match_cost_function_2d.cc:39-66 over interpolated_tsdf_2d.h:41-121;
 * ceres_scan_matcher_2d.cc:83-90) instead of the occupied-space cost. That
 * functor fails to evaluate where no point reads a weighted cell: at the
 * initial pose the item returns its initial pose and 0 iterations (Ceres ends
 * with FAILURE and CeresScanMatcher2D::Match ignores the summary); at a
 * candidate the step counts as one of infinite cost and is rejected. */

/* Test-visible, like csm_fast2d_read_level: TSDFMatchCostFunction2D alone (no
 * delta rows) on a TSDF handle of ctx, through the device functions the
 * refinement uses. residuals[n] and the row-major n x 3 Jacobian by
 * (x, y, theta) as AutoDiff gives it; *valid is 0, and the outputs are zero,
 * when the functor returns false. A probability handle: CSM_EINVAL. */
int csm_ceres2d_tsdf_evaluate(csm_context* ctx, const csm_fast2d* tsdf_handle,
                              const float* points_xyz, int32_t n, double scaling_factor,
                              const double pose[3], double* residuals, double* jacobian,
                              int32_t* valid);

/* Test-visible: the whole cost of one probability item at `pose`, through the
 * pass over the rows that the refinement kernel runs each iteration (the same
 * device function, which here also writes its rows). The n occupied-space
 * rows of OccupiedSpaceCostFunction2D with weight occupied_space_weight /
 * sqrt(n), then the two translation delta rows to target_xy and the rotation
 * delta row to target_theta (the refinement's initial angle): residuals[n + 3]
 * and the row-major (n + 3) x 3 Jacobian by (x, y, theta). sums[10] are the
 * pass's block-reduced sums as the solver reads them: sum r^2, the upper
 * triangle of J^T J by rows (6), J^T r (3). n >= 1 finite points; the
 * iteration fields of options are not used. A TSDF handle: CSM_EINVAL. */
int csm_ceres2d_evaluate(csm_context* ctx, const csm_fast2d* probability_handle,
                         const csm_ceres2d_options* options, const double target_xy[2],
                         double target_theta, const csm_pose2d* pose, const float* points_xyz,
                         int32_t n, double* residuals, double* jacobian, double* sums);

/* CeresScanMatcher3D refinement (ConstraintBuilder3D::ComputeConstraint,
 * constraint_builder_3d.cc:264-275; ceres_scan_matcher_3d.cc:84-160): the
 * match pose is refined against the submap's high- and low-resolution
 * HybridGrids with the node's high- and low-resolution clouds. Item i uses
 * grids[high_grid], grids[low_grid] and nodes[node]; target is the match
 * translation. Same solver notes as csm_ceres2d_refine_batch. */
typedef struct csm_ceres3d_options {
  /* proto::CeresScanMatcherOptions3D (pose_graph.lua:49-60: 5, 30, 10, 1,
   * max_num_iterations 10). */
  double occupied_space_weight_0;
  double occupied_space_weight_1;
  double translation_weight;
  double rotation_weight;
  int32_t max_num_iterations;
  /* ceres_solver_options.use_nonmonotonic_steps (pose_graph.lua:56: false). */
  int32_t use_nonmonotonic_steps;
} csm_ceres3d_options;

typedef struct csm_refine3d {
  int32_t high_grid, low_grid, node;
  csm_pose3d initial;
  double target[3];
} csm_refine3d;

/* The grids may come from any context on ctx's device; the refinement waits
 * on the device for their builds. */
int csm_ceres3d_refine_batch(csm_context* ctx, const csm_hybrid_grid* const* grids,
                             int32_t num_grids, const csm_node3d* nodes, int32_t num_nodes,
                             const csm_refine3d* items, int64_t n,
                             const csm_ceres3d_options* options, csm_pose3d* out,
                             int32_t* iterations);

/* CeresScanMatcher3D::Match as LocalTrajectoryBuilder3D::ScanMatch calls it
 * with use_intensities (local_trajectory_builder_3d.cc:488-501):
 * csm_ceres3d_refine_batch plus, for item i with intensity_grid_of_item[i] >=
 * 0, an IntensityCostFunction3D block (intensity_cost_function_3d.h:67-85) on
 * the high-resolution cloud (cloud 0 only) in
 * intensity_grids[intensity_grid_of_item[i]], under ceres::HuberLoss
 * (ceres_scan_matcher_3d.cc:126-142): residual k is 0 where the point's
 * intensity is above the threshold and else weight / sqrt(N) * (I(T p_k) -
 * intensity_k), I the InterpolatedGrid over GetIntensity (0 for cells without
 * a return) and N the whole cloud's size. node_intensities[j] are the
 * intensities of node j's high-resolution cloud (NULL: none;
 * node_intensities NULL: no node has any). Items without a grid
 * (intensity_grid_of_item NULL: all of them) run csm_ceres3d_refine_batch's
 * arithmetic and return its result bit for bit; one call may mix both kinds.
 * CSM_EINVAL, when any item has a grid: a weight, huber_scale or
 * intensity_threshold that is not positive (the reference's CHECK_GTs,
 * :127-130), an item whose node has no intensities, a non-finite intensity. A
 * resolution that differs from the high-resolution grid's is allowed, as in
 * the reference. Ceres is not part of this build: the Huber loss and the
 * Corrector rule are restated from Ceres 1.13 and unpinned, like the solver
 * loop. */
typedef struct csm_ceres3d_intensity_options {
  /* proto::IntensityCostFunctionOptions (ceres_scan_matcher_options_3d.proto). */
  double weight;
  double huber_scale;
  double intensity_threshold;
} csm_ceres3d_intensity_options;

int csm_ceres3d_refine_intensity_batch(
    csm_context* ctx, const csm_hybrid_grid* const* grids, int32_t num_grids,
    const csm_intensity_grid* const* intensity_grids, int32_t num_intensity_grids,
    const csm_node3d* nodes, const float* const* node_intensities, int32_t num_nodes,
    const csm_refine3d* items, const int32_t* intensity_grid_of_item, int64_t n,
    const csm_ceres3d_options* options, const csm_ceres3d_intensity_options* intensity_options,
    csm_pose3d* out, int32_t* iterations);

/* Test-visible, like csm_ceres2d_tsdf_evaluate: IntensityCostFunction3D alone
 * (no loss, no other block) at pose (t, then q as w, x, y, z), through the
 * device functions the refinement uses: residuals[n] and the row-major n x 6
 * Jacobian in the tangent space (translation, then the rotation increment of
 * ceres::QuaternionParameterization). Waits for the stream. */
int csm_ceres3d_intensity_evaluate(const csm_intensity_grid* grid, const float* points_xyz,
                                   const float* intensities, int32_t n, const double pose[7],
                                   double scaling_factor, float intensity_threshold,
                                   double* residuals, double* jacobian);

/* Test-visible, like csm_ceres2d_evaluate: the whole cost of one
 * csm_ceres3d_refine_batch item at `pose`, through the pass over the rows that
 * the kernel without an intensity block runs each iteration. The node's
 * high-resolution rows in `high`, its low-resolution rows in `low`, three
 * translation delta rows to target_translation and three rotation delta rows
 * vec(target_rotation^-1 * q) (the refinement takes its initial rotation as
 * target_rotation): with N = num_high_resolution + num_low_resolution + 6,
 * residuals[N] and the row-major N x 6 Jacobian in the tangent space
 * (translation, then the rotation increment of
 * ceres::QuaternionParameterization). sums[28]: sum r^2, the upper triangle of
 * J^T J by rows (21), J^T r (6). Both clouds hold at least one finite point;
 * the iteration fields of options are not used. */
int csm_ceres3d_evaluate(csm_context* ctx, const csm_hybrid_grid* high, const csm_hybrid_grid* low,
                         const csm_node3d* node, const csm_ceres3d_options* options,
                         const double target_translation[3], const double target_rotation[4],
                         const csm_pose3d* pose, double* residuals, double* jacobian,
                         double* sums);

/* ---- submap grid formats ---------------------------------------------------
 * Submap2D::Finish (submap_2d.cc:146-150) crops a finished submap's grid to
 * its known cells: ProbabilityGrid::ComputeCroppedGrid
 * (probability_grid.cc:91-106) with Grid2D::ComputeCroppedLimits
 * (grid_2d.cc:110-120). `cells` are num_x_cells * num_y_cells uint16 values
 * (x fastest); the known box is the bounding box of the nonzero cells.
 * csm_grid2d_cropped_limits returns the cropped MapLimits and the offset
 * (x, y) of its first cell; csm_grid2d_crop also copies the cells into
 * cropped_cells (capacity >= cropped nx * ny). An all-unknown grid crops to
 * one unknown cell, as the reference does. Host-only. */
int csm_grid2d_cropped_limits(const csm_map_limits* limits, const uint16_t* cells,
                              int32_t* offset_xy, csm_map_limits* cropped);
int csm_grid2d_crop(const csm_map_limits* limits, const uint16_t* cells,
                    csm_map_limits* cropped, uint16_t* cropped_cells, int64_t capacity);

/* ---- device-resident ProbabilityGrid: range-data insertion -----------------
 * A ProbabilityGrid (mapping/2d/probability_grid.h:31-68, grid_2d.h:40-123)
 * that lives on the device, is built there by
 * ProbabilityGridRangeDataInserter2D::Insert
 * (probability_grid_range_data_inserter_2d.cc:35-98, :124-136) bit for bit, and
 * feeds both 2D matchers without a host copy. Every call is enqueued on the
 * grid's context's stream under that context's lock; a later call on the same
 * context sees it. Only csm_probability_grid_read and _finish wait for the
 * device. Grids of up to 8192 cells per side (the csm_fast2d_create limit). */
typedef struct csm_probability_grid csm_probability_grid;

/* proto::ProbabilityGridRangeDataInserterOptions2D
 * (mapping/proto/probability_grid_range_data_inserter_options_2d.proto:19-30). */
typedef struct csm_inserter2d_options {
  float hit_probability, miss_probability;
  int32_t insert_free_space;
} csm_inserter2d_options;

/* ProbabilityGrid(const MapLimits&) (probability_grid.cc:26-30): all unknown
 * when cells is NULL, else num_x_cells * num_y_cells values, x fastest. */
int csm_probability_grid_create(csm_context* ctx, const csm_map_limits* limits,
                                const uint16_t* cells_or_null, csm_probability_grid** out);
void csm_probability_grid_destroy(csm_probability_grid* grid);
/* Grid2D::limits() (grid_2d.h:51) as of the last enqueued call. */
int csm_probability_grid_limits(const csm_probability_grid* grid, csm_map_limits* out);
/* correspondence_cost_cells() (grid_2d.h:103-105): copies the cells to the
 * host (capacity >= nx * ny values) after waiting for the stream. */
int csm_probability_grid_read(const csm_probability_grid* grid, uint16_t* out, int64_t capacity);

/* ProbabilityGridRangeDataInserter2D::Insert(range_data, grid)
 * (probability_grid_range_data_inserter_2d.cc:124-136): GrowAsNeeded (:35-50,
 * Grid2D::GrowLimits, grid_2d.cc:142-175), then CastRays (:52-98) with
 * RayToPixelMask at kSubpixelScale 1000, then FinishUpdate. Points are in the
 * grid's frame. Per cell the result is hit_table[old] where a return lands,
 * else miss_table[old] where a ray's pixel mask passes (insert_free_space),
 * else old: the update marker admits one update per cell and Insert, and hits
 * come first. CSM_EINVAL: a non-finite coordinate, a probability outside
 * (0, 1), a finished grid; CSM_ERANGE: growth past 8192 cells per side. Either
 * leaves the grid as it was and enqueues nothing. */
int csm_probability_grid_insert(csm_probability_grid* grid, const csm_inserter2d_options* options,
                                const float origin_xyz[3], const float* returns_xyz,
                                int32_t num_returns, const float* misses_xyz, int32_t num_misses);

/* Many Inserts in one call, e.g. ActiveSubmaps2D::InsertRangeData's two
 * submaps (submap_2d.cc:185-196) or a rebuild of many submaps. Scan s goes
 * into grids[grid_of_scan[s]]: origin origins_xyz[3s..], returns
 * [return_offsets[s], return_offsets[s+1]) of returns_xyz, misses likewise
 * (both miss arguments NULL: none). Scans of one grid are applied in array
 * order; scans of different grids run concurrently. All grids belong to ctx
 * and are distinct. Errors as for csm_probability_grid_insert, for the whole
 * call. */
int csm_probability_grid_insert_batch(csm_context* ctx, csm_probability_grid* const* grids,
                                      int32_t num_grids, const csm_inserter2d_options* options,
                                      int32_t num_scans, const int32_t* grid_of_scan,
                                      const float* origins_xyz, const float* returns_xyz,
                                      const int64_t* return_offsets, const float* misses_xyz,
                                      const int64_t* miss_offsets);

/* Submap2D::Finish (submap_2d.cc:146-150): replaces the grid by
 * ComputeCroppedGrid() (probability_grid.cc:91-106; the known-cells box is
 * the bounding box of the nonzero cells, reduced on the device). An
 * all-unknown grid crops to 1 x 1 at offset (0, 0). Later inserts return
 * CSM_EINVAL. */
int csm_probability_grid_finish(csm_probability_grid* grid);

/* csm_fast2d_create for a device-resident grid: the pyramid is built from the
 * device cells (no host copy), everything else is shared with
 * csm_fast2d_create. The grid may be inserted into or destroyed afterwards. */
int csm_fast2d_create_from_grid(csm_context* ctx, const csm_probability_grid* grid,
                                const csm_fast2d_options* options, csm_fast2d** out);

/* csm_rt2d_match for a device-resident grid of ctx. The converted grid is
 * cached per (grid id, generation, padding): every insert, growth and finish
 * bumps the generation. */
int csm_rt2d_match_grid(csm_context* ctx, const csm_rt_options* options,
                        const csm_probability_grid* grid, const csm_pose2d* initial,
                        const float* points_xyz, int32_t n, double* score, csm_pose2d* pose);

/* Test-visible, like csm_fast2d_read_level: RayToPixelMask
 * (mapping/internal/2d/ray_to_pixel_mask.cc:29-159) for a batch of rays, the
 * device function the inserter marks cells with. Ray r is (begin.x, begin.y,
 * end.x, end.y) in subpixel units, all in [0, 2^30). ray_offsets (num_rays + 1)
 * receives the cell offsets; cells_xy (may be NULL: offsets only; capacity in
 * cells >= ray_offsets[num_rays]) receives each ray's cells (x, y) in the
 * reference's order, begin and end swapped so that begin.x <= end.x. */
int csm_ray_to_pixel_mask(csm_context* ctx, const int32_t* begin_end_xyxy, int32_t num_rays,
                          int32_t subpixel_scale, int32_t* cells_xy, int64_t capacity,
                          int64_t* ray_offsets);
/* ComputeLookupTableToApplyCorrespondenceCostOdds(Odds(probability))
 * (probability_values.cc:89-106): 32768 entries, update marker included.
 * Host-only. */
int csm_inserter2d_lookup_table(float probability, uint16_t* out /* [32768] */);

/* ---- device-resident TSDF2D: TSDF range-data insertion ----------------------
 * A TSDF2D (mapping/internal/2d/tsdf_2d.h:34-78: a TSD plane and a weight
 * plane of uint16 values over one MapLimits) that lives on the device, is
 * built there by TSDFRangeDataInserter2D::Insert
 * (tsdf_range_data_inserter_2d.cc:131-240) bit for bit, and feeds the
 * real-time matcher without a host copy. Calls are enqueued on the grid's
 * context's stream under that context's lock, as for csm_probability_grid;
 * only csm_tsdf_grid_read and _finish wait for the device. Up to 8192 cells
 * per side. */
typedef struct csm_tsdf_grid csm_tsdf_grid;

/* proto::TSDFRangeDataInserterOptions2D
 * (mapping/proto/tsdf_range_data_inserter_options_2d.proto:19-55, with its
 * NormalEstimationOptions2D), in the proto's types; the casts to float happen
 * where the reference casts. */
typedef struct csm_tsdf_inserter_options {
  double truncation_distance;
  double maximum_weight;
  int32_t update_free_space;
  int32_t num_normal_samples;
  double sample_radius;
  int32_t project_sdf_distance_to_scan_normal;
  int32_t update_weight_range_exponent;
  double update_weight_angle_scan_normal_to_ray_kernel_bandwidth;
  double update_weight_distance_cell_to_hit_kernel_bandwidth;
} csm_tsdf_inserter_options;

/* TSDF2D(limits, truncation_distance, max_weight, tables) (tsdf_2d.cc:23-34):
 * all unknown when both cell arrays are NULL, else both hold
 * num_x_cells * num_y_cells values, x fastest (tsdf_2d.cc:36-48). One array
 * alone, or a truncation distance or maximum weight <= 0: CSM_EINVAL. */
int csm_tsdf_grid_create(csm_context* ctx, const csm_map_limits* limits,
                         float truncation_distance, float max_weight,
                         const uint16_t* tsd_cells_or_null, const uint16_t* weight_cells_or_null,
                         csm_tsdf_grid** out);
void csm_tsdf_grid_destroy(csm_tsdf_grid* grid);
/* Grid2D::limits() (grid_2d.h:51) as of the last enqueued call. */
int csm_tsdf_grid_limits(const csm_tsdf_grid* grid, csm_map_limits* out);
/* correspondence_cost_cells() and the weight cells (tsdf_2d.h:76): copies both
 * planes to the host (capacity >= nx * ny values each) after waiting for the
 * stream. */
int csm_tsdf_grid_read(const csm_tsdf_grid* grid, uint16_t* tsd_out, uint16_t* weight_out,
                       int64_t capacity);

/* TSDFRangeDataInserter2D::Insert(range_data, grid)
 * (tsdf_range_data_inserter_2d.cc:131-165): GrowAsNeeded (:33-47), the
 * RangeDataSorter (:69-88) and EstimateNormals (normal_estimation_2d.cc:74-109)
 * when the options ask for normals, InsertHit per return in that order
 * (:167-225) and FinishUpdate. Misses are ignored by the reference, so none
 * are passed. A cell is written by the first ray, in the reference's order,
 * whose pixel mask holds it with a non-zero update weight (TSDF2D::SetCell,
 * tsdf_2d.cc:56-69; UpdateCell, :227-239). With zero returns the limits still
 * grow around the origin. CSM_EINVAL: a non-finite coordinate, a truncation
 * distance or maximum weight <= 0, a negative num_normal_samples, a finished
 * grid; CSM_ERANGE: growth past 8192 cells per side. Either leaves the grid as
 * it was and enqueues nothing. */
int csm_tsdf_grid_insert(csm_tsdf_grid* grid, const csm_tsdf_inserter_options* options,
                         const float origin_xyz[3], const float* returns_xyz,
                         int32_t num_returns);

/* Many Inserts in one call, e.g. ActiveSubmaps2D::InsertRangeData's two
 * submaps (submap_2d.cc:171-182). Arguments as for
 * csm_probability_grid_insert_batch without the misses: scans of one grid are
 * applied in array order, scans of different grids run concurrently in
 * rounds. */
int csm_tsdf_grid_insert_batch(csm_context* ctx, csm_tsdf_grid* const* grids, int32_t num_grids,
                               const csm_tsdf_inserter_options* options, int32_t num_scans,
                               const int32_t* grid_of_scan, const float* origins_xyz,
                               const float* returns_xyz, const int64_t* return_offsets);

/* Submap2D::Finish (submap_2d.cc:146-150): replaces the grid by
 * TSDF2D::ComputeCroppedGrid() (tsdf_2d.cc:118-135): the known-cells box is
 * the bounding box of the cells whose TSD value is not 0, and every known
 * cell goes through SetCell(GetTSD, GetWeight) once more. An all-unknown grid
 * crops to 1 x 1 at offset (0, 0). Later inserts return CSM_EINVAL. */
int csm_tsdf_grid_finish(csm_tsdf_grid* grid);

/* csm_fast2d_create for a TSDF2D (GridType::TSDF): the
 * PrecomputationGridStack2D is built from the TSD cells exactly as
 * csm_fast2d_create builds it, with Grid2D's bounds of a TSDF2D, min = -trunc
 * and max = +trunc (tsdf_2d.cc:24-27; fast_correlative_scan_matcher_2d.cc:
 * 97-98, :105-160). The handle also keeps the weights, for the TSDF match cost
 * of csm_ceres2d_refine_batch. csm_fast2d_match, _match_full_submap,
 * _match_batch and _read_level work on it unchanged. Arrays as for
 * csm_rt2d_match_tsdf, copied. Errors as for csm_fast2d_create; one array
 * without the other, or a truncation distance or max weight <= 0: CSM_EINVAL. */
int csm_fast2d_create_tsdf(csm_context* ctx, const csm_map_limits* limits,
                           const uint16_t* tsd_cells, const uint16_t* weight_cells,
                           float truncation_distance, float max_weight,
                           const csm_fast2d_options* options, csm_fast2d** out);
/* The same from a device-resident TSDF2D, without a host copy. The grid may be
 * inserted into or destroyed afterwards, as for csm_fast2d_create_from_grid. */
int csm_fast2d_create_from_tsdf_grid(csm_context* ctx, const csm_tsdf_grid* grid,
                                     const csm_fast2d_options* options, csm_fast2d** out);

/* csm_rt2d_match_tsdf for a device-resident TSDF2D of ctx
 * (real_time_correlative_scan_matcher_2d.cc:38-59, :117-149). The converted
 * (term, weight) grid is cached per (grid id, generation, padding). */
int csm_rt2d_match_tsdf_grid(csm_context* ctx, const csm_rt_options* options,
                             const csm_tsdf_grid* grid, const csm_pose2d* initial,
                             const float* points_xyz, int32_t n, double* score, csm_pose2d* pose);

/* CeresScanMatcher2D::Match(target_translation, initial, cloud, grid, &pose)
 * (ceres_scan_matcher_2d.cc:64-105) on a device-resident grid of ctx, as
 * LocalTrajectoryBuilder2D::ScanMatch calls it on the active submap
 * (local_trajectory_builder_2d.cc:63-97): no pyramid is built and no plane is
 * converted, the kernel reads the uint16 cells through the value tables.
 * Validation as for csm_ceres2d_refine_batch; n >= 1 finite points.
 * iterations_out may be NULL. summary.final_cost is not returned. */
int csm_ceres2d_match_grid(csm_context* ctx, const csm_ceres2d_options* options,
                           const csm_probability_grid* grid, const double target_xy[2],
                           const csm_pose2d* initial, const float* points_xyz, int32_t n,
                           csm_pose2d* pose_out, int32_t* iterations_out);
int csm_ceres2d_match_tsdf_grid(csm_context* ctx, const csm_ceres2d_options* options,
                                const csm_tsdf_grid* grid, const double target_xy[2],
                                const csm_pose2d* initial, const float* points_xyz, int32_t n,
                                csm_pose2d* pose_out, int32_t* iterations_out);

/* Test-visible: csm_ceres2d_evaluate on a device-resident grid of ctx, through
 * the instantiation csm_ceres2d_match_grid runs (uint16 cells through the
 * value table). */
int csm_ceres2d_evaluate_grid(csm_context* ctx, const csm_probability_grid* grid,
                              const csm_ceres2d_options* options, const double target_xy[2],
                              double target_theta, const csm_pose2d* pose, const float* points_xyz,
                              int32_t n, double* residuals, double* jacobian, double* sums);

/* Test-visible and host-only, like csm_inserter2d_lookup_table: the per-ray
 * plan of one Insert that the device consumes. order[k] is the index of the
 * return cast as ray k (std::sort with the RangeDataSorter's comparator,
 * :69-88; the identity when the options need no normals), normals[k] its
 * estimated normal (NaN without normals), ray_weight[k] the float product of
 * the range and angle weight factors (:205-214, :81-87), cast[k] 0 where the
 * range is below the truncation distance (:174), else 1. Each output holds n
 * entries; any may be NULL. */
int csm_tsdf_plan_scan(const csm_tsdf_inserter_options* options, const float origin_xyz[3],
                       const float* returns_xyz, int32_t n, int32_t* order_out,
                       float* normals_out, float* ray_weight_out, uint8_t* cast_out);
/* Test-visible, host-only: the two round-trip tables Finish copies through,
 * TSDToValue(ValueToTSD(v)) and WeightToValue(ValueToWeight(v))
 * (tsd_value_converter.h:33-50), 32768 entries each. */
int csm_tsdf_round_trip_tables(float truncation_distance, float max_weight,
                               uint16_t* tsd_out /* [32768] */, uint16_t* weight_out /* [32768] */);

/* ---- device-resident HybridGrid: 3D range-data insertion --------------------
 * RangeDataInserter3D::Insert (mapping/3d/range_data_inserter_3d.cc:44-74,
 * :109-137) on the device brick of a csm_hybrid_grid, bit for bit: a grid
 * made by csm_hybrid_grid_create (an empty one, count 0, included) is updated
 * where it lives, and csm_rt3d_match, csm_hybrid_grid_get_probability,
 * csm_hybrid_grid_interpolate, csm_ceres3d_refine_batch and later
 * csm_fast3d_create calls see the new values without a host copy. Every call
 * is enqueued on the grid's context's stream under that context's lock and
 * re-records the grid's ready event; only csm_hybrid_grid_read and
 * csm_hybrid_grid_insert_stats wait for the device.
 *
 * After every insert csm_hybrid_grid_info reports exactly the bounding box of
 * the known cells and DynamicGrid's size (hybrid_grid.h:283-296, :384-399):
 * what csm_hybrid_grid_create would derive from the reference grid's iterator
 * list. A grid whose box grows is moved into a new brick on the device.
 *
 * One limit, as in the reference, where matchers are built from finished
 * submaps only (constraint_builder_3d.cc:170-198): inserting into a grid that
 * a live csm_fast3d was built from, or holds as its low-resolution grid, is
 * not supported. Calls that read a grid from another context's stream must
 * not overlap an insert into it. The intensity grid (IntensityHybridGrid,
 * range_data_inserter_3d.cc:76-89) is a handle of its own, csm_intensity_grid
 * below, filled by csm_hybrid_grid_insert_intensities*. */

/* proto::RangeDataInserterOptions3D
 * (mapping/proto/range_data_inserter_options_3d.proto); the intensity
 * threshold is an argument of csm_hybrid_grid_insert_intensities*. */
typedef struct csm_inserter3d_options {
  float hit_probability, miss_probability;
  int32_t num_free_space_voxels;
} csm_inserter3d_options;

/* RangeDataInserter3D::Insert(range_data, hybrid_grid)
 * (range_data_inserter_3d.cc:109-137): every return's cell (GetCellIndex,
 * hybrid_grid.h:428-433) takes hit_table[old]; then, per ray, the last
 * num_free_space_voxels cells origin_cell + delta * position / num_samples
 * before the hit (InsertMissesIntoGrid, :44-74) take miss_table[old] unless
 * already updated in this call (ApplyLookupTable's update marker,
 * hybrid_grid.h:497-513); FinishUpdate (:515-521). Points are in the grid's
 * frame. CSM_EINVAL: a non-finite coordinate, a probability outside (0, 1), a
 * negative num_free_space_voxels. CSM_ERANGE: a ray of 2^15 cells or more
 * (the reference's CHECK_LT, :58) or a brick past 2^31 cells. Either leaves
 * the grid as it was and enqueues nothing. */
int csm_hybrid_grid_insert(csm_hybrid_grid* grid, const csm_inserter3d_options* options,
                           const float origin_xyz[3], const float* returns_xyz,
                           int32_t num_returns);

/* Many Inserts in one call: Submap3D::InsertData (submap_3d.cc:323-347) for
 * the two active submaps, four grids, is one call. The scans go up once, in
 * the local frame: scan s has origin origins_xyz[3s..] and returns
 * [return_offsets[s], return_offsets[s+1]) of returns_xyz. Job k inserts scan
 * scan_of_job[k] into grids[grid_of_job[k]], after
 *  - transform_of_job[k] >= 0: sensor::TransformRangeData by the Rigid3f
 *    transforms[7 t..] (translation, then rotation w, x, y, z; submap from
 *    local), applied to the origin and every return as Rigid3f * Vector3f
 *    (rigid_transform.h:191-196). transform_of_job NULL: no job has one.
 *  - max_ranges[k] > 0: FilterRangeDataByMaxRange (submap_3d.cc:91-99), which
 *    keeps a return when (p - origin).norm() <= max_range in float, after the
 *    transform. max_ranges NULL: no job filters.
 * Jobs on one grid are applied in array order; jobs on different grids run
 * concurrently. All grids belong to ctx and are distinct. Errors as for
 * csm_hybrid_grid_insert, for the whole call. */
int csm_hybrid_grid_insert_batch(csm_context* ctx, csm_hybrid_grid* const* grids,
                                 int32_t num_grids, const csm_inserter3d_options* options,
                                 int32_t num_scans, const float* origins_xyz,
                                 const float* returns_xyz, const int64_t* return_offsets,
                                 int32_t num_jobs, const int32_t* grid_of_job,
                                 const int32_t* scan_of_job, const float* transforms,
                                 int32_t num_transforms, const int32_t* transform_of_job,
                                 const float* max_ranges);

/* ---- device-resident IntensityHybridGrid ------------------------------------
 * IntensityHybridGrid (hybrid_grid.h:547-571) in the shape csm_hybrid_grid has:
 * a dense brick, x fastest, over the bounding box of the cells with count > 0,
 * in two planes, the float sum and the int32 count of AverageIntensityData.
 * The bricks come from the context's pool, every insert is enqueued on the
 * context's stream and re-records the grid's ready event. create makes the
 * empty grid (no device call); destroy is what ActiveSubmaps3D does when it
 * forgets a finished submap's intensity grid (submap_3d.cc:396-405). */
int csm_intensity_grid_create(csm_context* ctx, float resolution, csm_intensity_grid** out);
void csm_intensity_grid_destroy(csm_intensity_grid* grid);
/* The box of the cells with count > 0 (dims 0 while there is none) and the
 * size DynamicGrid::Grow has reached (128 at first), exact after every insert. */
int csm_intensity_grid_info(const csm_intensity_grid* grid, int32_t* origin3, int32_t* dims3,
                            int32_t* grid_size);
/* The sums and counts over that box, capacity >= nx * ny * nz each. Waits for
 * the stream. */
int csm_intensity_grid_read(const csm_intensity_grid* grid, float* sums_out, int32_t* counts_out,
                            int64_t capacity);
/* IntensityHybridGrid::GetIntensity at n cell indices, on the device: sum /
 * count in one float division, 0 for a cell with count 0 or outside the box. */
int csm_intensity_grid_get_intensity(const csm_intensity_grid* grid, const int32_t* xyz_indices,
                                     int64_t n, float* out);
int64_t csm_intensity_grid_device_bytes(const csm_intensity_grid* grid);

/* RangeDataInserter3D::Insert(range_data, hybrid_grid, intensity_hybrid_grid)
 * (range_data_inserter_3d.cc:117-137). The HybridGrid is updated by the code
 * of csm_hybrid_grid_insert, so its bytes are the same. Then
 * InsertIntensitiesIntoGrid (:76-89): every return with !(intensity >
 * intensity_threshold) adds 1 to the count and its intensity to the sum of
 * the cell intensity_grid's own GetCellIndex gives it (the two resolutions
 * may differ, as in the reference). A cell's new sum is ((old + v_a) + v_b) +
 * ... in float, a < b < ... the indices of its returns, as the reference's
 * loop leaves it: the returns are sorted by cell on the device with their
 * order kept and one thread adds a cell's run, so the result is the same on
 * every run; no float atomic is used. intensities NULL (a cloud without
 * intensities, :79) or intensity_grid NULL: the intensity grid is left alone.
 * CSM_EINVAL also for a non-finite intensity or a NaN threshold, CSM_ERANGE
 * also for an intensity brick past 2^31 cells; either leaves both grids as
 * they were and enqueues nothing. */
int csm_hybrid_grid_insert_intensities(csm_hybrid_grid* grid, csm_intensity_grid* intensity_grid,
                                       const csm_inserter3d_options* options,
                                       float intensity_threshold, const float origin_xyz[3],
                                       const float* returns_xyz, const float* intensities,
                                       int32_t num_returns);

/* csm_hybrid_grid_insert_batch with intensities: scan s has the intensities
 * scan_intensities[s][0 .. its number of returns), or none where that pointer
 * (or scan_intensities itself) is NULL. Job k adds them to
 * intensity_grids[intensity_grid_of_job[k]] (-1, or intensity_grid_of_job
 * NULL: to none) after its transform and under its max_range mask, as
 * PointCloud::copy_if keeps them (point_cloud.h:60-84). The intensity grids
 * belong to ctx and are distinct, and within one call every job of an
 * intensity grid names the same HybridGrid (a submap's high-resolution grid,
 * submap_3d.cc:332-339): jobs on it are applied in array order with that
 * grid's. */
int csm_hybrid_grid_insert_intensities_batch(
    csm_context* ctx, csm_hybrid_grid* const* grids, int32_t num_grids,
    csm_intensity_grid* const* intensity_grids, int32_t num_intensity_grids,
    const csm_inserter3d_options* options, float intensity_threshold, int32_t num_scans,
    const float* origins_xyz, const float* returns_xyz, const int64_t* return_offsets,
    const float* const* scan_intensities, int32_t num_jobs, const int32_t* grid_of_job,
    const int32_t* scan_of_job, const int32_t* intensity_grid_of_job, const float* transforms,
    int32_t num_transforms, const int32_t* transform_of_job, const float* max_ranges);

/* The uint16 values of the device brick (x fastest) over the box
 * csm_hybrid_grid_info reports, capacity >= nx * ny * nz values: with the box
 * origin, what HybridGrid's iterator / ToProto yields (hybrid_grid.h:530-541;
 * unknown cells are 0). Waits for the stream. */
int csm_hybrid_grid_read(const csm_hybrid_grid* grid, uint16_t* values_out, int64_t capacity);

/* Test-visible, like csm_fast3d_read_level: totals over the grid's inserts of
 * the cells the FinishUpdate pass looked at (one per return and per miss
 * position, duplicates included) and of the cells it updated. The pass walks
 * the returns again, never the brick. Waits for the stream. */
int csm_hybrid_grid_insert_stats(const csm_hybrid_grid* grid, int64_t* cells_visited,
                                 int64_t* cells_updated);

/* ComputeLookupTableToApplyOdds(Odds(probability))
 * (probability_values.cc:76-87): 32768 entries, update marker included.
 * Host-only. */
int csm_inserter3d_lookup_table(float probability, uint16_t* out /* [32768] */);

/* RotationalScanMatcher::RotateHistogram(histogram, angle)
 * (rotational_scan_matcher.cc:138-158), which Submap3D::InsertData adds to
 * the submap's histogram (submap_3d.cc:341-346). out may be histogram.
 * Host-only. */
int csm_rotate_histogram(const float* histogram, int32_t size, float angle, float* out);

/* RotationalScanMatcher::ComputeHistogram(point_cloud, histogram_size)
 * (rotational_scan_matcher.cc:160-171 with AddValueToHistogram :34-49,
 * ComputeCentroid :51-58, AddPointCloudSliceToHistogram :60-88 and
 * SortSlice :92-117): the histogram LocalTrajectoryBuilder3D::InsertIntoSubmap
 * makes of a node's gravity-aligned returns (local_trajectory_builder_3d.cc:
 * 898-903). points_xyz holds n points (x, y, z); out receives histogram_size
 * floats. The same slices (a map keyed by RoundToInt(z / 0.2)), the same
 * std::sort by the angle about the slice's centroid, the same float order, so
 * the result is the reference's bit for bit on a host whose atan2f is the
 * reference's. Host-only on purpose (it takes no context): its atan2f is the
 * C library's. CSM_EINVAL: n < 0, histogram_size <= 0, a null pointer. */
int csm_compute_histogram(const float* points_xyz, int64_t n, int32_t histogram_size, float* out);

/* ---- node clouds: voxel filters -------------------------------------------
 * sensor::VoxelFilter and sensor::AdaptiveVoxelFilter
 * (sensor/internal/voxel_filter.h, voxel_filter.cc:212-232 and :263-268), the
 * filters that make the clouds the matchers search with
 * (local_trajectory_builder_2d.cc:61-62, :229-231;
 * local_trajectory_builder_3d.cc:682-683, :735-748). A batch of clouds: cloud
 * c is points [offsets[c], offsets[c+1]) of xyz (float x, y, z). keep[i] = 1
 * when point i survives; the reference returns the survivors in input order
 * and filters intensities with the same mask. counts[c] = survivors of cloud c
 * (may be NULL). The kept set is the reference's exactly (same voxel keys, same
 * minstd_rand0 reservoir draws). Clouds of up to 8192 points (larger:
 * CSM_ERANGE). */
typedef struct csm_adaptive_voxel_filter_options {
  /* proto::AdaptiveVoxelFilterOptions
   * (sensor/proto/adaptive_voxel_filter_options.proto): all floats. */
  float max_length;
  float min_num_points;
  float max_range;
} csm_adaptive_voxel_filter_options;

int csm_voxel_filter(csm_context* ctx, const float* xyz, const int64_t* offsets,
                     int32_t num_clouds, float resolution, uint8_t* keep, int32_t* counts);
int csm_adaptive_voxel_filter(csm_context* ctx, const float* xyz, const int64_t* offsets,
                              int32_t num_clouds, const csm_adaptive_voxel_filter_options* options,
                              uint8_t* keep, int32_t* counts);
/* The same on device-resident buffers (d_offsets relative to d_xyz), enqueued
 * on the context's stream without synchronising; max_points bounds every
 * cloud's size. */
int csm_voxel_filter_device(csm_context* ctx, const float* d_xyz, const int64_t* d_offsets,
                            int32_t num_clouds, int32_t max_points, float resolution,
                            uint8_t* d_keep, int32_t* d_counts);
int csm_adaptive_voxel_filter_device(csm_context* ctx, const float* d_xyz,
                                     const int64_t* d_offsets, int32_t num_clouds,
                                     int32_t max_points,
                                     const csm_adaptive_voxel_filter_options* options,
                                     uint8_t* d_keep, int32_t* d_counts);

/* The same two filters for one cloud of up to 2^20 points (larger: CSM_ERANGE,
 * checked before the device is touched), the size of a 3D sweep
 * (local_trajectory_builder_3d.cc:680-683 filters the accumulated returns,
 * :734-745 the returns in the tracking frame; the reference's own
 * LocalTrajectoryBuilderTest feeds 16 000 points per scan). The kept set is
 * RandomizedVoxelFilterIndices' (voxel_filter.cc:136-162) exactly, and the
 * adaptive filter is FilterByMaxRange (:31-36), AdaptivelyVoxelFiltered
 * (:38-76) and AdaptiveVoxelFilter (:263-268) exactly, whatever the size: the
 * cloud lives in global memory, sorted by voxel key with a device radix sort.
 * keep[i] = 1 for a surviving point; *count = survivors. n == 0: CSM_OK and a
 * zero count. CSM_EINVAL: a null pointer with n > 0, a null count,
 * resolution <= 0, max_length <= 0. Working memory is kept with the context
 * and grows on demand. */
int csm_voxel_filter_large(csm_context* ctx, const float* xyz, int64_t n, float resolution,
                           uint8_t* keep, int64_t* count);
int csm_adaptive_voxel_filter_large(csm_context* ctx, const float* xyz, int64_t n,
                                    const csm_adaptive_voxel_filter_options* options,
                                    uint8_t* keep, int64_t* count);

/* ---- range data: the front end of LocalTrajectoryBuilder2D ------------------
 * From one accumulated sweep of rangefinder points to what the inserters and
 * the scan matchers take (mapping/internal/2d/local_trajectory_builder_2d.cc).
 * Rigid3f arguments are (t x y z, q w x y z). All arithmetic is float, not
 * contracted, in Eigen's order, so every output float is the reference's bit
 * for bit, and every output cloud is in input order. */
typedef struct csm_range_data2d_options {
  /* proto::LocalTrajectoryBuilderOptions2D
   * (mapping/proto/local_trajectory_builder_options_2d.proto): all floats. */
  float min_range;
  float max_range;
  float missing_data_ray_length;
  float min_z;
  float max_z;
  float voxel_filter_size;
  csm_adaptive_voxel_filter_options adaptive_voxel_filter;
} csm_range_data2d_options;

/* AddRangeData's range loop (local_trajectory_builder_2d.cc:163-185),
 * TransformToGravityAlignedFrameAndFilter (:51-63) and the AdaptiveVoxelFilter
 * of AddAccumulatedRangeData (:228-231), in one upload, one chain of launches
 * and one download. Point i is hits_xyz[3 i ..] measured from
 * origins_xyz[3 origin_index[i] ..], both moved by poses_tq[7 i ..]
 * (range_data_poses[i]): dropped below min_range (or with a NaN range), a
 * return up to max_range, else a miss at missing_data_ray_length along the
 * ray. Returns and misses are moved by gravity_from_local_tq
 * (transform_to_gravity_aligned_frame), cropped to min_z <= z <= max_z
 * (sensor/point_cloud.cc:76-81) and voxel-filtered: returns_out / misses_out
 * with num_returns / num_misses points; origin_out is local_origin_xyz
 * (range_data_poses.back().translation()) moved likewise. filtered_out /
 * num_filtered is AdaptiveVoxelFilter(returns_out). Each output cloud needs
 * room for n points. n up to 8192 (larger: CSM_ERANGE); n == 0 gives zero
 * counts. CSM_EINVAL: a null pointer with n > 0, an origin_index outside
 * [0, num_origins), voxel_filter_size <= 0 or a non-positive adaptive
 * max_length. */
int csm_range_data2d_prepare(csm_context* ctx, const csm_range_data2d_options* options,
                             const float* hits_xyz, const int32_t* origin_index,
                             const float* poses_tq, int32_t n, const float* origins_xyz,
                             int32_t num_origins, const float gravity_from_local_tq[7],
                             const float local_origin_xyz[3], float origin_out[3],
                             float* returns_out, int32_t* num_returns, float* misses_out,
                             int32_t* num_misses, float* filtered_out, int32_t* num_filtered);

/* ---- range data: the front end of LocalTrajectoryBuilder3D ------------------ */
typedef struct csm_range_data3d_options {
  /* proto::LocalTrajectoryBuilderOptions3D
   * (mapping/proto/local_trajectory_builder_options_3d.proto). */
  float min_range;
  float max_range;
  float voxel_filter_size;
  csm_adaptive_voxel_filter_options high_resolution_adaptive_voxel_filter;
  csm_adaptive_voxel_filter_options low_resolution_adaptive_voxel_filter;
} csm_range_data3d_options;

/* AddRangeData's range loop (local_trajectory_builder_3d.cc:636-669), the two
 * VoxelFilter calls (:680-683), TransformRangeData by tracking_from_local
 * (:696-698) and the two AdaptiveVoxelFilter calls of AddAccumulatedRangeData
 * on the transformed returns (:734-745), in one upload, one chain of launches
 * and one download. Point i is hits_xyz[3 i ..] measured from
 * origins_xyz[3 origin_index[i] ..], both moved by poses_tq[7 i ..]: dropped
 * below min_range (or with a NaN range), a return up to max_range carrying
 * intensities[i], else a miss at origin + (max_range / range) * delta (the 3D
 * builder crops the ray to max_range). Returns and misses are voxel-filtered
 * at voxel_filter_size and moved by tracking_from_local_tq
 * (current_pose.inverse().cast<float>()): returns_out / misses_out;
 * origin_out is local_origin_xyz (current_pose.translation().cast<float>())
 * moved likewise. high_out / low_out are AdaptiveVoxelFilter(returns_out) with
 * the two option sets. Intensities follow their points through every filter;
 * intensities == NULL: none, and the intensity outputs are not written (they
 * may be NULL). Every output cloud is in input order and needs room for n
 * points. n up to 2^20 (larger: CSM_ERANGE); n == 0 gives zero counts.
 * CSM_EINVAL: a null pointer with n > 0, an origin_index outside
 * [0, num_origins), voxel_filter_size <= 0 or a non-positive max_length. */
int csm_range_data3d_prepare(csm_context* ctx, const csm_range_data3d_options* options,
                             const float* hits_xyz, const float* intensities,
                             const int32_t* origin_index, const float* poses_tq, int32_t n,
                             const float* origins_xyz, int32_t num_origins,
                             const float tracking_from_local_tq[7],
                             const float local_origin_xyz[3], float origin_out[3],
                             float* returns_out, float* returns_intensities_out,
                             int32_t* num_returns, float* misses_out, int32_t* num_misses,
                             float* high_out, float* high_intensities_out, int32_t* num_high,
                             float* low_out, float* low_intensities_out, int32_t* num_low);

/* sensor::TransformRangeData (sensor/range_data.cc:25-32) by a Rigid3f: the
 * origin, the returns and the misses (local_trajectory_builder_2d.cc:246-248
 * moves the gravity-aligned range data by Embed3D(pose_estimate_2d) before the
 * insert). The outputs may not alias the inputs. */
int csm_range_data_transform(csm_context* ctx, const float transform_tq[7],
                             const float origin_xyz[3], const float* returns_xyz,
                             int32_t num_returns, const float* misses_xyz, int32_t num_misses,
                             float origin_out[3], float* returns_out, float* misses_out);

/* ---- pbstream ingest --------------------------------------------------------
 * Reads a serialized state file (io/proto_stream.cc:26-86: magic, then per
 * message an 8-byte size and a gzip member; SerializationHeader then
 * SerializedData, mapping/proto/serialization.proto:72-88) and keeps what a
 * ConstraintBuilder2D needs: every Submap2D (id, local pose, finished flag,
 * Grid2D as in Grid2D::Grid2D(proto), mapping/2d/grid_2d.cc:75-96) and every
 * Node (id, timestamp, gravity alignment, local pose and the decompressed
 * filtered_gravity_aligned_point_cloud, sensor/compressed_point_cloud.cc:79-97).
 * Poses are (tx, ty, tz, qw, qx, qy, qz); gravity_alignment is (w, x, y, z).
 * 3D submaps and the nodes' 3D clouds are kept too (below). Other message
 * kinds (pose graph, options, sensor data) are skipped. Host-only; returns CSM_EINVAL for a malformed file. Pass NULL for
 * any output not wanted; cells / xyz need capacity >= the item's size
 * (CSM_ERANGE otherwise). */
typedef struct csm_pbstream csm_pbstream;
int csm_pbstream_open(const char* path, csm_pbstream** out);
void csm_pbstream_close(csm_pbstream* stream);
uint32_t csm_pbstream_format_version(const csm_pbstream* stream);
int32_t csm_pbstream_num_submaps2d(const csm_pbstream* stream);
int32_t csm_pbstream_num_nodes(const csm_pbstream* stream);
/* ids = (trajectory_id, submap_index); min_max_cc = (min, max)
 * correspondence cost; cells are num_x_cells * num_y_cells values, x fastest. */
int csm_pbstream_submap2d(const csm_pbstream* stream, int32_t index, int32_t* ids,
                          csm_map_limits* limits, float* min_max_cc, int32_t* finished,
                          double* local_pose7, uint16_t* cells, int64_t capacity);
/* ids = (trajectory_id, node_index); capacity and num_points count points. */
int csm_pbstream_node(const csm_pbstream* stream, int32_t index, int32_t* ids,
                      int64_t* timestamp, double* local_pose7, double* gravity_alignment,
                      float* xyz, int64_t capacity, int32_t* num_points);
/* A node's clouds: which = 0 filtered_gravity_aligned_point_cloud (what
 * csm_pbstream_node returns), 1 high_resolution_point_cloud, 2
 * low_resolution_point_cloud (the 3D matcher's inputs); and its
 * rotational_scan_matcher_histogram (size = number of buckets). */
int csm_pbstream_node_cloud(const csm_pbstream* stream, int32_t index, int32_t which, float* xyz,
                            int64_t capacity, int32_t* num_points);
int csm_pbstream_node_histogram(const csm_pbstream* stream, int32_t index, float* histogram,
                                int32_t capacity, int32_t* size);
/* Submap3D (submap.proto:32-39): ids, finished, local pose, the cell counts of
 * its (high, low) resolution HybridGrids and its histogram size. A grid's
 * cells come back as csm_hybrid_grid_create takes them (xyz_indices 3 per
 * cell, uint16 values as HybridGrid(proto) stores them, hybrid_grid.h:473-484);
 * which = 0 high, 1 low resolution. */
int32_t csm_pbstream_num_submaps3d(const csm_pbstream* stream);
int csm_pbstream_submap3d(const csm_pbstream* stream, int32_t index, int32_t* ids,
                          int32_t* finished, double* local_pose7, int64_t* num_cells,
                          int32_t* histogram_size);
int csm_pbstream_submap3d_grid(const csm_pbstream* stream, int32_t index, int32_t which,
                               float* resolution, int32_t* xyz_indices, uint16_t* values,
                               int64_t capacity);
int csm_pbstream_submap3d_histogram(const csm_pbstream* stream, int32_t index, float* histogram,
                                    int32_t capacity);

/* ---- Multi-GPU hand-off ------------------------------------
 * The constraint queue shards across ranks (one process per GPU) with no
 * data-path collective; the one exchange is gathering every rank's accepted
 * constraints to rank 0 for the CPU pose-graph solve, where WhenDone's
 * submission order is restored (constraint_builder_2d.cc:279-300 delivers
 * results in submission order through one callback). The reference runs one
 * process and has no counterpart; these calls are what a sharded
 * ConstraintBuilder2D (include/cartographer_amd/constraint_builder_2d.h,
 * set_communicator) uses. Transports: RCCL over xGMI (rank r on its context's
 * device; rank 0 makes the id with csm_comm_get_unique_id and the caller
 * distributes it) or TCP between host processes (CPU tests, rehearsals). */
#define CSM_COMM_ID_BYTES 128
#define CSM_REDUCE_SUM 0
#define CSM_REDUCE_MAX 1
typedef struct csm_comm csm_comm;
int csm_comm_get_unique_id(uint8_t* id /* CSM_COMM_ID_BYTES */);
int csm_comm_create_rccl(csm_context* ctx, int32_t rank, int32_t world_size, const uint8_t* id,
                         csm_comm** out);
/* Rank 0 listens on `port`; the others connect to root_host:port. */
int csm_comm_create_tcp(int32_t rank, int32_t world_size, const char* root_host, int32_t port,
                        csm_comm** out);
void csm_comm_destroy(csm_comm* comm);
int32_t csm_comm_rank(const csm_comm* comm);
int32_t csm_comm_size(const csm_comm* comm);
/* Collective: every rank contributes send_bytes; rank 0 keeps all blobs in
 * rank order (total in *total_bytes, 0 on other ranks) and copies them out
 * with csm_comm_gathered (sizes: world_size entries, bytes per rank). */
int csm_comm_gather(csm_comm* comm, const void* send, int64_t send_bytes, int64_t* total_bytes);
int csm_comm_gathered(const csm_comm* comm, void* out, int64_t capacity, int64_t* sizes);
/* Collective: element-wise sum or max over ranks, in place. */
int csm_comm_allreduce_i64(csm_comm* comm, int64_t* values, int32_t count, int32_t op);
int csm_comm_barrier(csm_comm* comm);
/* Dynamic work claiming: the shared queue of the reference's
 * common::ThreadPool (thread_pool.cc:80-106, idle workers take the next task;
 * ConstraintBuilder2D schedules one task per pair, constraint_builder_2d.cc:102-111)
 * stretched over ranks. claim_open is collective: rank 0 serves a table of
 * int64 counters from a host thread on `port`, the others connect to
 * root_host:port (any transport; a world of 1 keeps the table locally).
 * fetch_add is NOT collective: *old_value = counter[key], counter[key] += delta,
 * atomically across ranks; counters start at 0. */
int csm_comm_claim_open(csm_comm* comm, const char* root_host, int32_t port);
int csm_comm_fetch_add(csm_comm* comm, int64_t key, int64_t delta, int64_t* old_value);

/* ---- OptimizationProblem2D: the sparse pose-graph solve ----------------------
 * The part of OptimizationProblem2D::Solve
 * (mapping/internal/optimization/optimization_problem_2d.cc:240-409) built from
 * submaps, nodes and constraints, as a flat problem: V vertices of (x, y,
 * angle) and E edges, each the SPA cost of one observed relative pose
 * (ComputeUnscaledError and ScaleError, cost_functions/cost_helpers_impl.h:28-56,
 * the angle through NormalizeAngleDifference, common/math.h). Landmarks,
 * fixed-frame poses, IMU and the time interpolation of odometry are not part
 * of it; an odometry term is one more edge. */
#define CSM_POSE_GRAPH2D_LOSS_NONE 0  /* nullptr loss (INTRA_SUBMAP, :337-347) */
#define CSM_POSE_GRAPH2D_LOSS_HUBER 1 /* ceres::HuberLoss(huber_scale) (INTER_SUBMAP, :289-298) */
#define CSM_POSE_GRAPH2D_MAX_VERTICES (1 << 22)
#define CSM_POSE_GRAPH2D_MAX_EDGES (1 << 26)
#define CSM_POSE_GRAPH2D_MAX_CG_ITERATIONS (1 << 16)
#define CSM_POSE_GRAPH2D_MAX_LM_ITERATIONS (1 << 16)

/* One residual block of :289-298 / :337-347: `end` observed from `start` as
 * zbar (x, y, angle), Constraint::Pose's weights, and the loss. */
typedef struct csm_pose_graph2d_edge {
  int32_t start, end; /* vertex indices */
  double zbar[3];
  double translation_weight, rotation_weight;
  int32_t loss; /* CSM_POSE_GRAPH2D_LOSS_* */
  int32_t reserved;
} csm_pose_graph2d_edge;

/* optimization_problem_options (huber_scale) and its ceres_solver_options
 * (configuration_files/pose_graph.lua: 10, 50 iterations, monotonic steps).
 * The linear solve is a preconditioned conjugate-gradient iteration:
 * max_cg_iterations is Ceres's max_linear_solver_iterations (500), and an
 * iteration stops at |r| <= cg_relative_tolerance |r0|. */
typedef struct csm_pose_graph2d_options {
  double huber_scale;
  int32_t max_num_iterations;
  int32_t use_nonmonotonic_steps;
  int32_t max_cg_iterations;
  int32_t reserved;
  double cg_relative_tolerance;
} csm_pose_graph2d_options;
/* 10, 50, 0, 500, 1e-8. */
void csm_pose_graph2d_default_options(csm_pose_graph2d_options* out);

/* ceres::Solver::Summary's termination, split by the tolerance that fired. */
#define CSM_POSE_GRAPH2D_CONVERGENCE_GRADIENT 0
#define CSM_POSE_GRAPH2D_CONVERGENCE_PARAMETER 1
#define CSM_POSE_GRAPH2D_CONVERGENCE_FUNCTION 2
#define CSM_POSE_GRAPH2D_NO_CONVERGENCE 3
#define CSM_POSE_GRAPH2D_FAILURE 4
typedef struct csm_pose_graph2d_summary {
  double initial_cost, final_cost;
  int32_t num_iterations;       /* Levenberg-Marquardt iterations after the first evaluation */
  int32_t num_successful_steps; /* those whose step was accepted */
  int32_t num_cg_iterations;    /* over all steps */
  int32_t num_cg_capped_steps;  /* steps whose linear solve ran into max_cg_iterations */
  int32_t termination;          /* CSM_POSE_GRAPH2D_* above */
  int32_t reserved;
} csm_pose_graph2d_summary;

/* The cost 1/2 sum rho(|r|^2) at `poses` (V x 3), and on request every edge's
 * residual as the SPA cost function returns it (E x 3, before the loss) and
 * the cost's gradient (V x 3, every vertex taken as variable). No solve. */
int csm_pose_graph2d_evaluate(csm_context* ctx, const csm_pose_graph2d_options* options,
                              const double* poses, int32_t num_vertices,
                              const csm_pose_graph2d_edge* edges, int64_t num_edges, double* cost,
                              double* residuals, double* gradient);

/* ceres::Solve of :403-407 on the flat problem, with Ceres 1.13's trust-region
 * minimizer and Levenberg-Marquardt strategy restated on the device and its
 * defaults for everything `options` does not name. constant[v] != 0 is
 * SetParameterBlockConstant (:272-277, :284-286); NULL: none. poses_inout
 * receives the solution; constant vertices keep their bits. An edge between
 * two constant vertices is no part of the minimisation; its cost is added to
 * both reported costs (Ceres's fixed_cost). Two calls on the same input return
 * the same bits.
 * Before anything is enqueued: CSM_EINVAL for a null pointer, a non-finite
 * pose, observation or weight, a vertex index outside [0, V), start == end, an
 * unknown loss, a non-positive huber_scale, cg tolerance or iteration limit;
 * CSM_ERANGE past CSM_POSE_GRAPH2D_MAX_*. num_edges == 0 and a problem whose
 * vertices are all constant are successes that launch nothing: the poses stay,
 * the summary reports CONVERGENCE_GRADIENT after 0 iterations and, since
 * nothing was evaluated, costs of 0. */
int csm_pose_graph2d_solve(csm_context* ctx, const csm_pose_graph2d_options* options,
                           double* poses_inout, const uint8_t* constant, int32_t num_vertices,
                           const csm_pose_graph2d_edge* edges, int64_t num_edges,
                           csm_pose_graph2d_summary* summary);
/* Host seconds of the context's last solve that reached the device, by phase:
 * set-up (adjacency and upload), linearisations, linear solves, candidate
 * evaluations. Each phase ends in a read-back, so the clock sees the device. */
void csm_pose_graph2d_last_phase_seconds(csm_context* ctx, double out[4]);

/* Human-readable text for a return code. */
const char* csm_strerror(int code);

#ifdef __cplusplus
}
#endif

#endif /* CSM_AMD_H_ */
