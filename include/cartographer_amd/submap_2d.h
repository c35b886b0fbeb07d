// C++ drop-in shim over the csm_amd C-ABI for Cartographer's 2D submaps on
// device-resident grids:
//   submap_2d.h:41-72     Submap2D (InsertRangeData, Finish)
//   submap_2d.h:86-115    ActiveSubmaps2D::InsertRangeData (.cc:153-232)
//   probability_grid_range_data_inserter_2d.h:37-56  Insert(range_data, grid)
//   probability_grid.h:31-68  ProbabilityGrid (limits, cells, ComputeCroppedGrid)
//   tsdf_2d.h:34-78           TSDF2D (limits, both planes, ComputeCroppedGrid)
//   tsdf_range_data_inserter_2d.h:33-55  Insert(range_data, grid)
//
// The grid lives on the device: Insert grows and updates it there with the
// reference's values bit for bit, Finish crops it there, and both 2D matchers
// read it without a host copy (FastMatcherFor, MatchRealTime below). The
// reference types are the POD views of scan_matching.h; negative return codes
// abort like the reference's CHECKs.
#ifndef CARTOGRAPHER_AMD_SUBMAP_2D_H_
#define CARTOGRAPHER_AMD_SUBMAP_2D_H_

#include <memory>
#include <vector>

#include "scan_matching.h"

namespace cartographer_amd {

// sensor::RangeData (sensor/range_data.h:31-35), in the grid's frame.
struct RangeData {
  float origin[3] = {0.f, 0.f, 0.f};
  PointCloud returns;
  PointCloud misses;
};

// proto::ProbabilityGridRangeDataInserterOptions2D
// (trajectory_builder_2d.lua:81-87 defaults).
struct ProbabilityGridRangeDataInserterOptions2D {
  float hit_probability = 0.55f;
  float miss_probability = 0.49f;
  bool insert_free_space = true;
};

// probability_grid.h:31-68: RAII holder of the device grid.
class ProbabilityGrid {
 public:
  // ProbabilityGrid(const MapLimits&): all cells unknown.
  ProbabilityGrid(double resolution, double max_x, double max_y, int num_x_cells, int num_y_cells,
                  csm_context* context = nullptr)
      : context_(context ? context : ThreadContext()) {
    const csm_map_limits l{resolution, max_x, max_y, num_x_cells, num_y_cells};
    CheckOk(csm_probability_grid_create(context_, &l, nullptr, &handle_), "ProbabilityGrid");
  }
  ~ProbabilityGrid() { csm_probability_grid_destroy(handle_); }
  ProbabilityGrid(const ProbabilityGrid&) = delete;
  ProbabilityGrid& operator=(const ProbabilityGrid&) = delete;

  // Grid2D::limits().
  csm_map_limits limits() const {
    csm_map_limits l{};
    CheckOk(csm_probability_grid_limits(handle_, &l), "ProbabilityGrid::limits");
    return l;
  }
  // correspondence_cost_cells(), read back (waits for the device).
  std::vector<uint16_t> cells() const {
    const csm_map_limits l = limits();
    std::vector<uint16_t> out(static_cast<size_t>(l.num_x_cells) * l.num_y_cells);
    CheckOk(csm_probability_grid_read(handle_, out.data(), static_cast<int64_t>(out.size())),
            "ProbabilityGrid::cells");
    return out;
  }
  // probability_grid.cc:91-106, in place (Submap2D::Finish replaces the grid
  // by its cropped copy; nothing else calls it).
  void ComputeCroppedGrid() {
    CheckOk(csm_probability_grid_finish(handle_), "ProbabilityGrid::ComputeCroppedGrid");
  }

  csm_probability_grid* handle() const { return handle_; }
  csm_context* context() const { return context_; }

 private:
  csm_context* context_;
  csm_probability_grid* handle_ = nullptr;
};

// FastCorrelativeScanMatcher2D(grid, options) for a device grid
// (constraint_builder_2d.cc:179-181): a csm_fast2d handle, matched through
// csm_fast2d_match / _match_full_submap / _match_batch; the caller destroys it
// with csm_fast2d_destroy.
inline csm_fast2d* FastMatcherFor(const ProbabilityGrid& grid,
                                  const FastCorrelativeScanMatcherOptions2D& options) {
  const csm_fast2d_options o{options.linear_search_window, options.angular_search_window,
                             options.branch_and_bound_depth, 0};
  csm_fast2d* h = nullptr;
  CheckOk(csm_fast2d_create_from_grid(grid.context(), grid.handle(), &o, &h), "FastMatcherFor");
  return h;
}

// RealTimeCorrelativeScanMatcher2D::Match on a device grid
// (local_trajectory_builder_2d.cc:78-80).
inline double MatchRealTime(const RealTimeCorrelativeScanMatcherOptions& o,
                            const Rigid2d& initial_pose_estimate, const PointCloud& point_cloud,
                            const ProbabilityGrid& grid, Rigid2d* pose_estimate) {
  const csm_rt_options opts{o.linear_search_window, o.angular_search_window,
                            o.translation_delta_cost_weight, o.rotation_delta_cost_weight};
  const csm_pose2d init{initial_pose_estimate.x, initial_pose_estimate.y,
                        initial_pose_estimate.theta};
  csm_pose2d out{};
  double score = 0.;
  CheckOk(csm_rt2d_match_grid(grid.context(), &opts, grid.handle(), &init, point_cloud.xyz.data(),
                              static_cast<int32_t>(point_cloud.size()), &score, &out),
          "MatchRealTime");
  *pose_estimate = Rigid2d{out.x, out.y, out.theta};
  return score;
}

// proto::TSDFRangeDataInserterOptions2D (trajectory_builder_2d.lua:100-112
// defaults), in the proto's types.
struct TSDFRangeDataInserterOptions2D {
  double truncation_distance = 0.3;
  double maximum_weight = 10.;
  bool update_free_space = false;
  int num_normal_samples = 4;
  double sample_radius = 0.5;
  bool project_sdf_distance_to_scan_normal = true;
  int update_weight_range_exponent = 0;
  double update_weight_angle_scan_normal_to_ray_kernel_bandwidth = 0.5;
  double update_weight_distance_cell_to_hit_kernel_bandwidth = 0.5;
};

// tsdf_2d.h:34-78: RAII holder of the device TSDF.
class TSDF2D {
 public:
  // TSDF2D(limits, truncation_distance, max_weight, tables): all cells unknown.
  TSDF2D(double resolution, double max_x, double max_y, int num_x_cells, int num_y_cells,
         float truncation_distance, float max_weight, csm_context* context = nullptr)
      : context_(context ? context : ThreadContext()) {
    const csm_map_limits l{resolution, max_x, max_y, num_x_cells, num_y_cells};
    CheckOk(csm_tsdf_grid_create(context_, &l, truncation_distance, max_weight, nullptr, nullptr,
                                 &handle_),
            "TSDF2D");
  }
  ~TSDF2D() { csm_tsdf_grid_destroy(handle_); }
  TSDF2D(const TSDF2D&) = delete;
  TSDF2D& operator=(const TSDF2D&) = delete;

  // Grid2D::limits().
  csm_map_limits limits() const {
    csm_map_limits l{};
    CheckOk(csm_tsdf_grid_limits(handle_, &l), "TSDF2D::limits");
    return l;
  }
  // correspondence_cost_cells() (the TSD values) and the weight cells, read
  // back (waits for the device).
  void cells(std::vector<uint16_t>* tsd, std::vector<uint16_t>* weight) const {
    const csm_map_limits l = limits();
    const size_t n = static_cast<size_t>(l.num_x_cells) * l.num_y_cells;
    tsd->assign(n, 0);
    weight->assign(n, 0);
    CheckOk(csm_tsdf_grid_read(handle_, tsd->data(), weight->data(), static_cast<int64_t>(n)),
            "TSDF2D::cells");
  }
  // tsdf_2d.cc:118-135, in place (Submap2D::Finish replaces the grid by its
  // cropped copy; nothing else calls it).
  void ComputeCroppedGrid() { CheckOk(csm_tsdf_grid_finish(handle_), "TSDF2D::ComputeCroppedGrid"); }

  csm_tsdf_grid* handle() const { return handle_; }
  csm_context* context() const { return context_; }

 private:
  csm_context* context_;
  csm_tsdf_grid* handle_ = nullptr;
};

// RealTimeCorrelativeScanMatcher2D::Match on a device TSDF
// (real_time_correlative_scan_matcher_2d.cc:38-59, :117-149); declared in
// scan_matching.h.
inline double RealTimeCorrelativeScanMatcher2D::Match(const Rigid2d& initial_pose_estimate,
                                                      const PointCloud& point_cloud,
                                                      const TSDF2D& grid,
                                                      Rigid2d* pose_estimate) const {
  const csm_pose2d init{initial_pose_estimate.x, initial_pose_estimate.y,
                        initial_pose_estimate.theta};
  csm_pose2d out{};
  double score = 0.;
  CheckOk(csm_rt2d_match_tsdf_grid(grid.context(), &options_, grid.handle(), &init,
                                   point_cloud.xyz.data(),
                                   static_cast<int32_t>(point_cloud.size()), &score, &out),
          "RealTimeCorrelativeScanMatcher2D::Match");
  *pose_estimate = Rigid2d{out.x, out.y, out.theta};
  return score;
}

// FastCorrelativeScanMatcher2D(grid, options) for a device TSDF: a TSDF handle
// (the pyramid from the TSD cells, the weights for the Ceres refinement),
// without a host copy. Used and destroyed as the probability grid's.
inline csm_fast2d* FastMatcherFor(const TSDF2D& grid,
                                  const FastCorrelativeScanMatcherOptions2D& options) {
  const csm_fast2d_options o{options.linear_search_window, options.angular_search_window,
                             options.branch_and_bound_depth, 0};
  csm_fast2d* h = nullptr;
  CheckOk(csm_fast2d_create_from_tsdf_grid(grid.context(), grid.handle(), &o, &h),
          "FastMatcherFor");
  return h;
}

// CeresScanMatcher2D::Match on the device grids (ceres_scan_matcher_2d.cc:
// 64-105); declared in scan_matching.h.
inline void CeresScanMatcher2D::Match(const double target_translation[2],
                                      const Rigid2d& initial_pose_estimate,
                                      const PointCloud& point_cloud, const ProbabilityGrid& grid,
                                      Rigid2d* pose_estimate, int* iterations) const {
  const csm_pose2d init{initial_pose_estimate.x, initial_pose_estimate.y,
                        initial_pose_estimate.theta};
  csm_pose2d out{};
  int32_t iters = 0;
  CheckOk(csm_ceres2d_match_grid(grid.context(), &options_, grid.handle(), target_translation,
                                 &init, point_cloud.xyz.data(),
                                 static_cast<int32_t>(point_cloud.size()), &out, &iters),
          "CeresScanMatcher2D::Match");
  *pose_estimate = Rigid2d{out.x, out.y, out.theta};
  if (iterations) *iterations = iters;
}

inline void CeresScanMatcher2D::Match(const double target_translation[2],
                                      const Rigid2d& initial_pose_estimate,
                                      const PointCloud& point_cloud, const TSDF2D& grid,
                                      Rigid2d* pose_estimate, int* iterations) const {
  const csm_pose2d init{initial_pose_estimate.x, initial_pose_estimate.y,
                        initial_pose_estimate.theta};
  csm_pose2d out{};
  int32_t iters = 0;
  CheckOk(csm_ceres2d_match_tsdf_grid(grid.context(), &options_, grid.handle(),
                                      target_translation, &init, point_cloud.xyz.data(),
                                      static_cast<int32_t>(point_cloud.size()), &out, &iters),
          "CeresScanMatcher2D::Match");
  *pose_estimate = Rigid2d{out.x, out.y, out.theta};
  if (iterations) *iterations = iters;
}

// tsdf_range_data_inserter_2d.h:33-55 (the reference ignores the misses).
class TSDFRangeDataInserter2D {
 public:
  explicit TSDFRangeDataInserter2D(const TSDFRangeDataInserterOptions2D& o)
      : options_{o.truncation_distance,
                 o.maximum_weight,
                 o.update_free_space ? 1 : 0,
                 o.num_normal_samples,
                 o.sample_radius,
                 o.project_sdf_distance_to_scan_normal ? 1 : 0,
                 o.update_weight_range_exponent,
                 o.update_weight_angle_scan_normal_to_ray_kernel_bandwidth,
                 o.update_weight_distance_cell_to_hit_kernel_bandwidth} {}

  void Insert(const RangeData& range_data, TSDF2D* grid) const {
    CheckOk(csm_tsdf_grid_insert(grid->handle(), &options_, range_data.origin,
                                 range_data.returns.xyz.data(),
                                 static_cast<int32_t>(range_data.returns.size())),
            "TSDFRangeDataInserter2D::Insert");
  }

  // The same scan into several grids of one context in one call.
  void Insert(const RangeData& range_data, const std::vector<TSDF2D*>& grids) const {
    if (grids.empty()) return;
    const int n = static_cast<int>(grids.size());
    std::vector<csm_tsdf_grid*> handles;
    std::vector<int32_t> grid_of_scan;
    std::vector<float> origins, returns;
    std::vector<int64_t> return_offsets{0};
    for (int g = 0; g < n; ++g) {
      handles.push_back(grids[g]->handle());
      grid_of_scan.push_back(g);
      origins.insert(origins.end(), range_data.origin, range_data.origin + 3);
      returns.insert(returns.end(), range_data.returns.xyz.begin(), range_data.returns.xyz.end());
      return_offsets.push_back(static_cast<int64_t>(returns.size() / 3));
    }
    CheckOk(csm_tsdf_grid_insert_batch(grids[0]->context(), handles.data(), n, &options_, n,
                                       grid_of_scan.data(), origins.data(), returns.data(),
                                       return_offsets.data()),
            "TSDFRangeDataInserter2D::Insert");
  }

 private:
  csm_tsdf_inserter_options options_;
};

// probability_grid_range_data_inserter_2d.h:37-56
class ProbabilityGridRangeDataInserter2D {
 public:
  explicit ProbabilityGridRangeDataInserter2D(
      const ProbabilityGridRangeDataInserterOptions2D& options)
      : options_{options.hit_probability, options.miss_probability,
                 options.insert_free_space ? 1 : 0} {}

  void Insert(const RangeData& range_data, ProbabilityGrid* grid) const {
    CheckOk(csm_probability_grid_insert(
                grid->handle(), &options_, range_data.origin, range_data.returns.xyz.data(),
                static_cast<int32_t>(range_data.returns.size()), range_data.misses.xyz.data(),
                static_cast<int32_t>(range_data.misses.size())),
            "ProbabilityGridRangeDataInserter2D::Insert");
  }

  // The same scan into several grids of one context in one call.
  void Insert(const RangeData& range_data, const std::vector<ProbabilityGrid*>& grids) const {
    if (grids.empty()) return;
    const int n = static_cast<int>(grids.size());
    std::vector<csm_probability_grid*> handles;
    std::vector<int32_t> grid_of_scan;
    std::vector<float> origins, returns, misses;
    std::vector<int64_t> return_offsets{0}, miss_offsets{0};
    for (int g = 0; g < n; ++g) {
      handles.push_back(grids[g]->handle());
      grid_of_scan.push_back(g);
      origins.insert(origins.end(), range_data.origin, range_data.origin + 3);
      returns.insert(returns.end(), range_data.returns.xyz.begin(), range_data.returns.xyz.end());
      misses.insert(misses.end(), range_data.misses.xyz.begin(), range_data.misses.xyz.end());
      return_offsets.push_back(static_cast<int64_t>(returns.size() / 3));
      miss_offsets.push_back(static_cast<int64_t>(misses.size() / 3));
    }
    CheckOk(csm_probability_grid_insert_batch(grids[0]->context(), handles.data(), n, &options_, n,
                                              grid_of_scan.data(), origins.data(), returns.data(),
                                              return_offsets.data(), misses.data(),
                                              miss_offsets.data()),
            "ProbabilityGridRangeDataInserter2D::Insert");
  }

 private:
  csm_inserter2d_options options_;
};

// submap_2d.h:41-72. The grid is a ProbabilityGrid (grid()) or a TSDF2D
// (tsdf()); the other accessor returns null.
class Submap2D {
 public:
  Submap2D(float origin_x, float origin_y, std::unique_ptr<ProbabilityGrid> grid)
      : origin_x_(origin_x), origin_y_(origin_y), grid_(std::move(grid)) {}
  Submap2D(float origin_x, float origin_y, std::unique_ptr<TSDF2D> tsdf)
      : origin_x_(origin_x), origin_y_(origin_y), tsdf_(std::move(tsdf)) {}

  const ProbabilityGrid* grid() const { return grid_.get(); }
  ProbabilityGrid* mutable_grid() { return grid_.get(); }
  const TSDF2D* tsdf() const { return tsdf_.get(); }
  TSDF2D* mutable_tsdf() { return tsdf_.get(); }
  float origin_x() const { return origin_x_; }
  float origin_y() const { return origin_y_; }
  int num_range_data() const { return num_range_data_; }
  bool insertion_finished() const { return insertion_finished_; }

  // submap_2d.cc:137-144
  void InsertRangeData(const RangeData& range_data,
                       const ProbabilityGridRangeDataInserter2D* range_data_inserter) {
    CheckOk(insertion_finished_ ? CSM_EINVAL : CSM_OK, "Submap2D::InsertRangeData");
    CheckOk(grid_ ? CSM_OK : CSM_EINVAL, "Submap2D::InsertRangeData");
    range_data_inserter->Insert(range_data, grid_.get());
    ++num_range_data_;
  }
  void InsertRangeData(const RangeData& range_data,
                       const TSDFRangeDataInserter2D* range_data_inserter) {
    CheckOk(insertion_finished_ || !tsdf_ ? CSM_EINVAL : CSM_OK, "Submap2D::InsertRangeData");
    range_data_inserter->Insert(range_data, tsdf_.get());
    ++num_range_data_;
  }
  // submap_2d.cc:146-151
  void Finish() {
    CheckOk(insertion_finished_ ? CSM_EINVAL : CSM_OK, "Submap2D::Finish");
    if (grid_) grid_->ComputeCroppedGrid();
    else tsdf_->ComputeCroppedGrid();
    insertion_finished_ = true;
  }

 private:
  friend class ActiveSubmaps2D;
  float origin_x_, origin_y_;
  std::unique_ptr<ProbabilityGrid> grid_;
  std::unique_ptr<TSDF2D> tsdf_;
  int num_range_data_ = 0;
  bool insertion_finished_ = false;
};

// proto::SubmapsOptions2D, the fields this path reads
// (trajectory_builder_2d.lua:69-88 defaults).
struct SubmapsOptions2D {
  int num_range_data = 90;
  float resolution = 0.05f;
  // grid_options_2d.grid_type; it selects the inserter too
  // (CreateGrid / CreateRangeDataInserter, submap_2d.cc:176-222).
  Grid2DView::GridType grid_type = Grid2DView::GridType::PROBABILITY_GRID;
  ProbabilityGridRangeDataInserterOptions2D range_data_inserter_options;
  TSDFRangeDataInserterOptions2D tsdf_range_data_inserter_options;
};

// submap_2d.h:86-115
class ActiveSubmaps2D {
 public:
  explicit ActiveSubmaps2D(const SubmapsOptions2D& options, csm_context* context = nullptr)
      : options_(options),
        context_(context ? context : ThreadContext()),
        range_data_inserter_(options.range_data_inserter_options),
        tsdf_range_data_inserter_(options.tsdf_range_data_inserter_options) {}

  std::vector<std::shared_ptr<const Submap2D>> submaps() const {
    return std::vector<std::shared_ptr<const Submap2D>>(submaps_.begin(), submaps_.end());
  }

  // submap_2d.cc:162-175: both active submaps take the scan in one batch call.
  std::vector<std::shared_ptr<const Submap2D>> InsertRangeData(const RangeData& range_data) {
    if (submaps_.empty() || submaps_.back()->num_range_data() == options_.num_range_data)
      AddSubmap(range_data.origin[0], range_data.origin[1]);
    std::vector<ProbabilityGrid*> grids;
    std::vector<TSDF2D*> tsdfs;
    for (auto& submap : submaps_) {
      CheckOk(submap->insertion_finished() ? CSM_EINVAL : CSM_OK, "ActiveSubmaps2D");
      if (submap->mutable_grid()) grids.push_back(submap->mutable_grid());
      else tsdfs.push_back(submap->mutable_tsdf());
    }
    range_data_inserter_.Insert(range_data, grids);
    tsdf_range_data_inserter_.Insert(range_data, tsdfs);
    for (auto& submap : submaps_) ++submap->num_range_data_;
    if (submaps_.front()->num_range_data() == 2 * options_.num_range_data)
      submaps_.front()->Finish();
    return submaps();
  }

 private:
  // submap_2d.cc:192-232: a kInitialSubmapSize^2 grid of options_.grid_type
  // centred on the origin.
  void AddSubmap(float origin_x, float origin_y) {
    if (submaps_.size() >= 2) {
      CheckOk(submaps_.front()->insertion_finished() ? CSM_OK : CSM_EINVAL, "AddSubmap");
      submaps_.erase(submaps_.begin());
    }
    constexpr int kInitialSubmapSize = 100;
    const float resolution = options_.resolution;
    const double half = 0.5 * kInitialSubmapSize * resolution;
    if (options_.grid_type == Grid2DView::GridType::TSDF) {
      const TSDFRangeDataInserterOptions2D& t = options_.tsdf_range_data_inserter_options;
      submaps_.push_back(std::make_shared<Submap2D>(
          origin_x, origin_y,
          std::make_unique<TSDF2D>(resolution, static_cast<double>(origin_x) + half,
                                   static_cast<double>(origin_y) + half, kInitialSubmapSize,
                                   kInitialSubmapSize, static_cast<float>(t.truncation_distance),
                                   static_cast<float>(t.maximum_weight), context_)));
      return;
    }
    submaps_.push_back(std::make_shared<Submap2D>(
        origin_x, origin_y,
        std::make_unique<ProbabilityGrid>(resolution, static_cast<double>(origin_x) + half,
                                          static_cast<double>(origin_y) + half, kInitialSubmapSize,
                                          kInitialSubmapSize, context_)));
  }

  SubmapsOptions2D options_;
  csm_context* context_;
  ProbabilityGridRangeDataInserter2D range_data_inserter_;
  TSDFRangeDataInserter2D tsdf_range_data_inserter_;
  std::vector<std::shared_ptr<Submap2D>> submaps_;
};

}  // namespace cartographer_amd

#endif  // CARTOGRAPHER_AMD_SUBMAP_2D_H_
