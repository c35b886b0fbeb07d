// C++ drop-in shim over the csm_amd C-ABI for Cartographer's 3D submaps on
// device-resident grids:
//   submap_3d.h:43-104      Submap3D (InsertData, Finish; .cc:323-354)
//   submap_3d.h:119-152     ActiveSubmaps3D::InsertData, AddSubmap (.cc:362-416)
//   range_data_inserter_3d.h:35-51  RangeDataInserter3D::Insert (.cc:109-137)
//   hybrid_grid.h:463-545   HybridGrid
//   hybrid_grid.h:547-571   IntensityHybridGrid
//
// The grids live on the device: Insert updates and grows them there with the
// reference's values bit for bit, and the 3D matchers read them without a host
// copy (FastMatcherFor, MatchRealTime below). One batch call per scan covers
// every grid of the active submaps. With use_intensities a submap also keeps
// its high_resolution_intensity_hybrid_grid() (range_data_inserter_3d.cc:76-89,
// submap_3d.cc:332-339), filled in the same batch call, read by
// CeresScanMatcher3D::Match (scan_matching_3d.h) and forgotten when the submap
// leaves the active pair (submap_3d.cc:396-405); without it nothing is
// allocated for intensities. As in the reference,
// matchers are built from finished submaps only: a submap must not be
// inserted into while a FastMatcherFor result built from it is alive.
// Negative return codes abort like the reference's CHECKs.
#ifndef CARTOGRAPHER_AMD_SUBMAP_3D_H_
#define CARTOGRAPHER_AMD_SUBMAP_3D_H_

#include <cmath>
#include <memory>
#include <vector>

#include "scan_matching_3d.h"
#include "submap_2d.h"

namespace cartographer_amd {

// proto::RangeDataInserterOptions3D (trajectory_builder_3d.lua:100-106
// defaults).
struct RangeDataInserterOptions3D {
  float hit_probability = 0.55f;
  float miss_probability = 0.49f;
  int num_free_space_voxels = 2;
  float intensity_threshold = 40.f;
};

// hybrid_grid.h:463-545: RAII holder of a device grid that starts empty.
class HybridGrid {
 public:
  explicit HybridGrid(float resolution, csm_context* context = nullptr)
      : context_(context ? context : ThreadContext()) {
    CheckOk(csm_hybrid_grid_create(context_, resolution, nullptr, nullptr, 0, 0, &handle_),
            "HybridGrid");
  }
  ~HybridGrid() { csm_hybrid_grid_destroy(handle_); }
  HybridGrid(const HybridGrid&) = delete;
  HybridGrid& operator=(const HybridGrid&) = delete;

  // The known cells' bounding box and DynamicGrid::grid_size().
  void info(int32_t origin[3], int32_t dims[3], int32_t* grid_size) const {
    CheckOk(csm_hybrid_grid_info(handle_, origin, dims, grid_size), "HybridGrid::info");
  }
  // The uint16 values over that box, x fastest (waits for the device).
  std::vector<uint16_t> values() const {
    int32_t o[3], d[3], gs;
    info(o, d, &gs);
    std::vector<uint16_t> out(static_cast<size_t>(d[0]) * d[1] * d[2]);
    CheckOk(csm_hybrid_grid_read(handle_, out.data(), static_cast<int64_t>(out.size())),
            "HybridGrid::values");
    return out;
  }

  csm_hybrid_grid* handle() const { return handle_; }
  csm_context* context() const { return context_; }

 private:
  csm_context* context_;
  csm_hybrid_grid* handle_ = nullptr;
};

// hybrid_grid.h:547-571: RAII holder of a device intensity grid that starts
// empty.
class IntensityHybridGrid {
 public:
  explicit IntensityHybridGrid(float resolution, csm_context* context = nullptr)
      : context_(context ? context : ThreadContext()) {
    CheckOk(csm_intensity_grid_create(context_, resolution, &handle_), "IntensityHybridGrid");
  }
  ~IntensityHybridGrid() { csm_intensity_grid_destroy(handle_); }
  IntensityHybridGrid(const IntensityHybridGrid&) = delete;
  IntensityHybridGrid& operator=(const IntensityHybridGrid&) = delete;

  // The box of the cells with count > 0 and DynamicGrid::grid_size().
  void info(int32_t origin[3], int32_t dims[3], int32_t* grid_size) const {
    CheckOk(csm_intensity_grid_info(handle_, origin, dims, grid_size),
            "IntensityHybridGrid::info");
  }
  // The sums and counts over that box, x fastest (waits for the device).
  void read(std::vector<float>* sums, std::vector<int32_t>* counts) const {
    int32_t o[3], d[3], gs;
    info(o, d, &gs);
    const size_t n = static_cast<size_t>(d[0]) * d[1] * d[2];
    sums->assign(n, 0.f);
    counts->assign(n, 0);
    CheckOk(csm_intensity_grid_read(handle_, sums->data(), counts->data(),
                                    static_cast<int64_t>(n)),
            "IntensityHybridGrid::read");
  }
  // GetIntensity at one cell (waits for the device).
  float GetIntensity(int32_t x, int32_t y, int32_t z) const {
    const int32_t index[3] = {x, y, z};
    float out = 0.f;
    CheckOk(csm_intensity_grid_get_intensity(handle_, index, 1, &out),
            "IntensityHybridGrid::GetIntensity");
    return out;
  }

  csm_intensity_grid* handle() const { return handle_; }
  csm_context* context() const { return context_; }

 private:
  csm_context* context_;
  csm_intensity_grid* handle_ = nullptr;
};

// range_data_inserter_3d.h:35-51
class RangeDataInserter3D {
 public:
  explicit RangeDataInserter3D(const RangeDataInserterOptions3D& options)
      : options_{options.hit_probability, options.miss_probability,
                 options.num_free_space_voxels},
        intensity_threshold_(options.intensity_threshold) {}

  // Insert(range_data, hybrid_grid, nullptr): range_data in the grid's frame.
  void Insert(const RangeData& range_data, HybridGrid* grid) const {
    CheckOk(csm_hybrid_grid_insert(grid->handle(), &options_, range_data.origin,
                                   range_data.returns.xyz.data(),
                                   static_cast<int32_t>(range_data.returns.size())),
            "RangeDataInserter3D::Insert");
  }

  // Insert(range_data, hybrid_grid, intensity_hybrid_grid); the latter may be
  // null, and a cloud without intensities leaves it alone.
  void Insert(const RangeData& range_data, HybridGrid* grid,
              IntensityHybridGrid* intensity_grid) const {
    const PointCloud& returns = range_data.returns;
    CheckOk(returns.intensities.empty() || returns.intensities.size() == returns.size()
                ? CSM_OK
                : CSM_EINVAL,
            "RangeDataInserter3D::Insert intensities");
    CheckOk(csm_hybrid_grid_insert_intensities(
                grid->handle(), intensity_grid ? intensity_grid->handle() : nullptr, &options_,
                intensity_threshold_, range_data.origin, returns.xyz.data(),
                returns.intensities.empty() ? nullptr : returns.intensities.data(),
                static_cast<int32_t>(returns.size())),
            "RangeDataInserter3D::Insert");
  }

  const csm_inserter3d_options& options() const { return options_; }
  float intensity_threshold() const { return intensity_threshold_; }

 private:
  csm_inserter3d_options options_;
  float intensity_threshold_;
};

namespace submap_3d_internal {
// Quaternion::_transformVector and the quaternion product, in double with
// Eigen's operation order.
inline void Rotate(const Quaterniond& q, const double v[3], double out[3]) {
  double u[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
  for (double& c : u) c += c;
  const double c[3] = {q.y * u[2] - q.z * u[1], q.z * u[0] - q.x * u[2], q.x * u[1] - q.y * u[0]};
  for (int a = 0; a < 3; ++a) out[a] = (v[a] + q.w * u[a]) + c[a];
}
inline Quaterniond Multiply(const Quaterniond& a, const Quaterniond& b) {
  return Quaterniond{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
                     a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                     a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                     a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
// Rigid3d::inverse (rigid_transform.h:159-163).
inline Rigid3d Inverse(const Rigid3d& r) {
  Rigid3d out;
  out.rotation = Quaterniond{r.rotation.w, -r.rotation.x, -r.rotation.y, -r.rotation.z};
  double t[3];
  Rotate(out.rotation, r.t, t);
  for (int a = 0; a < 3; ++a) out.t[a] = -t[a];
  return out;
}
}  // namespace submap_3d_internal

// submap_3d.h:43-104
class Submap3D {
 public:
  Submap3D(float high_resolution, float low_resolution, const Rigid3d& local_submap_pose,
           int rotational_scan_matcher_histogram_size, csm_context* context = nullptr,
           bool use_intensities = false)
      : local_pose_(local_submap_pose),
        high_(new HybridGrid(high_resolution, context)),
        low_(new HybridGrid(low_resolution, context)),
        high_intensity_(use_intensities ? new IntensityHybridGrid(high_resolution, context)
                                        : nullptr),
        histogram_(rotational_scan_matcher_histogram_size, 0.f) {}

  const Rigid3d& local_pose() const { return local_pose_; }
  const HybridGrid& high_resolution_hybrid_grid() const { return *high_; }
  const HybridGrid& low_resolution_hybrid_grid() const { return *low_; }
  // submap_3d.h:73-82: null without use_intensities and once forgotten.
  const IntensityHybridGrid* high_resolution_intensity_hybrid_grid() const {
    return high_intensity_.get();
  }
  void ForgetIntensityHybridGrid() { high_intensity_.reset(); }
  const std::vector<float>& rotational_scan_matcher_histogram() const { return histogram_; }
  int num_range_data() const { return num_range_data_; }
  bool insertion_finished() const { return insertion_finished_; }

  // submap_3d.cc:323-347; range_data in the local frame.
  void InsertData(const RangeData& range_data_in_local,
                  const RangeDataInserter3D& range_data_inserter, float high_resolution_max_range,
                  const Quaterniond& local_from_gravity_aligned,
                  const std::vector<float>& scan_histogram_in_gravity) {
    std::vector<Submap3D*> one{this};
    InsertBatch(one, range_data_in_local, range_data_inserter, high_resolution_max_range,
                local_from_gravity_aligned, scan_histogram_in_gravity);
  }

  // submap_3d.cc:349-352
  void Finish() {
    CheckOk(insertion_finished_ ? CSM_EINVAL : CSM_OK, "Submap3D::Finish");
    insertion_finished_ = true;
  }

  // InsertData of the same scan for several submaps of one context: one
  // csm_hybrid_grid_insert_batch call, two jobs (high resolution with the
  // range filter, low resolution without) per submap, each with the submap's
  // local_pose().inverse().cast<float>(). When a submap keeps an intensity
  // grid the call is csm_hybrid_grid_insert_intensities_batch and the
  // high-resolution job fills that grid too.
  static void InsertBatch(const std::vector<Submap3D*>& submaps, const RangeData& range_data,
                          const RangeDataInserter3D& range_data_inserter,
                          float high_resolution_max_range,
                          const Quaterniond& local_from_gravity_aligned,
                          const std::vector<float>& scan_histogram_in_gravity) {
    if (submaps.empty()) return;
    std::vector<csm_hybrid_grid*> grids;
    std::vector<csm_intensity_grid*> intensity_grids;
    std::vector<int32_t> grid_of_job, scan_of_job, transform_of_job, intensity_grid_of_job;
    std::vector<float> transforms, max_ranges;
    for (size_t s = 0; s < submaps.size(); ++s) {
      Submap3D* submap = submaps[s];
      CheckOk(submap->insertion_finished_ ? CSM_EINVAL : CSM_OK, "Submap3D::InsertData");
      const Rigid3d inv = submap_3d_internal::Inverse(submap->local_pose_);
      for (int a = 0; a < 3; ++a) transforms.push_back(static_cast<float>(inv.t[a]));
      transforms.push_back(static_cast<float>(inv.rotation.w));
      transforms.push_back(static_cast<float>(inv.rotation.x));
      transforms.push_back(static_cast<float>(inv.rotation.y));
      transforms.push_back(static_cast<float>(inv.rotation.z));
      for (int k = 0; k < 2; ++k) {
        grid_of_job.push_back(static_cast<int32_t>(grids.size()));
        grids.push_back(k == 0 ? submap->high_->handle() : submap->low_->handle());
        scan_of_job.push_back(0);
        transform_of_job.push_back(static_cast<int32_t>(s));
        max_ranges.push_back(k == 0 ? high_resolution_max_range : 0.f);
        if (k == 0 && submap->high_intensity_) {
          intensity_grid_of_job.push_back(static_cast<int32_t>(intensity_grids.size()));
          intensity_grids.push_back(submap->high_intensity_->handle());
        } else {
          intensity_grid_of_job.push_back(-1);
        }
      }
    }
    const int64_t offsets[2] = {0, static_cast<int64_t>(range_data.returns.size())};
    const PointCloud& returns = range_data.returns;
    if (intensity_grids.empty()) {
      CheckOk(csm_hybrid_grid_insert_batch(
                  submaps[0]->high_->context(), grids.data(), static_cast<int32_t>(grids.size()),
                  &range_data_inserter.options(), 1, range_data.origin, returns.xyz.data(),
                  offsets, static_cast<int32_t>(grid_of_job.size()), grid_of_job.data(),
                  scan_of_job.data(), transforms.data(), static_cast<int32_t>(submaps.size()),
                  transform_of_job.data(), max_ranges.data()),
              "Submap3D::InsertData");
    } else {
      CheckOk(returns.intensities.empty() || returns.intensities.size() == returns.size()
                  ? CSM_OK
                  : CSM_EINVAL,
              "Submap3D::InsertData intensities");
      const float* intensities =
          returns.intensities.empty() ? nullptr : returns.intensities.data();
      CheckOk(csm_hybrid_grid_insert_intensities_batch(
                  submaps[0]->high_->context(), grids.data(), static_cast<int32_t>(grids.size()),
                  intensity_grids.data(), static_cast<int32_t>(intensity_grids.size()),
                  &range_data_inserter.options(), range_data_inserter.intensity_threshold(), 1,
                  range_data.origin, returns.xyz.data(), offsets, &intensities,
                  static_cast<int32_t>(grid_of_job.size()), grid_of_job.data(),
                  scan_of_job.data(), intensity_grid_of_job.data(), transforms.data(),
                  static_cast<int32_t>(submaps.size()), transform_of_job.data(),
                  max_ranges.data()),
              "Submap3D::InsertData");
    }
    for (Submap3D* submap : submaps) {
      ++submap->num_range_data_;
      // submap_3d.cc:341-346: the yaw in double, cast to float.
      const Quaterniond q = submap_3d_internal::Multiply(
          submap_3d_internal::Inverse(submap->local_pose_).rotation, local_from_gravity_aligned);
      const double unit_x[3] = {1., 0., 0.};
      double d[3];
      submap_3d_internal::Rotate(q, unit_x, d);
      const float yaw_in_submap_from_gravity = static_cast<float>(std::atan2(d[1], d[0]));
      std::vector<float> rotated(scan_histogram_in_gravity.size());
      CheckOk(csm_rotate_histogram(scan_histogram_in_gravity.data(),
                                   static_cast<int32_t>(scan_histogram_in_gravity.size()),
                                   yaw_in_submap_from_gravity, rotated.data()),
              "RotateHistogram");
      CheckOk(rotated.size() == submap->histogram_.size() ? CSM_OK : CSM_EINVAL,
              "Submap3D histogram size");
      for (size_t i = 0; i < rotated.size(); ++i) submap->histogram_[i] += rotated[i];
    }
  }

 private:
  Rigid3d local_pose_;
  std::unique_ptr<HybridGrid> high_, low_;
  std::unique_ptr<IntensityHybridGrid> high_intensity_;
  std::vector<float> histogram_;
  int num_range_data_ = 0;
  bool insertion_finished_ = false;
};

// proto::SubmapsOptions3D (trajectory_builder_3d.lua:92-104 defaults).
struct SubmapsOptions3D {
  float high_resolution = 0.10f;
  float high_resolution_max_range = 20.f;
  float low_resolution = 0.45f;
  int num_range_data = 160;
  RangeDataInserterOptions3D range_data_inserter_options;
  // LocalTrajectoryBuilderOptions3D::use_intensities
  // (trajectory_builder_3d.lua:109-112: false): keep and fill
  // high_resolution_intensity_hybrid_grid() per submap.
  bool use_intensities = false;
};

// submap_3d.h:119-152
class ActiveSubmaps3D {
 public:
  explicit ActiveSubmaps3D(const SubmapsOptions3D& options, csm_context* context = nullptr)
      : options_(options),
        context_(context ? context : ThreadContext()),
        range_data_inserter_(options.range_data_inserter_options) {}

  std::vector<std::shared_ptr<const Submap3D>> submaps() const {
    return std::vector<std::shared_ptr<const Submap3D>>(submaps_.begin(), submaps_.end());
  }

  // submap_3d.cc:362-393: every active grid takes the scan in one batch call.
  std::vector<std::shared_ptr<const Submap3D>> InsertData(
      const RangeData& range_data, const Quaterniond& local_from_gravity_aligned,
      const std::vector<float>& rotational_scan_matcher_histogram_in_gravity) {
    if (submaps_.empty() || submaps_.back()->num_range_data() == options_.num_range_data) {
      Rigid3d pose;
      for (int a = 0; a < 3; ++a) pose.t[a] = static_cast<double>(range_data.origin[a]);
      pose.rotation = local_from_gravity_aligned;
      AddSubmap(pose, static_cast<int>(rotational_scan_matcher_histogram_in_gravity.size()));
    }
    std::vector<Submap3D*> active;
    for (auto& submap : submaps_) active.push_back(submap.get());
    Submap3D::InsertBatch(active, range_data, range_data_inserter_,
                          options_.high_resolution_max_range, local_from_gravity_aligned,
                          rotational_scan_matcher_histogram_in_gravity);
    if (submaps_.front()->num_range_data() == 2 * options_.num_range_data)
      submaps_.front()->Finish();
    return submaps();
  }

  // submap_3d.cc:395-416
  void AddSubmap(const Rigid3d& local_submap_pose, int rotational_scan_matcher_histogram_size) {
    if (submaps_.size() >= 2) {
      CheckOk(submaps_.front()->insertion_finished() ? CSM_OK : CSM_EINVAL, "AddSubmap");
      // The active submaps' intensity grids are for scan matching only
      // (submap_3d.cc:399-404).
      submaps_.front()->ForgetIntensityHybridGrid();
      submaps_.erase(submaps_.begin());
    }
    submaps_.push_back(std::make_shared<Submap3D>(
        options_.high_resolution, options_.low_resolution, local_submap_pose,
        rotational_scan_matcher_histogram_size, context_, options_.use_intensities));
  }

 private:
  SubmapsOptions3D options_;
  csm_context* context_;
  RangeDataInserter3D range_data_inserter_;
  std::vector<std::shared_ptr<Submap3D>> submaps_;
};

// FastCorrelativeScanMatcher3D for a finished submap's device grids
// (constraint_builder_3d.cc:170-198): a csm_fast3d handle, matched through
// csm_fast3d_match / _match_full_submap / _match_batch; the caller destroys it
// with csm_fast3d_destroy, before the submap.
inline csm_fast3d* FastMatcherFor(const Submap3D& submap,
                                  const FastCorrelativeScanMatcherOptions3D& options) {
  const csm_fast3d_options o{options.branch_and_bound_depth, options.full_resolution_depth,
                             options.min_rotational_score, options.min_low_resolution_score,
                             options.linear_xy_search_window, options.linear_z_search_window,
                             options.angular_search_window};
  const std::vector<float>& h = submap.rotational_scan_matcher_histogram();
  csm_fast3d* out = nullptr;
  CheckOk(csm_fast3d_create(submap.high_resolution_hybrid_grid().context(),
                            submap.high_resolution_hybrid_grid().handle(),
                            submap.low_resolution_hybrid_grid().handle(), h.data(),
                            static_cast<int32_t>(h.size()), &o, &out),
          "FastMatcherFor");
  return out;
}

// RealTimeCorrelativeScanMatcher3D::Match on a device grid
// (local_trajectory_builder_3d.cc:481).
inline float MatchRealTime(const RealTimeCorrelativeScanMatcherOptions& o,
                           const Rigid3d& initial_pose_estimate, const PointCloud& point_cloud,
                           const HybridGrid& hybrid_grid, Rigid3d* pose_estimate) {
  const csm_rt_options opts{o.linear_search_window, o.angular_search_window,
                            o.translation_delta_cost_weight, o.rotation_delta_cost_weight};
  const csm_pose3d init = initial_pose_estimate.ToC();
  csm_pose3d out{};
  float score = 0.f;
  CheckOk(csm_rt3d_match(hybrid_grid.context(), &opts, hybrid_grid.handle(), &init,
                         point_cloud.xyz.data(), static_cast<int32_t>(point_cloud.size()), &score,
                         &out),
          "MatchRealTime");
  *pose_estimate = Rigid3d::FromC(out);
  return score;
}

}  // namespace cartographer_amd

#endif  // CARTOGRAPHER_AMD_SUBMAP_3D_H_
