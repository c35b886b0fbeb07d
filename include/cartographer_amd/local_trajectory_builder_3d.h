// C++ drop-in shim over the csm_amd C-ABI for Cartographer's 3D local SLAM
// loop on device-resident data:
//   mapping/internal/3d/local_trajectory_builder_3d.h:47-126  LocalTrajectoryBuilder3D
//     .cc:451-515  ScanMatch
//     .cc:540-700  AddRangeData
//     .cc:705-874  AddAccumulatedRangeData
//     .cc:886-925  InsertIntoSubmap
//   mapping/internal/motion_filter.h:34-49  MotionFilter (local_trajectory_builder_2d.h)
//   mapping/pose_extrapolator_interface.h:36-78  PoseExtrapolatorInterface
//
// The per-point work of a sweep (each point by its own extrapolated pose, the
// range test, both voxel filters, the move to the tracking frame and both
// adaptive voxel filters) is one csm_range_data3d_prepare call; the
// per-message voxel filter is csm_voxel_filter_large; the range data is moved
// by the pose estimate in csm_range_data_transform; the scan match and the
// insertion go through the matchers and ActiveSubmaps3D of scan_matching_3d.h
// and submap_3d.h. The rotational histogram is csm_compute_histogram on the
// host, of the returns rotated by csm_range_data_transform with a zero
// translation. The few rigid transforms in between are computed here on the
// host in Eigen's operation order. The caller supplies the pose extrapolator;
// PoseExtrapolator, ImuTracker and RangeDataCollator are not part of this.
// Times are seconds.
//
// Left out, all of them the fork's additions to upstream's builder:
// scanmatch_mode 3 and 4 (PCL ICP / NDT), use_edge_filter and VoxelFilterEdge,
// the IMU-acceleration gate of AddAccumulatedRangeData (.cc:714-719), the PCD
// dumps and logs, and the metrics gauges.
#ifndef CARTOGRAPHER_AMD_LOCAL_TRAJECTORY_BUILDER_3D_H_
#define CARTOGRAPHER_AMD_LOCAL_TRAJECTORY_BUILDER_3D_H_

#include <cmath>
#include <memory>
#include <vector>

#include "local_trajectory_builder_2d.h"
#include "submap_3d.h"

namespace cartographer_amd {

// proto::LocalTrajectoryBuilderOptions3D, the fields this builder reads
// (trajectory_builder_3d.lua:18-112 defaults).
struct LocalTrajectoryBuilderOptions3D {
  LocalTrajectoryBuilderOptions3D() {
    real_time_correlative_scan_matcher_options.linear_search_window = 0.15;
    real_time_correlative_scan_matcher_options.angular_search_window = 1. * M_PI / 180.;
    motion_filter_options.max_time_seconds = 0.5;
    motion_filter_options.max_distance_meters = 0.1;
    motion_filter_options.max_angle_radians = 0.004;
  }
  float min_range = 1.f;
  float max_range = 60.f;
  int num_accumulated_range_data = 1;
  float voxel_filter_size = 0.15f;
  csm_adaptive_voxel_filter_options high_resolution_adaptive_voxel_filter_options{2.f, 150.f,
                                                                                  15.f};
  csm_adaptive_voxel_filter_options low_resolution_adaptive_voxel_filter_options{4.f, 200.f,
                                                                                 60.f};
  bool use_online_correlative_scan_matching = false;
  RealTimeCorrelativeScanMatcherOptions real_time_correlative_scan_matcher_options;
  // With intensity_cost_function_options_0, read when use_intensities is set.
  CeresScanMatcherOptions3D ceres_scan_matcher_options;
  MotionFilterOptions motion_filter_options;
  int rotational_histogram_size = 120;
  SubmapsOptions3D submaps_options;  // its use_intensities follows the builder's
  bool use_intensities = false;
};

// sensor::TimedPointCloudOriginData::RangeMeasurement
// (sensor/timed_point_cloud_data.h:40-44): a point, its time relative to the
// sweep's (<= 0), its intensity and the index of the origin it was measured
// from.
struct RangeMeasurement3D {
  float position[3];
  float time;
  float intensity;
  int32_t origin_index;
};

// mapping/pose_extrapolator_interface.h:36-78: the 2D builder's methods and
// ExtrapolatePosesWithGravity, whose default body is PoseExtrapolator's
// (pose_extrapolator.cc:266-279).
class PoseExtrapolatorInterface3D : public PoseExtrapolatorInterface {
 public:
  struct ExtrapolationResult {
    std::vector<float> previous_poses;  // 7 floats (t, q w x y z) per time but the last
    Rigid3d current_pose;
    Quaterniond gravity_from_tracking;
  };
  virtual ExtrapolationResult ExtrapolatePosesWithGravity(const std::vector<double>& times) {
    namespace in = local_2d_internal;
    ExtrapolationResult result;
    result.previous_poses.reserve(7 * times.size());
    for (size_t i = 0; i + 1 < times.size(); ++i) {
      float tq[7];
      in::ToArray(in::Cast(in::FromRigid3d(ExtrapolatePose(times[i]))), tq);
      result.previous_poses.insert(result.previous_poses.end(), tq, tq + 7);
    }
    result.current_pose = ExtrapolatePose(times.back());
    result.gravity_from_tracking = EstimateGravityOrientation(times.back());
    return result;
  }
};

// TrajectoryNode::Data (trajectory_node.h:45-63), the fields the 3D builder fills.
struct TrajectoryNodeDataLocal3D {
  double time;
  Quaterniond gravity_alignment;
  PointCloud high_resolution_point_cloud;
  PointCloud low_resolution_point_cloud;
  std::vector<float> rotational_scan_matcher_histogram;
  Rigid3d local_pose;
};

class LocalTrajectoryBuilder3D {
 public:
  // local_trajectory_builder_3d.h:51-63
  struct InsertionResult {
    std::shared_ptr<const TrajectoryNodeDataLocal3D> constant_data;
    std::vector<std::shared_ptr<const Submap3D>> insertion_submaps;
  };
  struct MatchingResult {
    double time;
    Rigid3d local_pose;
    RangeData range_data_in_local;
    // 'nullptr' if dropped by the motion filter.
    std::unique_ptr<const InsertionResult> insertion_result;
  };

  LocalTrajectoryBuilder3D(const LocalTrajectoryBuilderOptions3D& options,
                           PoseExtrapolatorInterface3D* extrapolator,
                           csm_context* context = nullptr)
      : options_(options),
        context_(context ? context : ThreadContext()),
        extrapolator_(extrapolator),
        active_submaps_(WithIntensities(options), context_),
        motion_filter_(options.motion_filter_options),
        ceres_scan_matcher_(options.ceres_scan_matcher_options) {}

  LocalTrajectoryBuilder3D(const LocalTrajectoryBuilder3D&) = delete;
  LocalTrajectoryBuilder3D& operator=(const LocalTrajectoryBuilder3D&) = delete;

  const ActiveSubmaps3D& active_submaps() const { return active_submaps_; }
  // What the last csm_range_data3d_prepare call left (test-visible).
  const RangeData& last_range_data_in_tracking() const { return last_range_data_; }
  const PointCloud& last_high_resolution_point_cloud() const { return last_high_; }
  const PointCloud& last_low_resolution_point_cloud() const { return last_low_; }

  // .cc:540-700 on synchronized data. nullptr: no result yet (the early
  // returns of :552-572, or still accumulating) or none at all.
  // num_message_intensities: the unsynchronized message's intensity count,
  // for the check of :544-549 (negative: not checked).
  std::unique_ptr<MatchingResult> AddRangeData(double time, const std::vector<float>& origins_xyz,
                                               const std::vector<RangeMeasurement3D>& ranges,
                                               int64_t num_message_intensities = -1) {
    namespace in = local_2d_internal;
    if (options_.use_intensities && num_message_intensities >= 0)
      CheckOk(static_cast<size_t>(num_message_intensities) == ranges.size() ? CSM_OK : CSM_EINVAL,
              "AddRangeData: inconsistent number of intensities and ranges");
    if (ranges.empty()) return nullptr;           // :552-555
    if (extrapolator_ == nullptr) return nullptr;  // :557-562
    CheckOk(ranges.back().time <= 0.f ? CSM_OK : CSM_EINVAL, "AddRangeData");  // :565
    const double time_first_point = time + static_cast<double>(ranges.front().time);
    if (time_first_point < extrapolator_->GetLastPoseTime()) return nullptr;  // :566-572
    if (num_accumulated_ == 0) accumulated_.clear();
    // The per-message VoxelFilter (:584-585), on the sensor-frame positions.
    Accumulated data;
    data.time = time;
    data.origins = origins_xyz;
    {
      std::vector<float> xyz;
      xyz.reserve(3 * ranges.size());
      for (const RangeMeasurement3D& r : ranges) xyz.insert(xyz.end(), r.position, r.position + 3);
      std::vector<uint8_t> keep(ranges.size());
      int64_t kept = 0;
      CheckOk(csm_voxel_filter_large(context_, xyz.data(), static_cast<int64_t>(ranges.size()),
                                     0.5f * options_.voxel_filter_size, keep.data(), &kept),
              "csm_voxel_filter_large");
      data.ranges.reserve(static_cast<size_t>(kept));
      for (size_t i = 0; i < ranges.size(); ++i)
        if (keep[i]) data.ranges.push_back(ranges[i]);
    }
    accumulated_.push_back(std::move(data));
    ++num_accumulated_;
    if (num_accumulated_ < options_.num_accumulated_range_data) return nullptr;  // :593-595
    num_accumulated_ = 0;

    std::vector<double> hit_times;  // :598-620
    double prev_time_point = extrapolator_->GetLastExtrapolatedTime();
    for (const Accumulated& a : accumulated_) {
      for (const RangeMeasurement3D& hit : a.ranges) {
        double time_point = a.time + static_cast<double>(hit.time);
        if (time_point < prev_time_point) time_point = prev_time_point;
        hit_times.push_back(time_point);
        prev_time_point = time_point;
      }
    }
    hit_times.push_back(accumulated_.back().time);
    const PoseExtrapolatorInterface3D::ExtrapolationResult extrapolation_result =
        extrapolator_->ExtrapolatePosesWithGravity(hit_times);
    const std::vector<float>& poses = extrapolation_result.previous_poses;
    CheckOk(poses.size() / 7 + 1 == hit_times.size() ? CSM_OK : CSM_EINVAL,
            "ExtrapolatePosesWithGravity");  // :627

    std::vector<float> hits, intensities, origins;
    std::vector<int32_t> origin_index;
    for (const Accumulated& a : accumulated_) {
      const int32_t base = static_cast<int32_t>(origins.size() / 3);
      for (const RangeMeasurement3D& hit : a.ranges) {
        hits.insert(hits.end(), hit.position, hit.position + 3);
        intensities.push_back(hit.intensity);
        origin_index.push_back(base + hit.origin_index);
      }
      origins.insert(origins.end(), a.origins.begin(), a.origins.end());
    }
    accumulated_.clear();
    const in::Rigid3<double> current_pose = in::FromRigid3d(extrapolation_result.current_pose);
    float tracking_from_local[7];  // current_pose.inverse().cast<float>() (:698)
    in::ToArray(in::Cast(in::Inverse(current_pose)), tracking_from_local);
    const float local_origin[3] = {static_cast<float>(current_pose.t[0]),
                                   static_cast<float>(current_pose.t[1]),
                                   static_cast<float>(current_pose.t[2])};  // :681
    const csm_range_data3d_options o{options_.min_range, options_.max_range,
                                     options_.voxel_filter_size,
                                     options_.high_resolution_adaptive_voxel_filter_options,
                                     options_.low_resolution_adaptive_voxel_filter_options};
    const int32_t n = static_cast<int32_t>(origin_index.size());
    const size_t room = static_cast<size_t>(n);
    const bool with_intensities = options_.use_intensities;
    RangeData& rd = last_range_data_;
    for (PointCloud* cloud : {&rd.returns, &rd.misses, &last_high_, &last_low_}) {
      cloud->xyz.assign(3 * room, 0.f);
      cloud->intensities.assign(with_intensities && cloud != &rd.misses ? room : 0, 0.f);
    }
    int32_t num_returns = 0, num_misses = 0, num_high = 0, num_low = 0;
    CheckOk(csm_range_data3d_prepare(
                context_, &o, hits.data(), with_intensities ? intensities.data() : nullptr,
                origin_index.data(), poses.data(), n, origins.data(),
                static_cast<int32_t>(origins.size() / 3), tracking_from_local, local_origin,
                rd.origin, rd.returns.xyz.data(), rd.returns.intensities.data(), &num_returns,
                rd.misses.xyz.data(), &num_misses, last_high_.xyz.data(),
                last_high_.intensities.data(), &num_high, last_low_.xyz.data(),
                last_low_.intensities.data(), &num_low),
            "csm_range_data3d_prepare");
    Shrink(&rd.returns, num_returns);
    Shrink(&rd.misses, num_misses);
    Shrink(&last_high_, num_high);
    Shrink(&last_low_, num_low);
    const double current_time = hit_times.back();  // :678
    return AddAccumulatedRangeData(current_time, rd, last_high_, last_low_,
                                   extrapolation_result.current_pose,
                                   extrapolation_result.gravity_from_tracking);
  }

  // .cc:705-874 without the fork's additions and the wall-clock metrics; the
  // adaptive voxel filters of :734-745 have already run on the device.
  std::unique_ptr<MatchingResult> AddAccumulatedRangeData(
      double time, const RangeData& filtered_range_data_in_tracking,
      const PointCloud& high_resolution_point_cloud_in_tracking,
      const PointCloud& low_resolution_point_cloud_in_tracking, const Rigid3d& pose_prediction,
      const Quaterniond& gravity_alignment) {
    namespace in = local_2d_internal;
    if (filtered_range_data_in_tracking.returns.size() == 0) return nullptr;  // :722-725
    if (high_resolution_point_cloud_in_tracking.size() == 0) return nullptr;  // :738-741
    if (low_resolution_point_cloud_in_tracking.size() == 0) return nullptr;   // :746-749
    std::unique_ptr<Rigid3d> pose_estimate =
        ScanMatch(pose_prediction, low_resolution_point_cloud_in_tracking,
                  high_resolution_point_cloud_in_tracking);
    if (pose_estimate == nullptr) return nullptr;  // :785-788
    extrapolator_->AddPose(time, *pose_estimate);  // :799

    // TransformRangeData(filtered_range_data_in_tracking,
    //                    pose_estimate->cast<float>()) (:810-811).
    float local_from_tracking[7];
    in::ToArray(in::Cast(in::FromRigid3d(*pose_estimate)), local_from_tracking);
    const RangeData& g = filtered_range_data_in_tracking;
    RangeData range_data_in_local;
    range_data_in_local.returns.xyz.resize(g.returns.xyz.size());
    range_data_in_local.returns.intensities = g.returns.intensities;
    range_data_in_local.misses.xyz.resize(g.misses.xyz.size());
    CheckOk(csm_range_data_transform(
                context_, local_from_tracking, g.origin, g.returns.xyz.data(),
                static_cast<int32_t>(g.returns.size()), g.misses.xyz.data(),
                static_cast<int32_t>(g.misses.size()), range_data_in_local.origin,
                range_data_in_local.returns.xyz.data(), range_data_in_local.misses.xyz.data()),
            "csm_range_data_transform");
    std::unique_ptr<InsertionResult> insertion_result = InsertIntoSubmap(
        time, range_data_in_local, filtered_range_data_in_tracking,
        high_resolution_point_cloud_in_tracking, low_resolution_point_cloud_in_tracking,
        *pose_estimate, gravity_alignment);
    std::unique_ptr<MatchingResult> result(new MatchingResult{
        time, *pose_estimate, std::move(range_data_in_local), std::move(insertion_result)});
    return result;
  }

  // .cc:451-515, the upstream path: the real-time matcher (if enabled) refines
  // the start of the Ceres refinement, both on the first active submap's
  // device grids.
  std::unique_ptr<Rigid3d> ScanMatch(const Rigid3d& pose_prediction,
                                     const PointCloud& low_resolution_point_cloud_in_tracking,
                                     const PointCloud& high_resolution_point_cloud_in_tracking) {
    namespace in = local_2d_internal;
    if (active_submaps_.submaps().empty())  // :456-458
      return std::unique_ptr<Rigid3d>(new Rigid3d(pose_prediction));
    std::shared_ptr<const Submap3D> matching_submap = active_submaps_.submaps().front();
    const in::Rigid3<double> local_pose = in::FromRigid3d(matching_submap->local_pose());
    const in::Rigid3<double> in_submap =
        in::Mul(in::Inverse(local_pose), in::FromRigid3d(pose_prediction));
    Rigid3d initial_ceres_pose = in::ToRigid3d(in_submap);
    if (options_.use_online_correlative_scan_matching) {  // :478-485
      const Rigid3d initial_pose = initial_ceres_pose;
      MatchRealTime(options_.real_time_correlative_scan_matcher_options, initial_pose,
                    high_resolution_point_cloud_in_tracking,
                    matching_submap->high_resolution_hybrid_grid(), &initial_ceres_pose);
    }
    const IntensityHybridGrid* intensity_grid =
        options_.use_intensities ? matching_submap->high_resolution_intensity_hybrid_grid()
                                 : nullptr;
    Rigid3d pose_observation_in_submap;
    ceres_scan_matcher_.Match(
        in_submap.t, initial_ceres_pose,
        {{&high_resolution_point_cloud_in_tracking,
          matching_submap->high_resolution_hybrid_grid().handle(),
          intensity_grid ? intensity_grid->handle() : nullptr},
         {&low_resolution_point_cloud_in_tracking,
          matching_submap->low_resolution_hybrid_grid().handle(), nullptr}},
        &pose_observation_in_submap, context_);
    return std::unique_ptr<Rigid3d>(new Rigid3d(
        in::ToRigid3d(in::Mul(local_pose, in::FromRigid3d(pose_observation_in_submap)))));
  }

  // .cc:886-925
  std::unique_ptr<InsertionResult> InsertIntoSubmap(
      double time, const RangeData& filtered_range_data_in_local,
      const RangeData& filtered_range_data_in_tracking,
      const PointCloud& high_resolution_point_cloud_in_tracking,
      const PointCloud& low_resolution_point_cloud_in_tracking, const Rigid3d& pose_estimate,
      const Quaterniond& gravity_alignment) {
    if (motion_filter_.IsSimilar(time, pose_estimate)) return nullptr;
    // TransformPointCloud(returns, Rigid3f::Rotation(gravity_alignment.cast<float>()))
    // (:898-903) by the device kernel, with a zero translation.
    const float rotation[7] = {0.f,
                               0.f,
                               0.f,
                               static_cast<float>(gravity_alignment.w),
                               static_cast<float>(gravity_alignment.x),
                               static_cast<float>(gravity_alignment.y),
                               static_cast<float>(gravity_alignment.z)};
    const PointCloud& returns = filtered_range_data_in_tracking.returns;
    const float zero[3] = {0.f, 0.f, 0.f};
    float moved_origin[3];
    std::vector<float> in_gravity(returns.xyz.size());
    CheckOk(csm_range_data_transform(context_, rotation, zero, returns.xyz.data(),
                                     static_cast<int32_t>(returns.size()), nullptr, 0,
                                     moved_origin, in_gravity.data(), nullptr),
            "csm_range_data_transform");
    std::vector<float> histogram(static_cast<size_t>(options_.rotational_histogram_size));
    CheckOk(csm_compute_histogram(in_gravity.data(), static_cast<int64_t>(returns.size()),
                                  options_.rotational_histogram_size, histogram.data()),
            "csm_compute_histogram");
    // pose_estimate.rotation() * gravity_alignment.inverse() (:908-909): Eigen's
    // inverse is the conjugate over the squared norm, summed as its packet
    // reduction does.
    const Quaterniond& g = gravity_alignment;
    const double n2 = (g.x * g.x + g.z * g.z) + (g.y * g.y + g.w * g.w);
    const Quaterniond local_from_gravity_aligned = submap_3d_internal::Multiply(
        pose_estimate.rotation, Quaterniond{g.w / n2, -g.x / n2, -g.y / n2, -g.z / n2});
    last_local_from_gravity_aligned_ = local_from_gravity_aligned;
    std::vector<std::shared_ptr<const Submap3D>> insertion_submaps = active_submaps_.InsertData(
        filtered_range_data_in_local, local_from_gravity_aligned, histogram);
    std::unique_ptr<InsertionResult> result(new InsertionResult{
        std::make_shared<const TrajectoryNodeDataLocal3D>(TrajectoryNodeDataLocal3D{
            time, gravity_alignment, high_resolution_point_cloud_in_tracking,
            low_resolution_point_cloud_in_tracking, histogram, pose_estimate}),
        std::move(insertion_submaps)});
    return result;
  }

  const Quaterniond& last_local_from_gravity_aligned() const {
    return last_local_from_gravity_aligned_;
  }

 private:
  // One AddRangeData call's filtered message (TimedPointCloudOriginData).
  struct Accumulated {
    double time;
    std::vector<float> origins;
    std::vector<RangeMeasurement3D> ranges;
  };

  static SubmapsOptions3D WithIntensities(const LocalTrajectoryBuilderOptions3D& options) {
    SubmapsOptions3D submaps = options.submaps_options;
    submaps.use_intensities = options.use_intensities;
    return submaps;
  }
  static void Shrink(PointCloud* cloud, int32_t count) {
    cloud->xyz.resize(3 * static_cast<size_t>(count));
    if (!cloud->intensities.empty()) cloud->intensities.resize(static_cast<size_t>(count));
  }

  const LocalTrajectoryBuilderOptions3D options_;
  csm_context* context_;
  PoseExtrapolatorInterface3D* extrapolator_;
  ActiveSubmaps3D active_submaps_;
  MotionFilter motion_filter_;
  CeresScanMatcher3D ceres_scan_matcher_;
  int num_accumulated_ = 0;
  std::vector<Accumulated> accumulated_;
  RangeData last_range_data_;
  PointCloud last_high_, last_low_;
  Quaterniond last_local_from_gravity_aligned_{1., 0., 0., 0.};
};

}  // namespace cartographer_amd

#endif  // CARTOGRAPHER_AMD_LOCAL_TRAJECTORY_BUILDER_3D_H_
