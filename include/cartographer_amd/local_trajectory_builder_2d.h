// C++ drop-in shim over the csm_amd C-ABI for Cartographer's 2D local SLAM
// loop on device-resident data:
//   mapping/internal/2d/local_trajectory_builder_2d.h:45-124  LocalTrajectoryBuilder2D
//     .cc:51-63    TransformToGravityAlignedFrameAndFilter
//     .cc:65-102   ScanMatch
//     .cc:104-209  AddRangeData
//     .cc:211-277  AddAccumulatedRangeData
//     .cc:279-300  InsertIntoSubmap
//   mapping/internal/motion_filter.h:34-49  MotionFilter (.cc:40-58)
//   mapping/pose_extrapolator_interface.h:36-78  PoseExtrapolatorInterface
//
// The per-point work of a sweep (each point by its own extrapolated pose, the
// range test, the gravity alignment, the z crop, the voxel filters and the
// adaptive voxel filter) is one csm_range_data2d_prepare call; the range data
// is moved by the pose estimate in csm_range_data_transform; the scan match
// and the insertion go through the matchers and ActiveSubmaps2D of
// scan_matching.h and submap_2d.h, on either grid type. The few rigid
// transforms in between are computed here on the host in Eigen's operation
// order. The caller supplies the pose extrapolator; PoseExtrapolator,
// ImuTracker and RangeDataCollator are not part of this, nor are the metrics.
// Times are seconds, as in pose_graph_2d_search.h.
#ifndef CARTOGRAPHER_AMD_LOCAL_TRAJECTORY_BUILDER_2D_H_
#define CARTOGRAPHER_AMD_LOCAL_TRAJECTORY_BUILDER_2D_H_

#include <cmath>
#include <memory>
#include <vector>

#include "scan_matching_3d.h"
#include "submap_2d.h"

namespace cartographer_amd {

namespace local_2d_internal {

// transform::Rigid3<T>: translation and rotation (w, x, y, z).
template <typename T>
struct Rigid3 {
  T t[3] = {T(0), T(0), T(0)};
  T q[4] = {T(1), T(0), T(0), T(0)};
};

inline Rigid3<double> FromRigid3d(const Rigid3d& r) {
  Rigid3<double> out;
  for (int a = 0; a < 3; ++a) out.t[a] = r.t[a];
  out.q[0] = r.rotation.w, out.q[1] = r.rotation.x, out.q[2] = r.rotation.y,
  out.q[3] = r.rotation.z;
  return out;
}
inline Rigid3d ToRigid3d(const Rigid3<double>& r) {
  Rigid3d out;
  for (int a = 0; a < 3; ++a) out.t[a] = r.t[a];
  out.rotation = Quaterniond{r.q[0], r.q[1], r.q[2], r.q[3]};
  return out;
}
// Rigid3d::cast<float>().
inline Rigid3<float> Cast(const Rigid3<double>& r) {
  Rigid3<float> out;
  for (int a = 0; a < 3; ++a) out.t[a] = static_cast<float>(r.t[a]);
  for (int a = 0; a < 4; ++a) out.q[a] = static_cast<float>(r.q[a]);
  return out;
}

// Eigen QuaternionBase::_transformVector (cross products in coefficient order).
template <typename T>
inline void Rotate(const T q[4], const T v[3], T out[3]) {
  T uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
  for (T& c : uv) c += c;
  const T c[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2],
                  q[1] * uv[1] - q[2] * uv[0]};
  for (int a = 0; a < 3; ++a) out[a] = (v[a] + q[0] * uv[a]) + c[a];
}

// Rigid3 * Rigid3 (rigid_transform.h:181-188): Eigen's quaternion product,
// normalized (coeffs / norm, the squared norm summed as the packet reduction
// does over (x, y, z, w) storage).
template <typename T>
inline Rigid3<T> Mul(const Rigid3<T>& a, const Rigid3<T>& b) {
  Rigid3<T> out;
  T v[3];
  Rotate(a.q, b.t, v);
  for (int k = 0; k < 3; ++k) out.t[k] = v[k] + a.t[k];
  const T* p = a.q;
  const T* r = b.q;
  const T w = p[0] * r[0] - p[1] * r[1] - p[2] * r[2] - p[3] * r[3];
  const T x = p[0] * r[1] + p[1] * r[0] + p[2] * r[3] - p[3] * r[2];
  const T y = p[0] * r[2] + p[2] * r[0] + p[3] * r[1] - p[1] * r[3];
  const T z = p[0] * r[3] + p[3] * r[0] + p[1] * r[2] - p[2] * r[1];
  const T n = std::sqrt((x * x + z * z) + (y * y + w * w));
  if (n > T(0)) {
    out.q[0] = w / n, out.q[1] = x / n, out.q[2] = y / n, out.q[3] = z / n;
  } else {
    out.q[0] = w, out.q[1] = x, out.q[2] = y, out.q[3] = z;
  }
  return out;
}

// Rigid3::inverse (rigid_transform.h:150-154).
template <typename T>
inline Rigid3<T> Inverse(const Rigid3<T>& r) {
  Rigid3<T> out;
  out.q[0] = r.q[0], out.q[1] = -r.q[1], out.q[2] = -r.q[2], out.q[3] = -r.q[3];
  T v[3];
  Rotate(out.q, r.t, v);
  for (int a = 0; a < 3; ++a) out.t[a] = -v[a];
  return out;
}

// Eigen's redux of a 3-vector: x0 + (x1 + x2).
inline double Norm3(double x, double y, double z) { return std::sqrt(x * x + (y * y + z * z)); }

// transform::GetAngle (transform.h:34-37).
inline double GetAngle(const Rigid3<double>& r) {
  return 2. * std::atan2(Norm3(r.q[1], r.q[2], r.q[3]), std::abs(r.q[0]));
}

// transform::Project2D (transform.h:103-106) with GetYaw (:43-47).
inline Rigid2d Project2D(const Rigid3<double>& r) {
  const double unit_x[3] = {1., 0., 0.};
  double d[3];
  Rotate(r.q, unit_x, d);
  return Rigid2d{r.t[0], r.t[1], std::atan2(d[1], d[0])};
}

// transform::Embed3D (transform.h:110-115): AngleAxis(angle, UnitZ) as a
// quaternion (w = cos(angle / 2), vec = sin(angle / 2) * axis).
template <typename T>
inline Rigid3<T> Embed3D(T x, T y, T angle) {
  Rigid3<T> out;
  out.t[0] = x, out.t[1] = y, out.t[2] = T(0);
  const T ha = T(0.5) * angle;
  const T s = std::sin(ha);
  out.q[0] = std::cos(ha), out.q[1] = s * T(0), out.q[2] = s * T(0), out.q[3] = s * T(1);
  return out;
}

inline void ToArray(const Rigid3<float>& r, float out[7]) {
  for (int a = 0; a < 3; ++a) out[a] = r.t[a];
  for (int a = 0; a < 4; ++a) out[3 + a] = r.q[a];
}

}  // namespace local_2d_internal

// proto::MotionFilterOptions (trajectory_builder_2d.lua:56-60 defaults).
struct MotionFilterOptions {
  double max_time_seconds = 5.;
  double max_distance_meters = 0.2;
  double max_angle_radians = 1. * M_PI / 180.;
};

// motion_filter.h:34-49: takes poses, and filters them so that only poses
// that differ enough in time, distance or angle from the last kept one pass.
class MotionFilter {
 public:
  explicit MotionFilter(const MotionFilterOptions& options) : options_(options) {}

  // motion_filter.cc:40-58 without the log line. True: similar, drop it.
  bool IsSimilar(double time, const Rigid3d& pose) {
    namespace in = local_2d_internal;
    const in::Rigid3<double> p = in::FromRigid3d(pose);
    ++num_total_;
    if (num_total_ > 1 && time - last_time_ <= options_.max_time_seconds &&
        in::Norm3(p.t[0] - last_pose_.t[0], p.t[1] - last_pose_.t[1], p.t[2] - last_pose_.t[2]) <=
            options_.max_distance_meters &&
        in::GetAngle(in::Mul(in::Inverse(p), last_pose_)) <= options_.max_angle_radians) {
      return true;
    }
    last_time_ = time;
    last_pose_ = p;
    ++num_different_;
    return false;
  }

 private:
  MotionFilterOptions options_;
  int num_total_ = 0;
  int num_different_ = 0;
  double last_time_ = 0.;
  local_2d_internal::Rigid3<double> last_pose_;
};

// proto::LocalTrajectoryBuilderOptions2D, the fields this builder reads
// (trajectory_builder_2d.lua:17-60 defaults; submaps: :87-114).
struct LocalTrajectoryBuilderOptions2D {
  float min_range = 0.f;
  float max_range = 30.f;
  float min_z = -0.8f;
  float max_z = 2.f;
  float missing_data_ray_length = 5.f;
  int num_accumulated_range_data = 1;
  float voxel_filter_size = 0.025f;
  csm_adaptive_voxel_filter_options adaptive_voxel_filter_options{0.5f, 200.f, 50.f};
  bool use_online_correlative_scan_matching = false;
  RealTimeCorrelativeScanMatcherOptions real_time_correlative_scan_matcher_options;
  CeresScanMatcherOptions2D ceres_scan_matcher_options;
  MotionFilterOptions motion_filter_options;
  SubmapsOptions2D submaps_options;
};

// mapping/pose_extrapolator_interface.h:36-78, the methods the 2D builder calls.
class PoseExtrapolatorInterface {
 public:
  virtual ~PoseExtrapolatorInterface() {}
  virtual double GetLastPoseTime() const = 0;
  virtual double GetLastExtrapolatedTime() const = 0;
  virtual Rigid3d ExtrapolatePose(double time) = 0;
  // The rotation to the gravity-aligned frame.
  virtual Quaterniond EstimateGravityOrientation(double time) = 0;
  virtual void AddPose(double time, const Rigid3d& pose) = 0;
};

// sensor::TimedPointCloudOriginData::RangeMeasurement
// (sensor/timed_point_cloud_data.h:36-40): a point, its time relative to the
// sweep's (<= 0) and the index of the origin it was measured from.
struct RangeMeasurement {
  float position[3];
  float time;
  int32_t origin_index;
};

// TrajectoryNode::Data (trajectory_node.h:45-63), the fields the 2D builder fills.
struct TrajectoryNodeData2D {
  double time;
  Quaterniond gravity_alignment;
  PointCloud filtered_gravity_aligned_point_cloud;
  Rigid3d local_pose;
};

class LocalTrajectoryBuilder2D {
 public:
  // local_trajectory_builder_2d.h:49-62
  struct InsertionResult {
    std::shared_ptr<const TrajectoryNodeData2D> constant_data;
    std::vector<std::shared_ptr<const Submap2D>> insertion_submaps;
  };
  struct MatchingResult {
    double time;
    Rigid3d local_pose;
    RangeData range_data_in_local;
    // 'nullptr' if dropped by the motion filter.
    std::unique_ptr<const InsertionResult> insertion_result;
  };

  LocalTrajectoryBuilder2D(const LocalTrajectoryBuilderOptions2D& options,
                           PoseExtrapolatorInterface* extrapolator,
                           csm_context* context = nullptr)
      : options_(options),
        context_(context ? context : ThreadContext()),
        extrapolator_(extrapolator),
        active_submaps_(options.submaps_options, context_),
        motion_filter_(options.motion_filter_options),
        real_time_correlative_scan_matcher_(options.real_time_correlative_scan_matcher_options),
        ceres_scan_matcher_(options.ceres_scan_matcher_options) {}

  LocalTrajectoryBuilder2D(const LocalTrajectoryBuilder2D&) = delete;
  LocalTrajectoryBuilder2D& operator=(const LocalTrajectoryBuilder2D&) = delete;

  const ActiveSubmaps2D& active_submaps() const { return active_submaps_; }

  // .cc:104-209 on synchronized data. The raw points and their poses are kept
  // on the host until num_accumulated_range_data calls have come; then the
  // whole accumulation goes through one device call. nullptr: no result yet
  // (the early returns of :110-137, or still accumulating) or none at all.
  std::unique_ptr<MatchingResult> AddRangeData(double time, const std::vector<float>& origins_xyz,
                                               const std::vector<RangeMeasurement>& ranges) {
    namespace in = local_2d_internal;
    if (ranges.empty() || extrapolator_ == nullptr) return nullptr;  // :110-113, :121-126
    CheckOk(ranges.back().time <= 0.f ? CSM_OK : CSM_EINVAL, "AddRangeData");  // :130
    const double time_first_point = time + static_cast<double>(ranges.front().time);
    if (time_first_point < extrapolator_->GetLastPoseTime()) return nullptr;  // :131-137
    if (num_accumulated_ == 0) ClearAccumulation();
    in::Rigid3<float> last_pose;
    const int32_t origin_base = static_cast<int32_t>(origins_.size() / 3);
    for (const RangeMeasurement& range : ranges) {
      double time_point = time + static_cast<double>(range.time);
      if (time_point < extrapolator_->GetLastExtrapolatedTime())  // :144-152
        time_point = extrapolator_->GetLastExtrapolatedTime();
      last_pose = in::Cast(in::FromRigid3d(extrapolator_->ExtrapolatePose(time_point)));
      float tq[7];
      in::ToArray(last_pose, tq);
      poses_.insert(poses_.end(), tq, tq + 7);
      hits_.insert(hits_.end(), range.position, range.position + 3);
      origin_index_.push_back(origin_base + range.origin_index);
    }
    origins_.insert(origins_.end(), origins_xyz.begin(), origins_xyz.end());
    ++num_accumulated_;
    if (num_accumulated_ < options_.num_accumulated_range_data) return nullptr;
    num_accumulated_ = 0;
    Rigid3d gravity_alignment = Rigid3d::Rotation(extrapolator_->EstimateGravityOrientation(time));
    // gravity_alignment.cast<float>() * range_data_poses.back().inverse() (:204).
    float gravity_from_local[7];
    in::ToArray(in::Mul(in::Cast(in::FromRigid3d(gravity_alignment)), in::Inverse(last_pose)),
                gravity_from_local);
    const csm_range_data2d_options o{options_.min_range,
                                     options_.max_range,
                                     options_.missing_data_ray_length,
                                     options_.min_z,
                                     options_.max_z,
                                     options_.voxel_filter_size,
                                     options_.adaptive_voxel_filter_options};
    const int32_t n = static_cast<int32_t>(origin_index_.size());
    RangeData gravity_aligned_range_data;
    PointCloud filtered;
    gravity_aligned_range_data.returns.xyz.resize(3 * static_cast<size_t>(n));
    gravity_aligned_range_data.misses.xyz.resize(3 * static_cast<size_t>(n));
    filtered.xyz.resize(3 * static_cast<size_t>(n));
    int32_t num_returns = 0, num_misses = 0, num_filtered = 0;
    CheckOk(csm_range_data2d_prepare(
                context_, &o, hits_.data(), origin_index_.data(), poses_.data(), n,
                origins_.data(), static_cast<int32_t>(origins_.size() / 3), gravity_from_local,
                last_pose.t, gravity_aligned_range_data.origin,
                gravity_aligned_range_data.returns.xyz.data(), &num_returns,
                gravity_aligned_range_data.misses.xyz.data(), &num_misses, filtered.xyz.data(),
                &num_filtered),
            "csm_range_data2d_prepare");
    gravity_aligned_range_data.returns.xyz.resize(3 * static_cast<size_t>(num_returns));
    gravity_aligned_range_data.misses.xyz.resize(3 * static_cast<size_t>(num_misses));
    filtered.xyz.resize(3 * static_cast<size_t>(num_filtered));
    ClearAccumulation();
    return AddAccumulatedRangeData(time, gravity_aligned_range_data, gravity_alignment, filtered);
  }

  // .cc:211-277 without the wall-clock metrics; the adaptive voxel filter of
  // :228-231 has already run on the device.
  std::unique_ptr<MatchingResult> AddAccumulatedRangeData(
      double time, const RangeData& gravity_aligned_range_data, const Rigid3d& gravity_alignment,
      const PointCloud& filtered_gravity_aligned_point_cloud) {
    namespace in = local_2d_internal;
    if (gravity_aligned_range_data.returns.size() == 0) return nullptr;
    const in::Rigid3<double> alignment = in::FromRigid3d(gravity_alignment);
    const in::Rigid3<double> non_gravity_aligned_pose_prediction =
        in::FromRigid3d(extrapolator_->ExtrapolatePose(time));
    const Rigid2d pose_prediction =
        in::Project2D(in::Mul(non_gravity_aligned_pose_prediction, in::Inverse(alignment)));
    if (filtered_gravity_aligned_point_cloud.size() == 0) return nullptr;
    std::unique_ptr<Rigid2d> pose_estimate_2d =
        ScanMatch(time, pose_prediction, filtered_gravity_aligned_point_cloud);
    if (pose_estimate_2d == nullptr) return nullptr;
    const Rigid3d pose_estimate = in::ToRigid3d(in::Mul(
        in::Embed3D<double>(pose_estimate_2d->x, pose_estimate_2d->y, pose_estimate_2d->theta),
        alignment));
    extrapolator_->AddPose(time, pose_estimate);

    // TransformRangeData(gravity_aligned_range_data,
    //                    Embed3D(pose_estimate_2d->cast<float>())) (:246-248).
    float local_from_gravity_aligned[7];
    in::ToArray(in::Embed3D<float>(static_cast<float>(pose_estimate_2d->x),
                                   static_cast<float>(pose_estimate_2d->y),
                                   static_cast<float>(pose_estimate_2d->theta)),
                local_from_gravity_aligned);
    const RangeData& g = gravity_aligned_range_data;
    RangeData range_data_in_local;
    range_data_in_local.returns.xyz.resize(g.returns.xyz.size());
    range_data_in_local.misses.xyz.resize(g.misses.xyz.size());
    CheckOk(csm_range_data_transform(
                context_, local_from_gravity_aligned, g.origin, g.returns.xyz.data(),
                static_cast<int32_t>(g.returns.size()), g.misses.xyz.data(),
                static_cast<int32_t>(g.misses.size()), range_data_in_local.origin,
                range_data_in_local.returns.xyz.data(), range_data_in_local.misses.xyz.data()),
            "csm_range_data_transform");
    std::unique_ptr<InsertionResult> insertion_result =
        InsertIntoSubmap(time, range_data_in_local, filtered_gravity_aligned_point_cloud,
                         pose_estimate, gravity_alignment.rotation);
    std::unique_ptr<MatchingResult> result(new MatchingResult{
        time, pose_estimate, std::move(range_data_in_local), std::move(insertion_result)});
    return result;
  }

  // .cc:65-102: the real-time matcher (if enabled) refines the start of the
  // Ceres refinement, both on the first active submap's device grid.
  std::unique_ptr<Rigid2d> ScanMatch(double time, const Rigid2d& pose_prediction,
                                     const PointCloud& filtered_gravity_aligned_point_cloud) {
    (void)time;
    if (active_submaps_.submaps().empty())
      return std::unique_ptr<Rigid2d>(new Rigid2d(pose_prediction));
    std::shared_ptr<const Submap2D> matching_submap = active_submaps_.submaps().front();
    Rigid2d initial_ceres_pose = pose_prediction;
    const PointCloud& cloud = filtered_gravity_aligned_point_cloud;
    if (options_.use_online_correlative_scan_matching) {
      if (matching_submap->grid())
        MatchRealTime(options_.real_time_correlative_scan_matcher_options, pose_prediction, cloud,
                      *matching_submap->grid(), &initial_ceres_pose);
      else
        real_time_correlative_scan_matcher_.Match(pose_prediction, cloud, *matching_submap->tsdf(),
                                                  &initial_ceres_pose);
    }
    std::unique_ptr<Rigid2d> pose_observation(new Rigid2d());
    const double target_translation[2] = {pose_prediction.x, pose_prediction.y};
    if (matching_submap->grid())
      ceres_scan_matcher_.Match(target_translation, initial_ceres_pose, cloud,
                                *matching_submap->grid(), pose_observation.get());
    else
      ceres_scan_matcher_.Match(target_translation, initial_ceres_pose, cloud,
                                *matching_submap->tsdf(), pose_observation.get());
    return pose_observation;
  }

  // .cc:279-300
  std::unique_ptr<InsertionResult> InsertIntoSubmap(
      double time, const RangeData& range_data_in_local,
      const PointCloud& filtered_gravity_aligned_point_cloud, const Rigid3d& pose_estimate,
      const Quaterniond& gravity_alignment) {
    if (motion_filter_.IsSimilar(time, pose_estimate)) return nullptr;
    std::vector<std::shared_ptr<const Submap2D>> insertion_submaps =
        active_submaps_.InsertRangeData(range_data_in_local);
    std::unique_ptr<InsertionResult> result(new InsertionResult{
        std::make_shared<const TrajectoryNodeData2D>(TrajectoryNodeData2D{
            time, gravity_alignment, filtered_gravity_aligned_point_cloud, pose_estimate}),
        std::move(insertion_submaps)});
    return result;
  }

 private:
  void ClearAccumulation() {
    hits_.clear();
    origin_index_.clear();
    poses_.clear();
    origins_.clear();
  }

  const LocalTrajectoryBuilderOptions2D options_;
  csm_context* context_;
  PoseExtrapolatorInterface* extrapolator_;
  ActiveSubmaps2D active_submaps_;
  MotionFilter motion_filter_;
  RealTimeCorrelativeScanMatcher2D real_time_correlative_scan_matcher_;
  CeresScanMatcher2D ceres_scan_matcher_;
  // The accumulation: raw hits, their origins and per-point poses.
  int num_accumulated_ = 0;
  std::vector<float> hits_, poses_, origins_;
  std::vector<int32_t> origin_index_;
};

}  // namespace cartographer_amd

#endif  // CARTOGRAPHER_AMD_LOCAL_TRAJECTORY_BUILDER_2D_H_
