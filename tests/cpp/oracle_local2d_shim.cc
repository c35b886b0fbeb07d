// TEST INFRASTRUCTURE ONLY. The CPU restatement the LocalTrajectoryBuilder2D
// tests compare the device front end and the drop-in with, written from
//   mapping/internal/2d/local_trajectory_builder_2d.cc:51-63, :163-207, :222-248
//   sensor/range_data.cc:25-44, sensor/point_cloud.cc:76-81
//   mapping/internal/motion_filter.cc:40-58, transform/transform.h:34-47, :103-115
// over the oracle's Apply, Mul, Inverse, TransformPointCloud, VoxelFilter and
// AdaptiveVoxelFilterIndices (oracle/geometry.cc, oracle/voxel_filter.cc).
// Rigid3 arguments are (t x y z, q w x y z); Rigid2d ones (x, y, angle).
#include <cmath>
#include <cstdint>
#include <vector>

#include "csm_oracle.h"
#include "oracle_voxel.h"

using oracle::PointCloud;
using oracle::Quatd;
using oracle::Quatf;
using oracle::Rigid2d;
using oracle::Rigid2f;
using oracle::Rigid3d;
using oracle::Rigid3f;
using oracle::Vec3d;
using oracle::Vec3f;

namespace {

Rigid3f LoadF(const float* p) {
  return Rigid3f{Vec3f{p[0], p[1], p[2]}, Quatf{p[3], p[4], p[5], p[6]}};
}
Rigid3d LoadD(const double* p) {
  return Rigid3d{Vec3d{p[0], p[1], p[2]}, Quatd{p[3], p[4], p[5], p[6]}};
}
void StoreF(const Rigid3f& r, float* p) {
  p[0] = r.t.x, p[1] = r.t.y, p[2] = r.t.z;
  p[3] = r.q.w, p[4] = r.q.x, p[5] = r.q.y, p[6] = r.q.z;
}
void StoreD(const Rigid3d& r, double* p) {
  p[0] = r.t.x, p[1] = r.t.y, p[2] = r.t.z;
  p[3] = r.q.w, p[4] = r.q.x, p[5] = r.q.y, p[6] = r.q.z;
}
Rigid3d RotationD(const double* q) {
  return Rigid3d{Vec3d{0., 0., 0.}, Quatd{q[0], q[1], q[2], q[3]}};
}

// rigid_transform.h:150-154 in float.
Rigid3f InverseF(const Rigid3f& a) {
  const Quatf c{a.q.w, -a.q.x, -a.q.y, -a.q.z};
  const Vec3f t = oracle::Rotate(c, a.t);
  return Rigid3f{Vec3f{-t.x, -t.y, -t.z}, c};
}

// Eigen's redux of a 3-vector: x0 + (x1 + x2).
float Norm3(const Vec3f& v) { return std::sqrt(v.x * v.x + (v.y * v.y + v.z * v.z)); }
double Norm3(const Vec3d& v) { return std::sqrt(v.x * v.x + (v.y * v.y + v.z * v.z)); }

void StoreCloud(const PointCloud& cloud, float* out, int32_t* count) {
  *count = static_cast<int32_t>(cloud.size());
  for (size_t i = 0; i < cloud.size(); ++i) {
    out[3 * i] = cloud[i].x;
    out[3 * i + 1] = cloud[i].y;
    out[3 * i + 2] = cloud[i].z;
  }
}
PointCloud LoadCloud(const float* xyz, int32_t n) {
  PointCloud cloud;
  cloud.reserve(n);
  for (int32_t i = 0; i < n; ++i)
    cloud.push_back(Vec3f{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
  return cloud;
}

// sensor/point_cloud.cc:76-81
PointCloud CropPointCloud(const PointCloud& cloud, float min_z, float max_z) {
  PointCloud out;
  for (const Vec3f& p : cloud)
    if (min_z <= p.z && p.z <= max_z) out.push_back(p);
  return out;
}

// motion_filter.h:34-49; times in seconds.
struct MotionFilter {
  double max_time_seconds, max_distance_meters, max_angle_radians;
  int num_total = 0, num_different = 0;
  double last_time = 0.;
  Rigid3d last_pose{Vec3d{0., 0., 0.}, Quatd{1., 0., 0., 0.}};
};

}  // namespace

extern "C" {

// AddRangeData :163-185, TransformToGravityAlignedFrameAndFilter :51-63 and
// AdaptiveVoxelFilter :228-231. options: min_range, max_range,
// missing_data_ray_length, min_z, max_z, voxel_filter_size, then the adaptive
// filter's max_length, min_num_points, max_range.
void shiml_prepare(const float* options, const float* hits, const int32_t* origin_index,
                   const float* poses, int32_t n, const float* origins,
                   const float* gravity_from_local, const float* local_origin, float* origin_out,
                   float* returns_out, int32_t* num_returns, float* misses_out,
                   int32_t* num_misses, float* filtered_out, int32_t* num_filtered) {
  const float min_range = options[0], max_range = options[1], missing_data_ray_length = options[2];
  PointCloud returns, misses;
  for (int32_t i = 0; i < n; ++i) {
    const Rigid3f pose = LoadF(poses + 7 * i);
    const float* o = origins + 3 * origin_index[i];
    const Vec3f origin_in_local = oracle::Apply(pose, Vec3f{o[0], o[1], o[2]});
    Vec3f hit_in_local = oracle::Apply(pose, Vec3f{hits[3 * i], hits[3 * i + 1], hits[3 * i + 2]});
    const Vec3f delta{hit_in_local.x - origin_in_local.x, hit_in_local.y - origin_in_local.y,
                      hit_in_local.z - origin_in_local.z};
    const float range = Norm3(delta);
    if (range >= min_range) {
      if (range <= max_range) {
        returns.push_back(hit_in_local);
      } else {
        const float s = missing_data_ray_length / range;
        hit_in_local = Vec3f{origin_in_local.x + s * delta.x, origin_in_local.y + s * delta.y,
                             origin_in_local.z + s * delta.z};
        misses.push_back(hit_in_local);
      }
    }
  }
  const Rigid3f g = LoadF(gravity_from_local);
  const Vec3f origin = oracle::Apply(g, Vec3f{local_origin[0], local_origin[1], local_origin[2]});
  origin_out[0] = origin.x, origin_out[1] = origin.y, origin_out[2] = origin.z;
  const PointCloud cropped_returns =
      CropPointCloud(oracle::TransformPointCloud(returns, g), options[3], options[4]);
  const PointCloud cropped_misses =
      CropPointCloud(oracle::TransformPointCloud(misses, g), options[3], options[4]);
  const PointCloud filtered_returns = oracle::VoxelFilter(cropped_returns, options[5]);
  StoreCloud(filtered_returns, returns_out, num_returns);
  StoreCloud(oracle::VoxelFilter(cropped_misses, options[5]), misses_out, num_misses);
  oracle::AdaptiveVoxelFilterOptions a;
  a.max_length = options[6];
  a.min_num_points = options[7];
  a.max_range = options[8];
  PointCloud filtered;
  for (int index : oracle::AdaptiveVoxelFilterIndices(filtered_returns, a))
    filtered.push_back(filtered_returns[index]);
  StoreCloud(filtered, filtered_out, num_filtered);
}

// sensor::TransformRangeData (range_data.cc:25-32).
void shiml_transform(const float* transform, const float* origin, const float* returns,
                     int32_t num_returns, const float* misses, int32_t num_misses,
                     float* origin_out, float* returns_out, float* misses_out) {
  const Rigid3f r = LoadF(transform);
  const Vec3f o = oracle::Apply(r, Vec3f{origin[0], origin[1], origin[2]});
  origin_out[0] = o.x, origin_out[1] = o.y, origin_out[2] = o.z;
  int32_t count;
  StoreCloud(oracle::TransformPointCloud(LoadCloud(returns, num_returns), r), returns_out, &count);
  StoreCloud(oracle::TransformPointCloud(LoadCloud(misses, num_misses), r), misses_out, &count);
}

// gravity_alignment.cast<float>() * range_data_poses.back().inverse() (:204).
void shiml_gravity_from_local(const double* gravity_q, const float* last_pose, float* out) {
  StoreF(oracle::Mul(oracle::CastF(RotationD(gravity_q)), InverseF(LoadF(last_pose))), out);
}

// Project2D(non_gravity_aligned_pose_prediction * gravity_alignment.inverse())
// (:223-226; transform.h:43-47, :103-106).
void shiml_pose_prediction(const double* pose, const double* gravity_q, double* out) {
  const Rigid3d p = oracle::Mul(LoadD(pose), oracle::Inverse(RotationD(gravity_q)));
  const Vec3d direction = oracle::Rotate(p.q, Vec3d{1., 0., 0.});
  out[0] = p.t.x;
  out[1] = p.t.y;
  out[2] = std::atan2(direction.y, direction.x);
}

// Embed3D(*pose_estimate_2d) * gravity_alignment (:242-243).
void shiml_pose_estimate(const double* pose2d, const double* gravity_q, double* out) {
  StoreD(oracle::Mul(oracle::Embed3D(Rigid2d{pose2d[0], pose2d[1], pose2d[2]}),
                     RotationD(gravity_q)),
         out);
}

// Embed3D(pose_estimate_2d->cast<float>()) (:248).
void shiml_embed3d_f(const double* pose2d, float* out) {
  StoreF(oracle::Embed3D(Rigid2f{static_cast<float>(pose2d[0]), static_cast<float>(pose2d[1]),
                                 static_cast<float>(pose2d[2])}),
         out);
}

void* shiml_motion_filter_create(double max_time_seconds, double max_distance_meters,
                                 double max_angle_radians) {
  return new MotionFilter{max_time_seconds, max_distance_meters, max_angle_radians};
}
void shiml_motion_filter_destroy(void* filter) { delete static_cast<MotionFilter*>(filter); }

// MotionFilter::IsSimilar (motion_filter.cc:40-58) without the log line.
int32_t shiml_motion_filter_is_similar(void* filter, double time, const double* pose7) {
  MotionFilter& f = *static_cast<MotionFilter*>(filter);
  const Rigid3d pose = LoadD(pose7);
  ++f.num_total;
  if (f.num_total > 1 && time - f.last_time <= f.max_time_seconds &&
      Norm3(Vec3d{pose.t.x - f.last_pose.t.x, pose.t.y - f.last_pose.t.y,
                  pose.t.z - f.last_pose.t.z}) <= f.max_distance_meters) {
    // transform::GetAngle (transform.h:34-37).
    const Rigid3d d = oracle::Mul(oracle::Inverse(pose), f.last_pose);
    const double angle = 2. * std::atan2(Norm3(Vec3d{d.q.x, d.q.y, d.q.z}), std::abs(d.q.w));
    if (angle <= f.max_angle_radians) return 1;
  }
  f.last_time = time;
  f.last_pose = pose;
  ++f.num_different;
  return 0;
}

}  // extern "C"
