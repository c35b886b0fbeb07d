// TEST INFRASTRUCTURE ONLY. The CPU restatement the LocalTrajectoryBuilder3D
// tests compare the large voxel filters, the 3D range-data front end and the
// builder's host arithmetic with, written from
//   mapping/internal/3d/local_trajectory_builder_3d.cc:636-669, :680-683,
//     :696-698, :734-745, :898-909
//   sensor/internal/voxel_filter.cc:31-76, :263-268
//   sensor/range_data.cc:25-32, transform/rigid_transform.h:150-154
// over the oracle's Apply, Inverse, TransformPointCloud, VoxelFilter,
// AdaptiveVoxelFilterIndices and ComputeHistogram (oracle/geometry.cc,
// oracle/voxel_filter.cc, oracle/match3d.cc).
// Rigid3 arguments are (t x y z, q w x y z); quaternions (w, x, y, z).
#include <cmath>
#include <cstdint>
#include <vector>

#include "csm_oracle.h"
#include "oracle3d.h"
#include "oracle_voxel.h"

using oracle::PointCloud;
using oracle::Quatd;
using oracle::Quatf;
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

// Eigen's redux of a 3-vector: x0 + (x1 + x2).
float Norm3(const Vec3f& v) { return std::sqrt(v.x * v.x + (v.y * v.y + v.z * v.z)); }

PointCloud LoadCloud(const float* xyz, int32_t n) {
  PointCloud cloud;
  cloud.reserve(n);
  for (int32_t i = 0; i < n; ++i)
    cloud.push_back(Vec3f{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
  return cloud;
}

void StoreCloud(const PointCloud& cloud, const std::vector<float>& intensities, float* out,
                float* intensities_out, int32_t* count) {
  *count = static_cast<int32_t>(cloud.size());
  for (size_t i = 0; i < cloud.size(); ++i) {
    out[3 * i] = cloud[i].x;
    out[3 * i + 1] = cloud[i].y;
    out[3 * i + 2] = cloud[i].z;
    if (intensities_out) intensities_out[i] = intensities[i];
  }
}

struct Filtered {
  PointCloud points;
  std::vector<float> intensities;
};

Filtered Select(const PointCloud& cloud, const std::vector<float>& intensities,
                const std::vector<int>& kept) {
  Filtered out;
  for (int i : kept) {
    out.points.push_back(cloud[i]);
    if (!intensities.empty()) out.intensities.push_back(intensities[i]);
  }
  return out;
}

// AdaptiveVoxelFilter (:263-268): FilterByMaxRange (:31-36), then
// AdaptivelyVoxelFiltered (:38-76) over oracle::VoxelFilter, counting its
// VoxelFilter calls. Returns indices into `cloud`.
std::vector<int> AdaptiveCounted(const PointCloud& cloud,
                                 const oracle::AdaptiveVoxelFilterOptions& o, int32_t* passes) {
  *passes = 0;
  std::vector<int> in_range;
  PointCloud ranged;
  for (size_t i = 0; i < cloud.size(); ++i)
    if (Norm3(cloud[i]) <= o.max_range) {
      in_range.push_back(static_cast<int>(i));
      ranged.push_back(cloud[i]);
    }
  if (ranged.size() <= o.min_num_points) return in_range;
  std::vector<int> result, candidate;
  auto filter = [&](float length, std::vector<int>* kept) {
    ++*passes;
    kept->clear();
    oracle::VoxelFilter(ranged, length, kept);
  };
  auto finish = [&](const std::vector<int>& kept) {
    std::vector<int> out;
    for (int j : kept) out.push_back(in_range[j]);
    return out;
  };
  filter(o.max_length, &result);
  if (result.size() >= o.min_num_points) return finish(result);
  for (float high_length = o.max_length; high_length > 1e-2f * o.max_length; high_length /= 2.f) {
    float low_length = high_length / 2.f;
    filter(low_length, &result);
    if (result.size() >= o.min_num_points) {
      while ((high_length - low_length) / low_length > 1e-1f) {
        const float mid_length = (low_length + high_length) / 2.f;
        filter(mid_length, &candidate);
        if (candidate.size() >= o.min_num_points) {
          low_length = mid_length;
          result = candidate;
        } else {
          high_length = mid_length;
        }
      }
      return finish(result);
    }
  }
  return finish(result);
}

oracle::AdaptiveVoxelFilterOptions AdaptiveOptions(const float* o) {
  oracle::AdaptiveVoxelFilterOptions a;
  a.max_length = o[0];
  a.min_num_points = o[1];
  a.max_range = o[2];
  return a;
}

}  // namespace

extern "C" {

// AdaptiveVoxelFilter's keep mask and the number of VoxelFilter passes.
// Returns 1 when the counted restatement and the oracle's
// AdaptiveVoxelFilterIndices agree, 0 otherwise.
int32_t shim3_adaptive(const float* xyz, int32_t n, const float* options, uint8_t* keep,
                       int32_t* passes) {
  const PointCloud cloud = LoadCloud(xyz, n);
  const oracle::AdaptiveVoxelFilterOptions o = AdaptiveOptions(options);
  const std::vector<int> kept = AdaptiveCounted(cloud, o, passes);
  for (int32_t i = 0; i < n; ++i) keep[i] = 0;
  for (int i : kept) keep[i] = 1;
  return kept == oracle::AdaptiveVoxelFilterIndices(cloud, o) ? 1 : 0;
}

// The front end. options: min_range, max_range, voxel_filter_size, then the
// high and the low resolution adaptive filters' max_length, min_num_points,
// max_range. intensities and the intensity outputs may be null. passes[0..1]:
// the VoxelFilter passes of the high and the low adaptive filter.
void shim3_prepare(const float* options, const float* hits, const float* intensities,
                   const int32_t* origin_index, const float* poses, int32_t n,
                   const float* origins, const float* tracking_from_local,
                   const float* local_origin, float* origin_out, float* returns_out,
                   float* returns_intensities_out, int32_t* num_returns, float* misses_out,
                   int32_t* num_misses, float* high_out, float* high_intensities_out,
                   int32_t* num_high, float* low_out, float* low_intensities_out,
                   int32_t* num_low, int32_t* passes) {
  const float min_range = options[0], max_range = options[1], voxel_filter_size = options[2];
  PointCloud returns, misses;
  std::vector<float> returns_intensities;
  for (int32_t i = 0; i < n; ++i) {
    const Rigid3f pose = LoadF(poses + 7 * i);
    const float* o = origins + 3 * origin_index[i];
    const Vec3f hit_in_local =
        oracle::Apply(pose, Vec3f{hits[3 * i], hits[3 * i + 1], hits[3 * i + 2]});
    const Vec3f origin_in_local = oracle::Apply(pose, Vec3f{o[0], o[1], o[2]});
    const Vec3f delta{hit_in_local.x - origin_in_local.x, hit_in_local.y - origin_in_local.y,
                      hit_in_local.z - origin_in_local.z};
    const float range = Norm3(delta);
    if (range >= min_range) {
      if (range <= max_range) {
        returns.push_back(hit_in_local);
        if (intensities) returns_intensities.push_back(intensities[i]);
      } else {
        const float s = max_range / range;
        misses.push_back(Vec3f{origin_in_local.x + s * delta.x, origin_in_local.y + s * delta.y,
                               origin_in_local.z + s * delta.z});
      }
    }
  }
  std::vector<int> kept;
  oracle::VoxelFilter(returns, voxel_filter_size, &kept);
  const Filtered filtered_returns = Select(returns, returns_intensities, kept);
  const PointCloud filtered_misses = oracle::VoxelFilter(misses, voxel_filter_size);
  const Rigid3f t = LoadF(tracking_from_local);
  const Vec3f origin = oracle::Apply(t, Vec3f{local_origin[0], local_origin[1], local_origin[2]});
  origin_out[0] = origin.x, origin_out[1] = origin.y, origin_out[2] = origin.z;
  const PointCloud returns_in_tracking = oracle::TransformPointCloud(filtered_returns.points, t);
  StoreCloud(returns_in_tracking, filtered_returns.intensities, returns_out,
             intensities ? returns_intensities_out : nullptr, num_returns);
  StoreCloud(oracle::TransformPointCloud(filtered_misses, t), {}, misses_out, nullptr, num_misses);
  const Filtered high =
      Select(returns_in_tracking, filtered_returns.intensities,
             AdaptiveCounted(returns_in_tracking, AdaptiveOptions(options + 3), &passes[0]));
  StoreCloud(high.points, high.intensities, high_out, intensities ? high_intensities_out : nullptr,
             num_high);
  const Filtered low =
      Select(returns_in_tracking, filtered_returns.intensities,
             AdaptiveCounted(returns_in_tracking, AdaptiveOptions(options + 6), &passes[1]));
  StoreCloud(low.points, low.intensities, low_out, intensities ? low_intensities_out : nullptr,
             num_low);
}

// current_pose.inverse().cast<float>() (:698) and
// current_pose.translation().cast<float>() (:681).
void shim3_tracking_from_local(const double* pose, float* tracking_from_local,
                               float* local_origin) {
  const Rigid3d p = LoadD(pose);
  const Rigid3f inv = oracle::CastF(oracle::Inverse(p));
  tracking_from_local[0] = inv.t.x, tracking_from_local[1] = inv.t.y;
  tracking_from_local[2] = inv.t.z, tracking_from_local[3] = inv.q.w;
  tracking_from_local[4] = inv.q.x, tracking_from_local[5] = inv.q.y;
  tracking_from_local[6] = inv.q.z;
  local_origin[0] = static_cast<float>(p.t.x);
  local_origin[1] = static_cast<float>(p.t.y);
  local_origin[2] = static_cast<float>(p.t.z);
}

// ComputeHistogram(TransformPointCloud(returns,
// Rigid3f::Rotation(gravity_alignment.cast<float>())), size) (:898-903).
void shim3_histogram(const float* returns, int32_t n, const double* gravity_q, int32_t size,
                     float* out) {
  const Rigid3f r{Vec3f{0.f, 0.f, 0.f},
                  Quatf{static_cast<float>(gravity_q[0]), static_cast<float>(gravity_q[1]),
                        static_cast<float>(gravity_q[2]), static_cast<float>(gravity_q[3])}};
  const std::vector<float> h =
      oracle::ComputeHistogram(oracle::TransformPointCloud(LoadCloud(returns, n), r), size);
  for (int32_t i = 0; i < size; ++i) out[i] = h[i];
}

// pose_estimate.rotation() * gravity_alignment.inverse() (:908-909); Eigen's
// inverse is the conjugate over the squared norm (x^2 + z^2) + (y^2 + w^2).
void shim3_local_from_gravity_aligned(const double* pose_q, const double* gravity_q, double* out) {
  const Quatd g{gravity_q[0], gravity_q[1], gravity_q[2], gravity_q[3]};
  const double n2 = (g.x * g.x + g.z * g.z) + (g.y * g.y + g.w * g.w);
  const Quatd inv{g.w / n2, -g.x / n2, -g.y / n2, -g.z / n2};
  const Quatd r = oracle::QuatMul(Quatd{pose_q[0], pose_q[1], pose_q[2], pose_q[3]}, inv);
  out[0] = r.w, out[1] = r.x, out[2] = r.y, out[3] = r.z;
}

}  // extern "C"
