// The range-data front end of LocalTrajectoryBuilder3D on gfx950 (reference
// mapping/internal/3d/local_trajectory_builder_3d.cc): what turns one
// accumulated sweep of rangefinder points into the range data in the tracking
// frame and the two filtered clouds the 3D scan matchers search with.
//
// csm_range_data3d_prepare is one upload, one chain of launches on the
// context's stream and one download:
//   1. range_data3d_classify, one thread per point: hit and origin by the
//      point's own pose and the range test of AddRangeData (:636-669); every
//      point leaves it with its class (dropped, return, miss) and its position
//      in the local frame (a miss: the ray cropped to max_range);
//   2. the ordered split into returns (with intensities) and misses: the
//      compaction of voxel_filter_large.hip, per-block counts, their sums,
//      a scatter, once per class;
//   3. VoxelFilter of both clouds (:680-683) and their compaction;
//   4. range_data3d_transform of both by tracking_from_local (:696-698), into
//      the packed output;
//   5. AdaptiveVoxelFilter of the transformed returns with the high and the
//      low resolution options (:734-745) and the compaction of each.
// The voxel filters are voxel_filter_large.hip's; the host steers them by
// small read-backs (the two class counts, a report per filter pass, the
// range-filtered count of each adaptive filter), so it knows every count
// when it enqueues the step that needs it, packs the outputs back to back
// and downloads exactly what was produced.
// All arithmetic is float and non-contracted (-ffp-contract=off), in Eigen's
// order (rigid3_dev.h); sqrt and the division are correctly rounded.

#include <hip/hip_runtime.h>

#include <cstring>

#include "csm_internal.h"
#include "rigid3_dev.h"

namespace csm {
namespace {

constexpr int kRd3Threads = 256;
constexpr uint8_t kRd3Dropped = 0, kRd3Return = 1, kRd3Miss = 2;

__global__ void __launch_bounds__(kRd3Threads)
range_data3d_classify(const float* __restrict__ poses, const float* __restrict__ hits,
                      const int32_t* __restrict__ origin_index,
                      const float* __restrict__ origins, int n, float min_range, float max_range,
                      float* __restrict__ points, uint8_t* __restrict__ cls) {
  const int i = blockIdx.x * kRd3Threads + threadIdx.x;
  if (i >= n) return;
  const size_t at = 3 * static_cast<size_t>(i);
  const RdRigid3 pose = RdLoadRigid(poses + 7 * static_cast<size_t>(i));
  const float* op = origins + 3 * static_cast<size_t>(origin_index[i]);
  const RdVec3 o = RdApply(pose, RdVec3{op[0], op[1], op[2]});
  RdVec3 h = RdApply(pose, RdVec3{hits[at], hits[at + 1], hits[at + 2]});
  const RdVec3 delta{h.x - o.x, h.y - o.y, h.z - o.z};
  const float range = sqrtf(delta.x * delta.x + (delta.y * delta.y + delta.z * delta.z));
  uint8_t c = kRd3Dropped;
  if (range >= min_range) {  // a NaN range is dropped
    if (range <= max_range) {
      c = kRd3Return;
    } else {
      c = kRd3Miss;
      const float s = __fdiv_rn(max_range, range);
      h = RdVec3{o.x + s * delta.x, o.y + s * delta.y, o.z + s * delta.z};
    }
  }
  points[at] = h.x;
  points[at + 1] = h.y;
  points[at + 2] = h.z;
  cls[i] = c;
}

// sensor::TransformPointCloud (point_cloud.cc) by a Rigid3f.
__global__ void __launch_bounds__(kRd3Threads)
range_data3d_transform(const float* __restrict__ in, int count, RdRigid3 r,
                       float* __restrict__ out) {
  const int i = blockIdx.x * kRd3Threads + threadIdx.x;
  if (i >= count) return;
  const size_t at = 3 * static_cast<size_t>(i);
  const RdVec3 v = RdApply(r, RdVec3{in[at], in[at + 1], in[at + 2]});
  out[at] = v.x;
  out[at + 1] = v.y;
  out[at + 2] = v.z;
}

size_t Align256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

int Transform(hipStream_t st, const float* in, int count, const RdRigid3& r, float* out) {
  if (count == 0) return CSM_OK;
  hipLaunchKernelGGL(range_data3d_transform, dim3((count + kRd3Threads - 1) / kRd3Threads),
                     dim3(kRd3Threads), 0, st, in, count, r, out);
  CSM_HIP(hipGetLastError());
  return CSM_OK;
}

}  // namespace
}  // namespace csm

extern "C" {

int csm_range_data3d_prepare(csm_context* ctx, const csm_range_data3d_options* options,
                             const float* hits_xyz, const float* intensities,
                             const int32_t* origin_index, const float* poses_tq, int32_t n,
                             const float* origins_xyz, int32_t num_origins,
                             const float tracking_from_local_tq[7],
                             const float local_origin_xyz[3], float origin_out[3],
                             float* returns_out, float* returns_intensities_out,
                             int32_t* num_returns, float* misses_out, int32_t* num_misses,
                             float* high_out, float* high_intensities_out, int32_t* num_high,
                             float* low_out, float* low_intensities_out, int32_t* num_low) {
  using namespace csm;
  if (!ctx || !options || n < 0 || num_origins < 0 || !tracking_from_local_tq ||
      !local_origin_xyz || !origin_out || !num_returns || !num_misses || !num_high || !num_low)
    return CSM_EINVAL;
  if (!(options->voxel_filter_size > 0.f) ||
      !(options->high_resolution_adaptive_voxel_filter.max_length > 0.f) ||
      !(options->low_resolution_adaptive_voxel_filter.max_length > 0.f))
    return CSM_EINVAL;
  if (n > kVflMaxPoints) return CSM_ERANGE;
  const bool with_intensities = intensities != nullptr;
  if (n > 0) {
    if (!hits_xyz || !origin_index || !poses_tq || !origins_xyz || !returns_out || !misses_out ||
        !high_out || !low_out)
      return CSM_EINVAL;
    if (with_intensities &&
        (!returns_intensities_out || !high_intensities_out || !low_intensities_out))
      return CSM_EINVAL;
    for (int32_t i = 0; i < n; ++i)
      if (origin_index[i] < 0 || origin_index[i] >= num_origins) return CSM_EINVAL;
  }
  const float* g = tracking_from_local_tq;
  const RdRigid3 tracking_from_local{g[0], g[1], g[2], g[3], g[4], g[5], g[6]};
  // The origin is one point: moved here, by the arithmetic the kernels use.
  const RdVec3 origin = RdApply(
      tracking_from_local, RdVec3{local_origin_xyz[0], local_origin_xyz[1], local_origin_xyz[2]});
  origin_out[0] = origin.x;
  origin_out[1] = origin.y;
  origin_out[2] = origin.z;
  *num_returns = *num_misses = *num_high = *num_low = 0;
  if (n == 0) return CSM_OK;

  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t np = static_cast<size_t>(n), no = static_cast<size_t>(num_origins);
  // The upload: poses, hits, origin indices, intensities, origins.
  const size_t in_poses = 0, in_hits = in_poses + 28 * np, in_index = in_hits + 12 * np,
               in_intens = in_index + 4 * np,
               in_origins = in_intens + (with_intensities ? 4 * np : 0),
               in_bytes = in_origins + 12 * no;
  // The working set: the classified points, the raw and the filtered returns
  // (with intensities) and misses in the local frame, the high cloud's
  // intensities, a keep mask, the compactions' counts.
  const size_t cloud = Align256(12 * np), scalar = Align256(4 * np);
  const size_t w_points = 0, w_cls = w_points + cloud, w_raw_r = w_cls + Align256(np),
               w_raw_ri = w_raw_r + cloud, w_raw_m = w_raw_ri + scalar, w_fil_r = w_raw_m + cloud,
               w_fil_ri = w_fil_r + cloud, w_fil_m = w_fil_ri + scalar, w_high_i = w_fil_m + cloud,
               w_keep = w_high_i + scalar, w_counts = w_keep + Align256(np),
               w_bytes = w_counts + 256;
  // The download, packed: returns, misses, high, low, then the intensities of
  // returns, high and low. At most n points each.
  const size_t out_max = 12 * np * 4 + 4 * np * 3;
  int rc;
  if ((rc = VflReserve(ctx, n))) return rc;
  if ((rc = ctx->rd_in.Reserve(in_bytes))) return rc;
  if ((rc = ctx->rd_work.Reserve(w_bytes))) return rc;
  if ((rc = ctx->rd_out.Reserve(out_max))) return rc;
  if ((rc = ctx->rd_stage_in.Reserve(in_bytes))) return rc;
  hipStream_t st = ctx->stream;
  char* din = ctx->rd_in.as<char>();
  char* dw = ctx->rd_work.as<char>();
  char* dout = ctx->rd_out.as<char>();
  {
    char* s = ctx->rd_stage_in.as<char>();
    std::memcpy(s + in_poses, poses_tq, 28 * np);
    std::memcpy(s + in_hits, hits_xyz, 12 * np);
    std::memcpy(s + in_index, origin_index, 4 * np);
    if (with_intensities) std::memcpy(s + in_intens, intensities, 4 * np);
    std::memcpy(s + in_origins, origins_xyz, 12 * no);
    CSM_HIP(hipMemcpyAsync(din, s, in_bytes, hipMemcpyHostToDevice, st));
  }
  const float* d_intens = with_intensities ? reinterpret_cast<const float*>(din + in_intens) : nullptr;
  float* d_points = reinterpret_cast<float*>(dw + w_points);
  uint8_t* d_cls = reinterpret_cast<uint8_t*>(dw + w_cls);
  float* d_raw_r = reinterpret_cast<float*>(dw + w_raw_r);
  float* d_raw_ri = with_intensities ? reinterpret_cast<float*>(dw + w_raw_ri) : nullptr;
  float* d_raw_m = reinterpret_cast<float*>(dw + w_raw_m);
  float* d_fil_r = reinterpret_cast<float*>(dw + w_fil_r);
  float* d_fil_m = reinterpret_cast<float*>(dw + w_fil_m);
  uint8_t* d_keep = reinterpret_cast<uint8_t*>(dw + w_keep);
  int32_t* d_counts = reinterpret_cast<int32_t*>(dw + w_counts);

  hipLaunchKernelGGL(range_data3d_classify, dim3((n + kRd3Threads - 1) / kRd3Threads),
                     dim3(kRd3Threads), 0, st, reinterpret_cast<const float*>(din + in_poses),
                     reinterpret_cast<const float*>(din + in_hits),
                     reinterpret_cast<const int32_t*>(din + in_index),
                     reinterpret_cast<const float*>(din + in_origins), n, options->min_range,
                     options->max_range, d_points, d_cls);
  CSM_HIP(hipGetLastError());
  if ((rc = VflCompact(ctx, d_cls, kRd3Return, n, d_points, d_intens, d_raw_r, d_raw_ri, nullptr,
                       d_counts)))
    return rc;
  if ((rc = VflCompact(ctx, d_cls, kRd3Miss, n, d_points, nullptr, d_raw_m, nullptr, nullptr,
                       d_counts + 1)))
    return rc;
  int32_t raw[2] = {0, 0};
  CSM_HIP(hipMemcpyAsync(ctx->vfl_rb.ptr, d_counts, sizeof(raw), hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  std::memcpy(raw, ctx->vfl_rb.ptr, sizeof(raw));
  if (raw[0] < 0 || raw[1] < 0 || static_cast<int64_t>(raw[0]) + raw[1] > n) return CSM_EHIP;

  // VoxelFilter of the returns; the survivors' intensities go straight to the
  // output, the points wait for the transform.
  int32_t nr = 0, nm = 0, nh = 0, nl = 0;
  if ((rc = VflVoxelFilter(ctx, d_raw_r, raw[0], options->voxel_filter_size, d_keep, &nr)))
    return rc;
  const size_t o_returns = 0, o_misses = o_returns + 12 * static_cast<size_t>(nr);
  float* d_returns = reinterpret_cast<float*>(dout + o_returns);
  // The intensities' place in the output is known once every cloud is counted:
  // they stay in the working set until then.
  float* d_fil_ri = with_intensities ? reinterpret_cast<float*>(dw + w_fil_ri) : nullptr;
  if ((rc = VflCompact(ctx, d_keep, 1, raw[0], d_raw_r, d_raw_ri, d_fil_r, d_fil_ri, nullptr,
                       d_counts + 2)))
    return rc;
  if ((rc = VflVoxelFilter(ctx, d_raw_m, raw[1], options->voxel_filter_size, d_keep, &nm)))
    return rc;
  if ((rc = VflCompact(ctx, d_keep, 1, raw[1], d_raw_m, nullptr, d_fil_m, nullptr, nullptr,
                       d_counts + 3)))
    return rc;
  float* d_misses = reinterpret_cast<float*>(dout + o_misses);
  if ((rc = Transform(st, d_fil_r, nr, tracking_from_local, d_returns))) return rc;
  if ((rc = Transform(st, d_fil_m, nm, tracking_from_local, d_misses))) return rc;

  // AdaptiveVoxelFilter of the returns in the tracking frame, twice.
  if ((rc = VflAdaptiveVoxelFilter(ctx, d_returns, nr,
                                   &options->high_resolution_adaptive_voxel_filter, d_keep, &nh)))
    return rc;
  const size_t o_high = o_misses + 12 * static_cast<size_t>(nm);
  float* d_high = reinterpret_cast<float*>(dout + o_high);
  float* d_high_i = with_intensities ? reinterpret_cast<float*>(dw + w_high_i) : nullptr;
  if ((rc = VflCompact(ctx, d_keep, 1, nr, d_returns, d_fil_ri, d_high, d_high_i, nullptr,
                       d_counts + 4)))
    return rc;
  if ((rc = VflAdaptiveVoxelFilter(ctx, d_returns, nr,
                                   &options->low_resolution_adaptive_voxel_filter, d_keep, &nl)))
    return rc;
  const size_t o_low = o_high + 12 * static_cast<size_t>(nh);
  float* d_low = reinterpret_cast<float*>(dout + o_low);
  const size_t o_ri = o_low + 12 * static_cast<size_t>(nl), o_hi = o_ri + 4 * static_cast<size_t>(nr),
               o_li = o_hi + 4 * static_cast<size_t>(nh);
  float* d_low_i = with_intensities ? reinterpret_cast<float*>(dout + o_li) : nullptr;
  if ((rc = VflCompact(ctx, d_keep, 1, nr, d_returns, d_fil_ri, d_low, d_low_i, nullptr,
                       d_counts + 5)))
    return rc;
  size_t out_bytes = o_ri;
  if (with_intensities) {
    if (nr)
      CSM_HIP(hipMemcpyAsync(dout + o_ri, d_fil_ri, 4 * static_cast<size_t>(nr),
                             hipMemcpyDeviceToDevice, st));
    if (nh)
      CSM_HIP(hipMemcpyAsync(dout + o_hi, d_high_i, 4 * static_cast<size_t>(nh),
                             hipMemcpyDeviceToDevice, st));
    out_bytes = o_li + 4 * static_cast<size_t>(nl);
  }
  if (out_bytes > out_max) return CSM_EHIP;
  if (out_bytes > 0) {
    if ((rc = ctx->rd_stage_out.Reserve(out_bytes))) return rc;
    char* so = ctx->rd_stage_out.as<char>();
    CSM_HIP(hipMemcpyAsync(so, dout, out_bytes, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    if (nr) std::memcpy(returns_out, so + o_returns, 12 * static_cast<size_t>(nr));
    if (nm) std::memcpy(misses_out, so + o_misses, 12 * static_cast<size_t>(nm));
    if (nh) std::memcpy(high_out, so + o_high, 12 * static_cast<size_t>(nh));
    if (nl) std::memcpy(low_out, so + o_low, 12 * static_cast<size_t>(nl));
    if (with_intensities) {
      if (nr) std::memcpy(returns_intensities_out, so + o_ri, 4 * static_cast<size_t>(nr));
      if (nh) std::memcpy(high_intensities_out, so + o_hi, 4 * static_cast<size_t>(nh));
      if (nl) std::memcpy(low_intensities_out, so + o_li, 4 * static_cast<size_t>(nl));
    }
  } else {
    CSM_HIP(hipStreamSynchronize(st));
  }
  *num_returns = nr;
  *num_misses = nm;
  *num_high = nh;
  *num_low = nl;
  return CSM_OK;
}

}  // extern "C"
