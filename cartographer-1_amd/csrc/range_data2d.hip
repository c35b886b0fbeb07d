// The range-data front end of LocalTrajectoryBuilder2D on gfx950 (reference
// mapping/internal/2d/local_trajectory_builder_2d.cc): what turns one
// accumulated sweep of rangefinder points into the gravity-aligned range data
// the inserters take and the filtered cloud the scan matchers search with.
//
// csm_range_data2d_prepare is one upload, five launches on the context's
// stream and one download:
//   1. range_data2d_classify: every point by its own pose, the range test of
//      AddRangeData (:163-185), the gravity alignment and the z crop of
//      TransformToGravityAlignedFrameAndFilter (:55-58); returns and misses
//      leave it as two packed clouds in input order;
//   2. voxel_filter_batch over both clouds (:61-62);
//   3. range_data2d_compact of both clouds by their keep masks;
//   4. voxel_filter_batch, adaptive, over the filtered returns (:228-231);
//   5. range_data2d_compact of that mask.
// All arithmetic is float and non-contracted (-ffp-contract=off), in Eigen's
// order: Rotate is QuaternionBase::_transformVector, the norm is the 3-vector
// redux x^2 + (y^2 + z^2).
//
// Every compaction is stable and uses no ordering atomics: a workgroup of 16
// waves covers a cloud in tiles of 1024 points, each wave ballots its 64
// points of a tile, one wave scans the 16 x 8 per-wave counts in tile order,
// and a selected point lands at its wave's base plus the number of selected
// lanes below it. Clouds are at most 8192 points (the voxel filter's limit),
// so one workgroup holds a whole cloud.
//
// csm_range_data_transform is sensor::TransformRangeData (range_data.cc): one
// thread per point.

#include <hip/hip_runtime.h>

#include <cstring>

#include "csm_internal.h"
#include "rigid3_dev.h"

namespace csm {
namespace {

constexpr int kRdThreads = 1024;
constexpr int kRdWaves = kRdThreads / 64;
constexpr int kRdTiles = 8;
constexpr int kRdMaxPoints = kRdThreads * kRdTiles;  // 8192, the voxel filters' limit
constexpr int kRdSlots = kRdWaves * kRdTiles;        // per-wave counts of a cloud: 128

// What range_data2d_classify takes by value.
struct RdParams {
  float min_range, max_range, missing_data_ray_length, min_z, max_z;
  RdRigid3 gravity_from_local;
  RdVec3 local_origin;
};

// The packed outputs' header, in front of the three clouds.
struct RdHeader {
  int32_t num_returns, num_misses, num_filtered, pad0;
  float origin[3];
  float pad1;
};

// Bit t of `sel` says whether this thread's point of tile t (point
// t * 1024 + threadIdx.x) is selected. Leaves in cnt[t * 16 + wave] the number
// of selected points before that wave's 64 of tile t, and returns the total.
__device__ int RdOrderedScan(uint32_t sel, int* cnt, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < kRdTiles; ++t) {
    const unsigned long long b = __ballot((sel >> t) & 1u);
    if (lane == 0) cnt[t * kRdWaves + w] = __popcll(b);
  }
  __syncthreads();
  if (w == 0) {
    const int a = cnt[2 * lane], b = cnt[2 * lane + 1];
    int x = a + b;
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    const int ex = x - (a + b);
    cnt[2 * lane] = ex;
    cnt[2 * lane + 1] = ex + a;
    if (lane == 63) *total = x;
  }
  __syncthreads();
  return *total;
}

// The position of this thread's point of tile t among the selected (all
// lanes of the wave call it; the value is meaningful on selected lanes).
__device__ __forceinline__ int RdOrderedPos(uint32_t sel, int t, const int* cnt) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot((sel >> t) & 1u);
  return cnt[t * kRdWaves + w] + __popcll(b & ((1ull << lane) - 1ull));
}

// Stage 1. One workgroup. clouds: the cropped returns at [0, nr), the cropped
// misses at [nr, nr + nm); offsets = {0, nr, nr + nm}.
__global__ void __launch_bounds__(kRdThreads)
range_data2d_classify(const float* __restrict__ poses, const float* __restrict__ hits,
                      const int32_t* __restrict__ origin_index,
                      const float* __restrict__ origins, int n, RdParams p,
                      float* __restrict__ clouds, int64_t* __restrict__ offsets,
                      RdHeader* __restrict__ header) {
  __shared__ int cnt_r[kRdSlots], cnt_m[kRdSlots];
  __shared__ int total_r, total_m;
  float px[kRdTiles], py[kRdTiles], pz[kRdTiles];
  uint32_t is_return = 0, is_miss = 0;
#pragma unroll
  for (int t = 0; t < kRdTiles; ++t) {
    px[t] = py[t] = pz[t] = 0.f;
    const int i = t * kRdThreads + static_cast<int>(threadIdx.x);
    if (i < n) {
      const RdRigid3 pose = RdLoadRigid(poses + 7 * static_cast<size_t>(i));
      const float* op = origins + 3 * static_cast<size_t>(origin_index[i]);
      const RdVec3 o = RdApply(pose, RdVec3{op[0], op[1], op[2]});
      RdVec3 h = RdApply(pose, RdVec3{hits[3 * i], hits[3 * i + 1], hits[3 * i + 2]});
      const RdVec3 delta{h.x - o.x, h.y - o.y, h.z - o.z};
      const float range = sqrtf(delta.x * delta.x + (delta.y * delta.y + delta.z * delta.z));
      if (range >= p.min_range) {  // a NaN range is dropped
        const bool ret = range <= p.max_range;
        if (!ret) {
          const float s = __fdiv_rn(p.missing_data_ray_length, range);
          h = RdVec3{o.x + s * delta.x, o.y + s * delta.y, o.z + s * delta.z};
        }
        const RdVec3 g = RdApply(p.gravity_from_local, h);
        if (p.min_z <= g.z && g.z <= p.max_z) {  // point_cloud.cc:76-81
          px[t] = g.x;
          py[t] = g.y;
          pz[t] = g.z;
          if (ret) is_return |= 1u << t;
          else is_miss |= 1u << t;
        }
      }
    }
  }
  const int nr = RdOrderedScan(is_return, cnt_r, &total_r);
  const int nm = RdOrderedScan(is_miss, cnt_m, &total_m);
#pragma unroll
  for (int t = 0; t < kRdTiles; ++t) {
    const int pr = RdOrderedPos(is_return, t, cnt_r);
    const int pm = RdOrderedPos(is_miss, t, cnt_m);
    const bool r = (is_return >> t) & 1u, m = (is_miss >> t) & 1u;
    if (r || m) {
      float* out = clouds + 3 * static_cast<size_t>(r ? pr : nr + pm);  // nr + nm <= n
      out[0] = px[t];
      out[1] = py[t];
      out[2] = pz[t];
    }
  }
  if (threadIdx.x == 0) {
    offsets[0] = 0;
    offsets[1] = nr;
    offsets[2] = static_cast<int64_t>(nr) + nm;
    const RdVec3 o = RdApply(p.gravity_from_local, p.local_origin);
    header->origin[0] = o.x;
    header->origin[1] = o.y;
    header->origin[2] = o.z;
  }
}

// Stages 3 and 5. Workgroup c keeps the points of cloud c (points
// [offsets[c], offsets[c + 1]) of xyz) whose keep byte is set, in order, at
// out + c * out_stride floats; counts[c] = how many. next_offsets (optional,
// one cloud): {0, counts[0]}, the offsets of the next filter's cloud.
__global__ void __launch_bounds__(kRdThreads)
range_data2d_compact(const float* __restrict__ xyz, const int64_t* __restrict__ offsets,
                     const uint8_t* __restrict__ keep, float* __restrict__ out,
                     int64_t out_stride, int32_t* __restrict__ counts,
                     int64_t* __restrict__ next_offsets) {
  __shared__ int cnt[kRdSlots];
  __shared__ int total;
  const int c = blockIdx.x;
  const int64_t begin = offsets[c];
  const int m = min(static_cast<int>(offsets[c + 1] - begin), kRdMaxPoints);
  uint32_t sel = 0;
#pragma unroll
  for (int t = 0; t < kRdTiles; ++t) {
    const int i = t * kRdThreads + static_cast<int>(threadIdx.x);
    if (i < m && keep[begin + i]) sel |= 1u << t;
  }
  const int kept = RdOrderedScan(sel, cnt, &total);
  float* dst = out + c * out_stride;
#pragma unroll
  for (int t = 0; t < kRdTiles; ++t) {
    const int pos = RdOrderedPos(sel, t, cnt);
    if ((sel >> t) & 1u) {
      const float* src = xyz + 3 * (begin + t * kRdThreads + static_cast<int>(threadIdx.x));
      dst[3 * pos] = src[0];
      dst[3 * pos + 1] = src[1];
      dst[3 * pos + 2] = src[2];
    }
  }
  if (threadIdx.x == 0) {
    counts[c] = kept;
    if (next_offsets && c == 0) {
      next_offsets[0] = 0;
      next_offsets[1] = kept;
    }
  }
}

// sensor::TransformRangeData: point 0 is the origin, then returns, then misses.
__global__ void __launch_bounds__(256)
range_data_transform_points(const float* __restrict__ in, int64_t count, RdRigid3 r,
                            float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= count) return;
  const RdVec3 v = RdApply(r, RdVec3{in[3 * i], in[3 * i + 1], in[3 * i + 2]});
  out[3 * i] = v.x;
  out[3 * i + 1] = v.y;
  out[3 * i + 2] = v.z;
}

size_t Align256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

}  // namespace
}  // namespace csm

extern "C" {

int csm_range_data2d_prepare(csm_context* ctx, const csm_range_data2d_options* options,
                             const float* hits_xyz, const int32_t* origin_index,
                             const float* poses_tq, int32_t n, const float* origins_xyz,
                             int32_t num_origins, const float gravity_from_local_tq[7],
                             const float local_origin_xyz[3], float origin_out[3],
                             float* returns_out, int32_t* num_returns, float* misses_out,
                             int32_t* num_misses, float* filtered_out, int32_t* num_filtered) {
  using namespace csm;
  if (!ctx || !options || n < 0 || num_origins < 0 || !gravity_from_local_tq ||
      !local_origin_xyz || !origin_out || !num_returns || !num_misses || !num_filtered)
    return CSM_EINVAL;
  if (!(options->voxel_filter_size > 0.f) || !(options->adaptive_voxel_filter.max_length > 0.f))
    return CSM_EINVAL;
  if (n > kRdMaxPoints) return CSM_ERANGE;
  if (n > 0) {
    if (!hits_xyz || !origin_index || !poses_tq || !origins_xyz || !returns_out || !misses_out ||
        !filtered_out)
      return CSM_EINVAL;
    for (int32_t i = 0; i < n; ++i)
      if (origin_index[i] < 0 || origin_index[i] >= num_origins) return CSM_EINVAL;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t np = static_cast<size_t>(n), no = static_cast<size_t>(n > 0 ? num_origins : 0);
  // The upload: poses, hits, origin indices, origins.
  const size_t in_poses = 0, in_hits = in_poses + 28 * np, in_index = in_hits + 12 * np,
               in_origins = in_index + 4 * np, in_bytes = in_origins + 12 * no;
  // The working set: both cropped clouds, their offsets, the filtered
  // returns' offsets, the two keep masks.
  const size_t w_clouds = 0, w_offsets = Align256(w_clouds + 12 * np), w_offsets2 = w_offsets + 64,
               w_keep = w_offsets2 + 64, w_keep2 = Align256(w_keep + np),
               w_bytes = w_keep2 + np;
  // The download: header, returns, misses, filtered, n points of room each.
  const size_t out_cloud = sizeof(RdHeader), out_bytes = out_cloud + 3 * 12 * np;
  int rc;
  if ((rc = ctx->rd_in.Reserve(std::max<size_t>(in_bytes, 1)))) return rc;
  if ((rc = ctx->rd_work.Reserve(w_bytes + 256))) return rc;
  if ((rc = ctx->rd_out.Reserve(out_bytes))) return rc;
  if ((rc = ctx->rd_stage_in.Reserve(std::max<size_t>(in_bytes, 1)))) return rc;
  if ((rc = ctx->rd_stage_out.Reserve(out_bytes))) return rc;
  hipStream_t st = ctx->stream;
  char* din = ctx->rd_in.as<char>();
  char* dw = ctx->rd_work.as<char>();
  char* dout = ctx->rd_out.as<char>();
  if (n > 0) {
    char* s = ctx->rd_stage_in.as<char>();
    std::memcpy(s + in_poses, poses_tq, 28 * np);
    std::memcpy(s + in_hits, hits_xyz, 12 * np);
    std::memcpy(s + in_index, origin_index, 4 * np);
    std::memcpy(s + in_origins, origins_xyz, 12 * no);
    CSM_HIP(hipMemcpyAsync(din, s, in_bytes, hipMemcpyHostToDevice, st));
  }
  RdParams p;
  p.min_range = options->min_range;
  p.max_range = options->max_range;
  p.missing_data_ray_length = options->missing_data_ray_length;
  p.min_z = options->min_z;
  p.max_z = options->max_z;
  const float* g = gravity_from_local_tq;
  p.gravity_from_local = RdRigid3{g[0], g[1], g[2], g[3], g[4], g[5], g[6]};
  p.local_origin = RdVec3{local_origin_xyz[0], local_origin_xyz[1], local_origin_xyz[2]};

  float* d_clouds = reinterpret_cast<float*>(dw + w_clouds);
  int64_t* d_offsets = reinterpret_cast<int64_t*>(dw + w_offsets);
  int64_t* d_offsets2 = reinterpret_cast<int64_t*>(dw + w_offsets2);
  uint8_t* d_keep = reinterpret_cast<uint8_t*>(dw + w_keep);
  uint8_t* d_keep2 = reinterpret_cast<uint8_t*>(dw + w_keep2);
  RdHeader* d_header = reinterpret_cast<RdHeader*>(dout);
  float* d_returns = reinterpret_cast<float*>(dout + out_cloud);
  float* d_filtered = d_returns + 6 * np;

  hipLaunchKernelGGL(range_data2d_classify, dim3(1), dim3(kRdThreads), 0, st,
                     reinterpret_cast<const float*>(din + in_poses),
                     reinterpret_cast<const float*>(din + in_hits),
                     reinterpret_cast<const int32_t*>(din + in_index),
                     reinterpret_cast<const float*>(din + in_origins), n, p, d_clouds, d_offsets,
                     d_header);
  CSM_HIP(hipGetLastError());
  if ((rc = csm_voxel_filter_device(ctx, d_clouds, d_offsets, 2, n, options->voxel_filter_size,
                                    d_keep, nullptr)))
    return rc;
  // Returns to the first output cloud, misses to the second.
  hipLaunchKernelGGL(range_data2d_compact, dim3(2), dim3(kRdThreads), 0, st, d_clouds, d_offsets,
                     d_keep, d_returns, static_cast<int64_t>(3 * np), &d_header->num_returns,
                     d_offsets2);
  CSM_HIP(hipGetLastError());
  if ((rc = csm_adaptive_voxel_filter_device(ctx, d_returns, d_offsets2, 1, n,
                                             &options->adaptive_voxel_filter, d_keep2, nullptr)))
    return rc;
  hipLaunchKernelGGL(range_data2d_compact, dim3(1), dim3(kRdThreads), 0, st, d_returns,
                     d_offsets2, d_keep2, d_filtered, static_cast<int64_t>(0),
                     &d_header->num_filtered, static_cast<int64_t*>(nullptr));
  CSM_HIP(hipGetLastError());
  char* so = ctx->rd_stage_out.as<char>();
  CSM_HIP(hipMemcpyAsync(so, dout, out_bytes, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  RdHeader h;
  std::memcpy(&h, so, sizeof(h));
  if (h.num_returns < 0 || h.num_returns > n || h.num_misses < 0 || h.num_misses > n ||
      h.num_filtered < 0 || h.num_filtered > h.num_returns)
    return CSM_EHIP;
  *num_returns = h.num_returns;
  *num_misses = h.num_misses;
  *num_filtered = h.num_filtered;
  std::memcpy(origin_out, h.origin, sizeof(h.origin));
  const char* clouds = so + out_cloud;
  if (h.num_returns) std::memcpy(returns_out, clouds, 12 * static_cast<size_t>(h.num_returns));
  if (h.num_misses)
    std::memcpy(misses_out, clouds + 12 * np, 12 * static_cast<size_t>(h.num_misses));
  if (h.num_filtered)
    std::memcpy(filtered_out, clouds + 24 * np, 12 * static_cast<size_t>(h.num_filtered));
  return CSM_OK;
}

int csm_range_data_transform(csm_context* ctx, const float transform_tq[7],
                             const float origin_xyz[3], const float* returns_xyz,
                             int32_t num_returns, const float* misses_xyz, int32_t num_misses,
                             float origin_out[3], float* returns_out, float* misses_out) {
  using namespace csm;
  if (!ctx || !transform_tq || !origin_xyz || !origin_out || num_returns < 0 || num_misses < 0)
    return CSM_EINVAL;
  if (num_returns > 0 && (!returns_xyz || !returns_out)) return CSM_EINVAL;
  if (num_misses > 0 && (!misses_xyz || !misses_out)) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t nr = static_cast<size_t>(num_returns), nm = static_cast<size_t>(num_misses);
  const size_t count = 1 + nr + nm, bytes = 12 * count;
  int rc;
  if ((rc = ctx->rd_in.Reserve(bytes))) return rc;
  if ((rc = ctx->rd_out.Reserve(bytes))) return rc;
  if ((rc = ctx->rd_stage_in.Reserve(bytes))) return rc;
  if ((rc = ctx->rd_stage_out.Reserve(bytes))) return rc;
  char* s = ctx->rd_stage_in.as<char>();
  std::memcpy(s, origin_xyz, 12);
  if (nr) std::memcpy(s + 12, returns_xyz, 12 * nr);
  if (nm) std::memcpy(s + 12 + 12 * nr, misses_xyz, 12 * nm);
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(ctx->rd_in.ptr, s, bytes, hipMemcpyHostToDevice, st));
  const float* t = transform_tq;
  const unsigned blocks = static_cast<unsigned>((count + 255) / 256);
  hipLaunchKernelGGL(range_data_transform_points, dim3(blocks), dim3(256), 0, st,
                     ctx->rd_in.as<float>(), static_cast<int64_t>(count),
                     RdRigid3{t[0], t[1], t[2], t[3], t[4], t[5], t[6]}, ctx->rd_out.as<float>());
  CSM_HIP(hipGetLastError());
  char* so = ctx->rd_stage_out.as<char>();
  CSM_HIP(hipMemcpyAsync(so, ctx->rd_out.ptr, bytes, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  std::memcpy(origin_out, so, 12);
  if (nr) std::memcpy(returns_out, so + 12, 12 * nr);
  if (nm) std::memcpy(misses_out, so + 12 + 12 * nr, 12 * nm);
  return CSM_OK;
}

}  // extern "C"
