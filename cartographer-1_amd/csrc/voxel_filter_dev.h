// Device helpers shared by the two voxel filters (voxel_filter.hip: one cloud
// per workgroup in LDS; voxel_filter_large.hip: one cloud over the device):
// the voxel key of GetVoxelCellIndex (sensor/internal/voxel_filter.cc:79-86),
// std::minstd_rand0 with a jump to any stream position, libstdc++'s
// uniform_int_distribution draw, and the float arithmetic of
// AdaptivelyVoxelFiltered's edge-length search (:38-76).
#ifndef CSM_VOXEL_FILTER_DEV_H_
#define CSM_VOXEL_FILTER_DEV_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace csm {

constexpr uint32_t kMinstdM = 2147483647u;  // std::minstd_rand0: x <- 16807 x mod (2^31 - 1)
constexpr uint32_t kMinstdA = 16807u;
// uniform_int_distribution's __urngrange = max() - min() for minstd_rand0.
constexpr uint32_t kUrngRange = 2147483645u;

__device__ __forceinline__ uint32_t MulMod(uint32_t a, uint32_t b) {
  const uint64_t p = static_cast<uint64_t>(a) * b;  // < 2^62
  uint64_t r = (p & kMinstdM) + (p >> 31);          // < 2^32
  r = (r & kMinstdM) + (r >> 31);                   // <= 2^31
  return static_cast<uint32_t>(r >= kMinstdM ? r - kMinstdM : r);
}

// State of a seed-1 minstd_rand0 after e draws.
__device__ inline uint32_t MinstdJump(uint32_t e) {
  uint32_t result = 1u, base = kMinstdA;
  while (e) {
    if (e & 1u) result = MulMod(result, base);
    base = MulMod(base, base);
    e >>= 1;
  }
  return result;
}

// One uniform_int_distribution<>(1, k) draw from output x (no rejection):
// returns 1 when the draw equals k, 0 otherwise, 2 when x is rejected.
__device__ __forceinline__ int Draw(uint32_t x, uint32_t k) {
  const uint32_t scaling = kUrngRange / k;
  const uint32_t past = k * scaling;
  const uint32_t ret = x - 1u;  // __urng() - __urngmin
  if (ret >= past) return 2;
  return (ret / scaling + 1u == k) ? 1 : 0;
}

// GetVoxelCellIndex (voxel_filter.cc:79-86).
__device__ __forceinline__ uint64_t VoxelKeyCoord(float v, float resolution) {
  const float q = __fdiv_rn(v, resolution);
  // common::RoundToInt = std::lround narrowed to int, then widened to uint64_t.
  const int i = static_cast<int>(static_cast<long long>(roundf(q)));
  return static_cast<uint64_t>(static_cast<int64_t>(i));
}
__device__ __forceinline__ uint64_t VoxelKey(float x, float y, float z, float resolution) {
  return (VoxelKeyCoord(x, resolution) << 42) + (VoxelKeyCoord(y, resolution) << 21) +
         VoxelKeyCoord(z, resolution);
}

// FilterByMaxRange (:31-36): ||p|| <= max_range, Eigen's x0 + (x1 + x2) order.
__host__ __device__ __forceinline__ bool VfWithinRange(float x, float y, float z, float max_range) {
  return sqrtf(x * x + (y * y + z * z)) <= max_range;  // -ffp-contract=off
}

// Correctly rounded float division on either side.
__host__ __device__ __forceinline__ float VfDiv(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// AdaptivelyVoxelFiltered (:38-76) as a machine: which edge length to filter
// with next, given the count the last filter kept. The caller runs VoxelFilter
// at Length() while !Done(), reports the count with Step(), and copies the
// mask of that pass to its result when Step() returns true. Division by two
// and the additions are exact or correctly rounded on both sides, so host and
// device walk the same lengths.
struct VfLengthSearch {
  float max_length, min_num_points;
  float high_length, low_length;
  int phase = 0;  // 0: max_length, 1: halving, 2: bisecting, 3: done
  __host__ __device__ VfLengthSearch(float max_len, float min_points)
      : max_length(max_len), min_num_points(min_points), high_length(max_len), low_length(max_len) {}
  __host__ __device__ bool Done() const { return phase == 3; }
  __host__ __device__ float Length() const {
    return phase == 0 ? max_length : phase == 1 ? low_length : VfDiv(low_length + high_length, 2.f);
  }
  __host__ __device__ bool Bisecting() const {
    return VfDiv(high_length - low_length, low_length) > 1e-1f;
  }
  // Takes the count kept at Length(); true when that pass's mask is the result so far.
  __host__ __device__ bool Step(int kept) {
    const bool enough = static_cast<float>(kept) >= min_num_points;
    if (phase == 0) {
      if (enough || !(high_length > 1e-2f * max_length)) {
        phase = 3;
      } else {
        phase = 1;
        low_length = VfDiv(high_length, 2.f);
      }
      return true;
    }
    if (phase == 1) {
      if (enough) {
        phase = Bisecting() ? 2 : 3;
      } else {
        high_length = VfDiv(high_length, 2.f);
        if (high_length > 1e-2f * max_length) low_length = VfDiv(high_length, 2.f);
        else phase = 3;
      }
      return true;
    }
    const float mid_length = VfDiv(low_length + high_length, 2.f);
    if (enough) low_length = mid_length;
    else high_length = mid_length;
    if (!Bisecting()) phase = 3;
    return enough;
  }
};

}  // namespace csm

#endif  // CSM_VOXEL_FILTER_DEV_H_
