// Shared by the two CeresScanMatcher2D refinement kernels (ceres2d.hip: the
// probability grid's bicubic occupied-space cost; ceres2d_tsdf.hip: the TSDF
// match cost): the item descriptor, the solver options, the workgroup
// reductions and the 3x3 solve of the Levenberg-Marquardt loop.
#ifndef CSM_CERES2D_COMMON_H_
#define CSM_CERES2D_COMMON_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace csm {

constexpr int kRefineThreads = 256;

// One (grid, cloud) item. The grid's values come either as the float planes of
// a csm_fast2d handle (cost, and weight for a TSDF) or as the uint16 cells of
// a device-resident grid with their value tables (cells16 != nullptr; the
// update marker is masked off).
struct RefineDesc {
  const float* cost;  // num_y_cells x num_x_cells correspondence costs (a TSDF: TSD values)
  double max_x, max_y, resolution;
  int32_t nx, ny;
  double max_cost;  // a TSDF: the truncation distance
  int64_t point_offset;
  int32_t n;
  double initial[3], target[2];
  const float* weight;       // a TSDF handle's weights
  const uint16_t* cells16;   // device grid: correspondence-cost (TSD) cells
  const float* table;        // ... and their value -> cost table (unknown -> max cost)
  const uint16_t* weight16;  // device TSDF: weight cells
  const float* wtable;       // ... and ValueToWeight (unknown -> 0)
};

struct RefineOpts {
  double occupied, wt, wr;
  int max_iterations;
  int nonmonotonic;  // ceres_solver_options.use_nonmonotonic_steps
};

__device__ __forceinline__ double WaveSumD(double v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Sums k doubles per thread over the workgroup; every thread gets the totals.
template <int K>
__device__ void BlockSum(double* v, double (*red)[K]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double t = WaveSumD(v[k]);
    if (lane == 0) red[w][k] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = 0.;
    for (int q = 0; q < kRefineThreads / 64; ++q) t += red[q][k];
    v[k] = t;
  }
  __syncthreads();
}

__device__ inline bool Solve3(double M[3][4], double out[3]) {
  for (int c = 0; c < 3; ++c) {
    int piv = c;
    for (int i = c + 1; i < 3; ++i)
      if (fabs(M[i][c]) > fabs(M[piv][c])) piv = i;
    if (M[piv][c] == 0.) return false;
    for (int j = 0; j < 4; ++j) {
      const double t = M[c][j];
      M[c][j] = M[piv][j];
      M[piv][j] = t;
    }
    for (int i = c + 1; i < 3; ++i) {
      const double f = M[i][c] / M[c][c];
      for (int j = c; j < 4; ++j) M[i][j] -= f * M[c][j];
    }
  }
  for (int i = 2; i >= 0; --i) {
    double v = M[i][3];
    for (int j = i + 1; j < 3; ++j) v -= M[i][j] * out[j];
    out[i] = v / M[i][i];
  }
  return true;
}

// ceres2d_tsdf.hip: the TSDF refinement over `count` items. Workgroup b takes
// items[order[b]] (order == nullptr: items[b]) and writes its pose and
// iteration count at that item's index. u16: the items read a device grid's
// uint16 planes (cells16, weight16) instead of a handle's float planes.
hipError_t LaunchCeres2dTsdfRefine(const RefineDesc* items, const int32_t* order, int count,
                                   bool u16, const float* points, const RefineOpts& o,
                                   double* out_pose, int32_t* out_iters, hipStream_t st);

}  // namespace csm

#endif  // CSM_CERES2D_COMMON_H_
