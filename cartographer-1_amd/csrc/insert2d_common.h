// Shared by the two 2D range-data inserters (insert2d.hip: ProbabilityGrid,
// insert_tsdf2d.hip: TSDF2D): the closed-form column walk of RayToPixelMask
// (ray_to_pixel_mask.cc:29-159), Grid2D::GrowLimits on the limits alone
// (grid_2d.cc:142-175), and the rect-copy and bounding-box kernels of growth
// and Finish. Everything here has internal linkage: each translation unit
// that includes this header compiles its own copy of the kernels.
//
// ColumnRun. The reference walks a ray one pixel column at a time carrying
// sub_y, the height at the column's right border in units of 1 / denominator
// of a pixel, reduced by `denominator` per row stepped. Unreduced, the height
// after column k is Y_k = (2 (b.y % s) + 1) dx + dy first_pixel + k dy 2 s (and
// Y_K = Y_{K-1} + dy last_pixel at the end point), all in 64-bit integers. For
// dy > 0 the walk emits, in column k, the rows from its entry row up to the
// row that holds Y_k, where a height exactly on a row border belongs to the
// row below: ceil(Y_k / denominator) - 1. The next column is entered at
// floor(Y_k / denominator): one row higher exactly when Y_k is a multiple of
// the denominator, which is the corner rule (the walk steps diagonally and
// emits neither side cell). dy <= 0 mirrors it (floor for the run's end,
// ceil - 1 for the next entry). So each column's run is a closed form of k.
#ifndef CSM_INSERT2D_COMMON_H_
#define CSM_INSERT2D_COMMON_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>

#include "csm_internal.h"

namespace csm {

// Ids of device-resident 2D grids of either kind: process-unique, never 0.
inline std::atomic<uint64_t> g_next_grid_id{1};

namespace {

constexpr int kSubpixelScale = 1000;  // probability_grid_range_data_inserter_2d.cc:33
constexpr int kMaxSide = 8192;

__host__ __device__ inline int64_t FloorDiv(int64_t a, int64_t d) {  // d > 0
  const int64_t q = a / d;
  return (a % d != 0 && a < 0) ? q - 1 : q;
}
__host__ __device__ inline int64_t CeilDiv(int64_t a, int64_t d) {  // d > 0
  const int64_t q = a / d;
  return (a % d != 0 && a > 0) ? q + 1 : q;
}

// One ray's walk, begin.x <= end.x (ray_to_pixel_mask.cc:29-78 setup).
struct RayWalk {
  int col0, row0;  // begin pixel
  int K;           // end column - begin column
  int ylo, yhi;    // K == 0: the rows of the single column (:45-57)
  int64_t dy, denom, y0, step, last;
};

__host__ __device__ inline RayWalk MakeRayWalk(int bx, int by, int ex, int ey, int s) {
  if (bx > ex) {
    int t = bx; bx = ex; ex = t;
    t = by; by = ey; ey = t;
  }
  RayWalk w;
  w.col0 = bx / s;
  w.row0 = by / s;
  w.K = ex / s - w.col0;
  w.ylo = (by < ey ? by : ey) / s;
  w.yhi = (by < ey ? ey : by) / s;
  const int64_t dx = static_cast<int64_t>(ex) - bx;
  w.dy = static_cast<int64_t>(ey) - by;
  w.denom = 2 * static_cast<int64_t>(s) * dx;
  const int64_t first_pixel = 2 * s - 2 * (bx % s) - 1;
  const int64_t last_pixel = 2 * (ex % s) + 1;
  w.y0 = (2 * static_cast<int64_t>(by % s) + 1) * dx + w.dy * first_pixel;
  w.step = w.dy * 2 * s;
  w.last = w.dy * last_pixel;
  return w;
}

// The rows [lo, hi] the ray covers in column col0 + k, 0 <= k <= K.
__host__ __device__ inline void ColumnRun(const RayWalk& w, int k, int* lo, int* hi) {
  if (w.K == 0) {
    *lo = w.ylo;
    *hi = w.yhi;
    return;
  }
  const int64_t yprev = w.y0 + static_cast<int64_t>(k - 1) * w.step;  // used for k >= 1
  const int64_t yk = k < w.K ? w.y0 + static_cast<int64_t>(k) * w.step
                             : w.y0 + static_cast<int64_t>(w.K - 1) * w.step + w.last;
  int64_t a, b;
  if (w.dy > 0) {
    a = k == 0 ? 0 : FloorDiv(yprev, w.denom);
    b = CeilDiv(yk, w.denom) - 1;
  } else {
    b = k == 0 ? 0 : CeilDiv(yprev, w.denom) - 1;
    a = FloorDiv(yk, w.denom);
  }
  *lo = w.row0 + static_cast<int>(a);
  *hi = w.row0 + static_cast<int>(b);
}

// dst[(dy + y) * dnx + dx + x] = src[(sy + y) * snx + sx + x], w x h cells.
__global__ void __launch_bounds__(256)
insert2d_copy_rect(const uint16_t* __restrict__ src, int snx, int sx, int sy,
                   uint16_t* __restrict__ dst, int dnx, int dx, int dy, int w, int h) {
  const int64_t total = static_cast<int64_t>(w) * h;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int y = static_cast<int>(i / w), x = static_cast<int>(i % w);
    dst[static_cast<size_t>(dy + y) * dnx + dx + x] =
        src[static_cast<size_t>(sy + y) * snx + sx + x] & 0x7fff;
  }
}

// box: min x, min y, max x, max y of the nonzero cells (INT_MAX / -1 start).
__global__ void __launch_bounds__(256)
insert2d_box(const uint16_t* __restrict__ cells, int nx, int ny, int* __restrict__ box) {
  int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  const int64_t total = static_cast<int64_t>(nx) * ny;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    if (cells[i] == 0) continue;
    const int y = static_cast<int>(i / nx), x = static_cast<int>(i % nx);
    x0 = min(x0, x);
    y0 = min(y0, y);
    x1 = max(x1, x);
    y1 = max(y1, y);
  }
  for (int o = 32; o > 0; o >>= 1) {
    x0 = min(x0, __shfl_xor(x0, o));
    y0 = min(y0, __shfl_xor(y0, o));
    x1 = max(x1, __shfl_xor(x1, o));
    y1 = max(y1, __shfl_xor(y1, o));
  }
  if ((threadIdx.x & 63) == 0 && x1 >= 0) {
    atomicMin(box + 0, x0);
    atomicMin(box + 1, y0);
    atomicMax(box + 2, x1);
    atomicMax(box + 3, y1);
  }
}

// ---------------------------------------------------------------- host -----

inline int EnsureDevice(csm_context* ctx) {
  return hipSetDevice(ctx->device) == hipSuccess ? CSM_OK : CSM_EHIP;
}

// DevBuf owns its pointer and has no move: hand it over by hand (`to` empty).
inline void MoveBuf(DevBuf* from, DevBuf* to) {
  to->ptr = from->ptr;
  to->bytes = from->bytes;
  from->ptr = nullptr;
  from->bytes = 0;
}

// MapLimits::GetCellIndex / Contains (map_limits.h:69-89).
inline void CellIndex(const csm_map_limits& l, double resolution, float px, float py, long* x,
                      long* y) {
  *x = std::lround((l.max_y - py) / resolution - 0.5);
  *y = std::lround((l.max_x - px) / resolution - 0.5);
}
inline bool Contains(const csm_map_limits& l, float px, float py) {
  long x, y;
  CellIndex(l, l.resolution, px, py, &x, &y);
  return x >= 0 && y >= 0 && x < l.num_x_cells && y < l.num_y_cells;
}

// Grid2D::GrowLimits (grid_2d.cc:142-175) on the limits alone: doubles about
// the centre until the point fits, adding each doubling's offset of the old
// cells. False past kMaxSide.
inline bool GrowLimits(csm_map_limits* l, float px, float py, int* off_x, int* off_y) {
  while (!Contains(*l, px, py)) {
    if (l->num_x_cells * 2 > kMaxSide || l->num_y_cells * 2 > kMaxSide) return false;
    const int xo = l->num_x_cells / 2, yo = l->num_y_cells / 2;
    l->max_x = l->max_x + l->resolution * yo;
    l->max_y = l->max_y + l->resolution * xo;
    l->num_x_cells *= 2;
    l->num_y_cells *= 2;
    *off_x += xo;
    *off_y += yo;
  }
  return true;
}

inline bool Finite3(const float* p) {
  return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
}

inline unsigned Blocks(int64_t items, int per_block, int cap) {
  const int64_t b = (items + per_block - 1) / per_block;
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(b, cap)));
}

}  // namespace
}  // namespace csm

#endif  // CSM_INSERT2D_COMMON_H_
