// Shared by the two 2D range-data inserters (insert2d.hip: ProbabilityGrid,
// insert_tsdf2d.hip: TSDF2D): the closed-form column walk of RayToPixelMask
// (ray_to_pixel_mask.cc:29-159), Grid2D::GrowLimits on the limits alone
// (grid_2d.cc:142-175), the rect-copy and bounding-box kernels of growth and
// Finish, and the host steps of growth, create and crop written once over a
// grid's list of planes (Plane2). Everything here has internal linkage: each
// translation unit that includes this header compiles its own copy of the
// kernels.
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
#include "insert_host.h"

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

// ---- growth and crop, the same steps for both inserters -------------------

// One plane of a 2D grid as growth sees it.
template <typename Grid>
struct Plane2 {
  DevBuf Grid::*buf;
  size_t (*bytes)(size_t nx, size_t ny);
  int fill;    // memset byte of a new plane
  bool cells;  // uint16 cells, x fastest: the old ones are copied in at their offset
};

constexpr int kMaxPlanes = 3;

// One scan's growth of its grid, planned on the host's copy of the limits.
struct GrowPlan2 {
  int grid = 0, round = 0;
  bool grew = false;
  int off_x = 0, off_y = 0;
  csm_map_limits before{}, after{};
  DevBuf grown[kMaxPlanes];  // the grown grid's planes
  void* seen[kMaxPlanes] = {};  // the planes the scan's kernels run on (TakeGrown2)
};

// GrowAsNeeded for the float box (min x, min y, max x, max y) of what the
// scan touches, padded by 1e-6f, and the scan's round within its grid. False
// past kMaxSide.
inline bool PlanGrowth2(int grid, const float* box, std::vector<csm_map_limits>* limits,
                        std::vector<int>* rounds, GrowPlan2* p) {
  constexpr float kPadding = 1e-6f;
  p->grid = grid;
  p->round = (*rounds)[grid]++;
  csm_map_limits& l = (*limits)[grid];
  p->before = l;
  if (!GrowLimits(&l, box[0] - kPadding, box[1] - kPadding, &p->off_x, &p->off_y) ||
      !GrowLimits(&l, box[2] + kPadding, box[3] + kPadding, &p->off_x, &p->off_y))
    return false;
  p->after = l;
  p->grew = l.num_x_cells != p->before.num_x_cells;
  return true;
}

inline void GiveBackGrown2(csm_context* ctx, std::vector<GrowPlan2>* plan) {
  for (GrowPlan2& p : *plan)
    for (DevBuf& b : p.grown) ctx->pool.Give(&b);
}

// Every grown grid's planes, before anything is enqueued, and the planes each
// scan will see: its own grown ones, else those the latest earlier scan of its
// grid grew, else the grid's.
template <typename Grid, size_t N>
int TakeGrown2(csm_context* ctx, Grid* const* grids, int32_t num_grids,
               const Plane2<Grid> (&planes)[N], std::vector<GrowPlan2>* plan) {
  std::vector<void*> cur(static_cast<size_t>(num_grids) * N);
  for (int g = 0; g < num_grids; ++g)
    for (size_t k = 0; k < N; ++k) cur[g * N + k] = (grids[g]->*planes[k].buf).ptr;
  for (GrowPlan2& p : *plan)
    for (size_t k = 0; k < N; ++k) {
      const size_t bytes = planes[k].bytes(p.after.num_x_cells, p.after.num_y_cells);
      if (int rc = p.grew ? ctx->pool.Take(bytes, &p.grown[k]) : CSM_OK) return rc;
      if (p.grew) cur[p.grid * N + k] = p.grown[k].ptr;
      p.seen[k] = cur[p.grid * N + k];
    }
  return CSM_OK;
}

// Enqueues a scan's growth (new planes filled, old cells copied to their
// offset), swaps the grown planes in and moves the grid's host state on.
template <typename Grid, size_t N>
int CommitScan2(csm_context* ctx, Grid* g, const Plane2<Grid> (&planes)[N], GrowPlan2* p,
                std::deque<DevBuf>* retired) {
  hipStream_t st = ctx->stream;
  const size_t nx = p->after.num_x_cells, ny = p->after.num_y_cells;
  const int ow = p->before.num_x_cells, oh = p->before.num_y_cells;
  for (size_t k = 0; p->grew && k < N; ++k)
    CSM_HIP(hipMemsetAsync(p->grown[k].ptr, planes[k].fill, planes[k].bytes(nx, ny), st));
  for (size_t k = 0; p->grew && k < N; ++k) {
    if (!planes[k].cells) continue;
    hipLaunchKernelGGL(insert2d_copy_rect, dim3(Blocks(int64_t{ow} * oh, 256, 4096)), dim3(256), 0,
                       st, (g->*planes[k].buf).template as<uint16_t>(), ow, 0, 0,
                       p->grown[k].as<uint16_t>(), static_cast<int>(nx), p->off_x, p->off_y, ow,
                       oh);
    CSM_HIP(hipGetLastError());
  }
  for (size_t k = 0; p->grew && k < N; ++k) {
    retired->push_back(std::move(g->*planes[k].buf));
    g->*planes[k].buf = std::move(p->grown[k]);
  }
  g->limits = p->after;
  ++g->generation;
  return CSM_OK;
}

template <typename Grid, size_t N>
void GivePlanes2(Grid* g, const Plane2<Grid> (&planes)[N]) {
  for (size_t k = 0; k < N; ++k) g->ctx->pool.Give(&(g->*planes[k].buf));
}

// A new grid's planes, taken from the pool: plane k copied from host[k] (the
// caller's memory is read, so the copy is waited for), else filled.
template <typename Grid, size_t N>
int NewPlanes2(Grid* g, const Plane2<Grid> (&planes)[N], const uint16_t* const (&host)[N]) {
  const size_t nx = g->limits.num_x_cells, ny = g->limits.num_y_cells;
  hipStream_t st = g->ctx->stream;
  for (size_t k = 0; k < N; ++k)
    if (int rc = g->ctx->pool.Take(planes[k].bytes(nx, ny), &(g->*planes[k].buf))) {
      GivePlanes2(g, planes);
      return rc;
    }
  bool wait = false;
  for (size_t k = 0; k < N; ++k) {
    void* p = (g->*planes[k].buf).ptr;
    if (host[k]) {
      CSM_HIP(hipMemcpyAsync(p, host[k], planes[k].bytes(nx, ny), hipMemcpyHostToDevice, st));
      wait = true;
    } else {
      CSM_HIP(hipMemsetAsync(p, planes[k].fill, planes[k].bytes(nx, ny), st));
    }
  }
  if (wait) CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

// Grid2D::ComputeCroppedLimits (grid_2d.cc:121-132) for Finish: the box of the
// nonzero cells of `cells`, 1 x 1 at the origin when there is none. Waits for
// the device.
struct Crop2 {
  bool empty;
  int ox, oy, nx, ny;
};
inline int CropBox2(csm_context* ctx, const uint16_t* cells, int nx, int ny, Crop2* c) {
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = ctx->ins_box.Reserve(4 * sizeof(int))) ||
      (rc = ctx->ins_box_host.Reserve(4 * sizeof(int))))
    return rc;
  int* hb = ctx->ins_box_host.as<int>();
  hb[0] = hb[1] = INT_MAX;
  hb[2] = hb[3] = -1;
  CSM_HIP(hipMemcpyAsync(ctx->ins_box.ptr, hb, 4 * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(insert2d_box, dim3(Blocks(int64_t{nx} * ny, 1024, 1024)), dim3(256), 0, st,
                     cells, nx, ny, ctx->ins_box.as<int>());
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(hb, ctx->ins_box.ptr, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  c->empty = hb[2] < 0;
  c->ox = c->empty ? 0 : hb[0];
  c->oy = c->empty ? 0 : hb[1];
  c->nx = c->empty ? 1 : hb[2] - hb[0] + 1;
  c->ny = c->empty ? 1 : hb[3] - hb[1] + 1;
  return CSM_OK;
}

// The cropped grid's limits and the handle's host state after Finish
// (probability_grid.cc:95-99, tsdf_2d.cc:122-124).
template <typename Grid>
void FinishCrop2(Grid* g, const Crop2& c) {
  g->limits.max_x = g->limits.max_x - g->limits.resolution * static_cast<double>(c.oy);
  g->limits.max_y = g->limits.max_y - g->limits.resolution * static_cast<double>(c.ox);
  g->limits.num_x_cells = c.nx;
  g->limits.num_y_cells = c.ny;
  g->finished = true;
  ++g->generation;
}

// What csm_*_grid_create asks of the limits.
inline int CheckLimits2(const csm_map_limits* limits) {
  if (limits->num_x_cells < 1 || limits->num_y_cells < 1 || !(limits->resolution > 0.) ||
      !std::isfinite(limits->resolution) || !std::isfinite(limits->max_x) ||
      !std::isfinite(limits->max_y))
    return CSM_EINVAL;
  return limits->num_x_cells > kMaxSide || limits->num_y_cells > kMaxSide ? CSM_ERANGE : CSM_OK;
}

}  // namespace
}  // namespace csm

#endif  // CSM_INSERT2D_COMMON_H_
