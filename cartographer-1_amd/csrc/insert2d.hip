// Device-resident ProbabilityGrid and ProbabilityGridRangeDataInserter2D on
// gfx950 (probability_grid_range_data_inserter_2d.cc:35-136,
// ray_to_pixel_mask.cc:29-159, grid_2d.cc:121-175, probability_grid.cc:51-106,
// probability_values.cc:89-106).
//
// Why the result does not depend on thread order. Within one Insert the
// update marker admits one table lookup per cell (probability_grid.cc:51-63)
// and every hit is applied before any miss (:60-96 of the inserter), so a
// cell ends as hit_table[old] if a return lands in it, else miss_table[old] if
// a ray's pixel mask holds it, else old. The device therefore only has to
// find two SETS of cells. It marks them in a per-grid plane of 2 bits per cell
// (bit 1: hit, bit 0: miss; 16 cells per 32-bit word, atomicOr, which
// commutes), and an apply pass over the scan's bounding box reads each word
// once, writes table[old] for its marked cells and stores zero back: every
// cell is written by exactly one thread, and the plane is all zero again when
// the call ends.
//
// Kernels.
//   insert2d_mark   one launch per round of a batch; blockIdx.y is the scan.
//                   A wave takes one ray (origin -> return or miss): every
//                   lane computes the fine (x1000) indices with
//                   MapLimits::GetCellIndex in double, lane 0 marks the hit,
//                   and lane k marks the run of rows the ray covers in pixel
//                   column k, k + 64, ... (ColumnRun below). Without free
//                   space only the hits are marked, one thread per return.
//   insert2d_apply  one thread per mark word of each scan's bounding box.
//   insert2d_copy_rect  GrowLimits' copy into the doubled grid (several
//                   doublings folded into one offset) and Finish's crop.
//   insert2d_box    bounding box of the nonzero cells (Finish).
//   ray_mask_count / ray_mask_write  csm_ray_to_pixel_mask, test-visible: the
//                   same ColumnRun, one thread per ray, cells in the
//                   reference's order.
// The column walk (RayWalk, ColumnRun), the growth of the limits and the
// copy_rect / box kernels are shared with the TSDF inserter:
// insert2d_common.h.
//
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "csm_internal.h"
#include "insert2d_common.h"

namespace csm {
namespace {

constexpr int kMaxCoord = 1 << 30;  // csm_ray_to_pixel_mask's coordinate limit

__host__ __device__ inline int MarkWords(int nx) { return (nx + 15) >> 4; }

// One scan of a batch, as the kernels see it.
struct ScanDev {
  uint16_t* cells;
  uint32_t* marks;
  int nx, ny;
  double max_x, max_y, fine_resolution;
  float ox, oy;
  int num_returns, num_misses;
  int64_t ret_begin, miss_begin;       // first point in the returns / misses arrays
  int box_x0, box_y0, box_x1, box_y1;  // cells the scan can touch, inclusive
};

// MapLimits::GetCellIndex (map_limits.h:69-75) on the x1000 limits; false
// when the index is outside them (the reference would CHECK-fail).
__device__ inline bool FineIndex(const ScanDev& d, float px, float py, int* fx, int* fy) {
  const long long x = llround((d.max_y - static_cast<double>(py)) / d.fine_resolution - 0.5);
  const long long y = llround((d.max_x - static_cast<double>(px)) / d.fine_resolution - 0.5);
  if (x < 0 || y < 0 || x >= static_cast<long long>(d.nx) * kSubpixelScale ||
      y >= static_cast<long long>(d.ny) * kSubpixelScale)
    return false;
  *fx = static_cast<int>(x);
  *fy = static_cast<int>(y);
  return true;
}

__device__ inline void Mark(const ScanDev& d, int x, int y, uint32_t bit) {
  if (static_cast<unsigned>(x) >= static_cast<unsigned>(d.nx) ||
      static_cast<unsigned>(y) >= static_cast<unsigned>(d.ny))
    return;
  uint32_t* w = d.marks + static_cast<size_t>(y) * MarkWords(d.nx) + (x >> 4);
  const uint32_t m = bit << ((x & 15) * 2);
  // Bits only rise during a mark pass: a stale zero costs one redundant
  // atomic, never a lost mark. Every ray of a scan starts in the origin's
  // cell; this keeps them off its word.
  if ((__atomic_load_n(w, __ATOMIC_RELAXED) & m) == m) return;
  atomicOr(w, m);
}

__global__ void __launch_bounds__(256)
insert2d_mark(const ScanDev* __restrict__ scans, const float* __restrict__ returns_xyz,
              const float* __restrict__ misses_xyz, int free_space) {
  const ScanDev d = scans[blockIdx.y];
  if (!free_space) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.num_returns;
         i += gridDim.x * blockDim.x) {
      const float* p = returns_xyz + 3 * (d.ret_begin + i);
      int ex, ey;
      if (FineIndex(d, p[0], p[1], &ex, &ey)) Mark(d, ex / kSubpixelScale, ey / kSubpixelScale, 2u);
    }
    return;
  }
  int bx, by;
  if (!FineIndex(d, d.ox, d.oy, &bx, &by)) return;
  const int lane = threadIdx.x & 63;
  const int waves = blockDim.x >> 6;
  const int nrays = d.num_returns + d.num_misses;
  for (int ray = blockIdx.x * waves + (threadIdx.x >> 6); ray < nrays; ray += gridDim.x * waves) {
    const bool is_return = ray < d.num_returns;
    const float* p = is_return ? returns_xyz + 3 * (d.ret_begin + ray)
                               : misses_xyz + 3 * (d.miss_begin + (ray - d.num_returns));
    int ex, ey;
    if (!FineIndex(d, p[0], p[1], &ex, &ey)) continue;  // wave-uniform
    if (is_return && lane == 0) Mark(d, ex / kSubpixelScale, ey / kSubpixelScale, 2u);
    const RayWalk w = MakeRayWalk(bx, by, ex, ey, kSubpixelScale);
    if (w.K == 0) {  // one column: lanes across its rows
      for (int y = w.ylo + lane; y <= w.yhi; y += 64) Mark(d, w.col0, y, 1u);
      continue;
    }
    for (int k = lane; k <= w.K; k += 64) {
      int lo, hi;
      ColumnRun(w, k, &lo, &hi);
      for (int y = lo; y <= hi; ++y) Mark(d, w.col0 + k, y, 1u);
    }
  }
}

// tabs: hit table then miss table, 32768 entries each, update marker removed.
__global__ void __launch_bounds__(256)
insert2d_apply(const ScanDev* __restrict__ scans, const uint16_t* __restrict__ tabs) {
  const ScanDev d = scans[blockIdx.y];
  if (d.box_x1 < d.box_x0 || d.box_y1 < d.box_y0) return;
  const int wx0 = d.box_x0 >> 4;
  const int nw = (d.box_x1 >> 4) - wx0 + 1;
  const int total = nw * (d.box_y1 - d.box_y0 + 1);
  const int mw = MarkWords(d.nx);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = d.box_y0 + i / nw;
    const int wx = wx0 + i % nw;
    uint32_t* mp = d.marks + static_cast<size_t>(y) * mw + wx;
    uint32_t m = *mp;
    if (m == 0) continue;
    *mp = 0;
    uint16_t* row = d.cells + static_cast<size_t>(y) * d.nx + wx * 16;
    const int n = min(16, d.nx - wx * 16);
    for (int c = 0; c < n; ++c, m >>= 2) {
      const uint32_t b = m & 3u;
      if (b == 0) continue;
      const uint16_t v = row[c] & 0x7fff;
      row[c] = tabs[(b & 2u) ? v : 32768 + v];
    }
  }
}

__global__ void ray_mask_count(const int4* __restrict__ rays, int num_rays, int scale,
                               long long* __restrict__ counts) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rays) return;
  const int4 q = rays[r];
  const RayWalk w = MakeRayWalk(q.x, q.y, q.z, q.w, scale);
  long long n = 0;
  for (int k = 0; k <= w.K; ++k) {
    int lo, hi;
    ColumnRun(w, k, &lo, &hi);
    n += hi - lo + 1;
  }
  counts[r] = n;
}

// The reference's order: column by column, within a column from the entry row
// towards the end point (rising for dy > 0, falling otherwise).
__global__ void ray_mask_write(const int4* __restrict__ rays, int num_rays, int scale,
                               const long long* __restrict__ offsets, int2* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= num_rays) return;
  const int4 q = rays[r];
  const RayWalk w = MakeRayWalk(q.x, q.y, q.z, q.w, scale);
  int2* o = out + offsets[r];
  const bool rising = w.K == 0 || w.dy > 0;
  for (int k = 0; k <= w.K; ++k) {
    int lo, hi;
    ColumnRun(w, k, &lo, &hi);
    if (rising)
      for (int y = lo; y <= hi; ++y) *o++ = make_int2(w.col0 + k, y);
    else
      for (int y = hi; y >= lo; --y) *o++ = make_int2(w.col0 + k, y);
  }
}

// ---------------------------------------------------------------- host -----

// probability_values.h:32-45, :84-87 and common/math.h Clamp, in float.
uint16_t CorrespondenceCostToValue(float cc) {
  const float lo = 1.f - (1.f - 0.1f), hi = 1.f - 0.1f;  // kMin/kMaxCorrespondenceCost
  const float c = cc > hi ? hi : (cc < lo ? lo : cc);
  return static_cast<uint16_t>(static_cast<int>(std::lround((c - lo) * (32766.f / (hi - lo)))) + 1);
}
float Odds(float p) { return p / (1.f - p); }
float ProbabilityFromOdds(float odds) { return odds / (odds + 1.f); }

// probability_values.cc:89-106.
void LookupTable(float odds, uint16_t* out) {
  const float lo = 1.f - (1.f - 0.1f), hi = 1.f - 0.1f;
  std::vector<float> cc(32768);
  ConversionTable(hi, lo, hi, cc.data());
  constexpr uint16_t kUpdateMarker = 1u << 15;
  out[0] = CorrespondenceCostToValue(1.f - ProbabilityFromOdds(odds)) + kUpdateMarker;
  for (int cell = 1; cell < 32768; ++cell)
    out[cell] = CorrespondenceCostToValue(1.f - ProbabilityFromOdds(odds * Odds(1.f - cc[cell]))) +
                kUpdateMarker;
}

struct ScanPlan {
  int grid = 0, round = 0;
  bool grew = false;
  int off_x = 0, off_y = 0;
  csm_map_limits before{}, after{};
  DevBuf cells, marks;  // the grown grid's buffers
};

int EnsureTables(csm_context* ctx, const csm_inserter2d_options* o) {
  if (ctx->ins_tab_key[0] == o->hit_probability && ctx->ins_tab_key[1] == o->miss_probability)
    return CSM_OK;
  std::vector<uint16_t> tabs(2 * 32768);
  LookupTable(Odds(o->hit_probability), tabs.data());
  LookupTable(Odds(o->miss_probability), tabs.data() + 32768);
  for (uint16_t& v : tabs) v &= 0x7fff;  // the device keeps no marker
  int rc;
  // Earlier inserts on the stream may still read the previous tables.
  CSM_HIP(hipStreamSynchronize(ctx->stream));
  if ((rc = ctx->ins_tabs.Reserve(tabs.size() * sizeof(uint16_t)))) return rc;
  CSM_HIP(hipMemcpy(ctx->ins_tabs.ptr, tabs.data(), tabs.size() * sizeof(uint16_t),
                    hipMemcpyHostToDevice));
  ctx->ins_tab_key[0] = o->hit_probability;
  ctx->ins_tab_key[1] = o->miss_probability;
  return CSM_OK;
}

int InsertBatch(csm_context* ctx, csm_probability_grid* const* grids, int32_t num_grids,
                const csm_inserter2d_options* o, int32_t num_scans, const int32_t* grid_of_scan,
                const float* origins, const float* returns, const int64_t* ret_off,
                const float* misses, const int64_t* miss_off) {
  if (!ctx || !grids || !o || num_grids < 1 || num_scans < 0) return CSM_EINVAL;
  if (num_scans > 0 && (!grid_of_scan || !origins || !ret_off)) return CSM_EINVAL;
  if (!miss_off) misses = nullptr;
  if (!(o->hit_probability > 0.f && o->hit_probability < 1.f && o->miss_probability > 0.f &&
        o->miss_probability < 1.f))
    return CSM_EINVAL;
  for (int g = 0; g < num_grids; ++g)
    if (!grids[g]) return CSM_EINVAL;
  if (num_scans == 0) return CSM_OK;
  const int64_t total_ret = ret_off[num_scans], total_miss = miss_off ? miss_off[num_scans] : 0;
  if (ret_off[0] != 0 || (miss_off && miss_off[0] != 0)) return CSM_EINVAL;
  if ((total_ret > 0 && !returns) || (total_miss > 0 && !misses)) return CSM_EINVAL;
  for (int s = 0; s < num_scans; ++s) {
    if (grid_of_scan[s] < 0 || grid_of_scan[s] >= num_grids) return CSM_EINVAL;
    if (ret_off[s + 1] < ret_off[s] || ret_off[s + 1] - ret_off[s] > (1 << 24)) return CSM_EINVAL;
    if (miss_off && (miss_off[s + 1] < miss_off[s] || miss_off[s + 1] - miss_off[s] > (1 << 24)))
      return CSM_EINVAL;
    if (!Finite3(origins + 3 * s)) return CSM_EINVAL;
  }
  for (int64_t i = 0; i < total_ret; ++i)
    if (!Finite3(returns + 3 * i)) return CSM_EINVAL;
  for (int64_t i = 0; i < total_miss; ++i)
    if (!Finite3(misses + 3 * i)) return CSM_EINVAL;

  // The points are checked before any handle is read.
  for (int g = 0; g < num_grids; ++g) {
    if (grids[g]->ctx != ctx) return CSM_EINVAL;
    for (int h = 0; h < g; ++h)
      if (grids[h] == grids[g]) return CSM_EINVAL;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;
  for (int g = 0; g < num_grids; ++g)
    if (grids[g]->finished) return CSM_EINVAL;

  // Plan, on the host's copy of the limits: each scan's growth (GrowAsNeeded,
  // :35-50: the float bounding box of origin, returns and misses, padded by
  // 1e-6f), its round, and the cells it can touch.
  std::vector<ScanPlan> plan(num_scans);
  std::vector<csm_map_limits> cur(num_grids);
  std::vector<int> rounds(num_grids, 0);
  std::vector<ScanDev> descs(num_scans);
  for (int g = 0; g < num_grids; ++g) cur[g] = grids[g]->limits;
  int num_rounds = 0;
  for (int s = 0; s < num_scans; ++s) {
    ScanPlan& p = plan[s];
    p.grid = grid_of_scan[s];
    p.round = rounds[p.grid]++;
    num_rounds = std::max(num_rounds, p.round + 1);
    const float* org = origins + 3 * s;
    float bmin_x = org[0], bmax_x = org[0], bmin_y = org[1], bmax_y = org[1];
    auto extend = [&](const float* q) {
      bmin_x = std::min(bmin_x, q[0]);
      bmax_x = std::max(bmax_x, q[0]);
      bmin_y = std::min(bmin_y, q[1]);
      bmax_y = std::max(bmax_y, q[1]);
    };
    for (int64_t i = ret_off[s]; i < ret_off[s + 1]; ++i) extend(returns + 3 * i);
    if (miss_off)
      for (int64_t i = miss_off[s]; i < miss_off[s + 1]; ++i) extend(misses + 3 * i);
    constexpr float kPadding = 1e-6f;
    csm_map_limits& l = cur[p.grid];
    p.before = l;
    if (!GrowLimits(&l, bmin_x - kPadding, bmin_y - kPadding, &p.off_x, &p.off_y) ||
        !GrowLimits(&l, bmax_x + kPadding, bmax_y + kPadding, &p.off_x, &p.off_y))
      return CSM_ERANGE;
    p.after = l;
    p.grew = l.num_x_cells != p.before.num_x_cells;
    // The fine index falls as the coordinate rises, so the box corners bound
    // every point's cell; one cell of slack, clamped to the grid.
    ScanDev& d = descs[s];
    d.nx = l.num_x_cells;
    d.ny = l.num_y_cells;
    d.max_x = l.max_x;
    d.max_y = l.max_y;
    d.fine_resolution = l.resolution / kSubpixelScale;
    d.ox = org[0];
    d.oy = org[1];
    d.num_returns = static_cast<int>(ret_off[s + 1] - ret_off[s]);
    d.num_misses = miss_off ? static_cast<int>(miss_off[s + 1] - miss_off[s]) : 0;
    d.ret_begin = ret_off[s];
    d.miss_begin = miss_off ? miss_off[s] : 0;
    long fx0, fy0, fx1, fy1;
    CellIndex(l, d.fine_resolution, bmax_x, bmax_y, &fx0, &fy0);
    CellIndex(l, d.fine_resolution, bmin_x, bmin_y, &fx1, &fy1);
    auto cell = [](long f, int n) {
      const long c = (f < 0 ? -((-f + kSubpixelScale - 1) / kSubpixelScale) : f / kSubpixelScale);
      return static_cast<int>(std::min<long>(std::max<long>(c, 0), n - 1));
    };
    d.box_x0 = cell(fx0 - kSubpixelScale, d.nx);
    d.box_y0 = cell(fy0 - kSubpixelScale, d.ny);
    d.box_x1 = cell(fx1 + kSubpixelScale, d.nx);
    d.box_y1 = cell(fy1 + kSubpixelScale, d.ny);
  }

  // Allocate every grown grid before anything is enqueued: a failure leaves
  // the grids as they were.
  int rc = EnsureTables(ctx, o);
  auto give_back = [&] {
    for (ScanPlan& p : plan) {
      if (p.cells.ptr) ctx->pool.Give(&p.cells);
      if (p.marks.ptr) ctx->pool.Give(&p.marks);
    }
  };
  for (int s = 0; s < num_scans && rc == CSM_OK; ++s) {
    ScanPlan& p = plan[s];
    if (!p.grew) continue;
    const size_t nx = p.after.num_x_cells, ny = p.after.num_y_cells;
    if ((rc = ctx->pool.Take(nx * ny * sizeof(uint16_t), &p.cells)) == CSM_OK)
      rc = ctx->pool.Take(static_cast<size_t>(MarkWords(nx)) * ny * sizeof(uint32_t), &p.marks);
  }
  // Scans in round order (stable), descriptors with the buffers each scan
  // will see, then one upload: descriptors, returns, misses.
  std::vector<int> order(num_scans);
  for (int s = 0; s < num_scans; ++s) order[s] = s;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return plan[a].round < plan[b].round; });
  const size_t desc_bytes = (sizeof(ScanDev) * num_scans + 255) & ~size_t(255);
  const size_t ret_bytes = (sizeof(float) * 3 * total_ret + 255) & ~size_t(255);
  const size_t miss_bytes = sizeof(float) * 3 * total_miss;
  const size_t bytes = desc_bytes + ret_bytes + miss_bytes;
  StageRing::Slot* slot = nullptr;
  if (rc == CSM_OK) rc = ctx->ins_stage.Take(bytes, &slot);
  if (rc == CSM_OK && ctx->ins_dev.bytes < bytes) {
    // The buffer is replaced: earlier inserts on the stream may still read it.
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = CSM_EHIP;
    else rc = ctx->ins_dev.Reserve(bytes + bytes / 2);
  }
  if (rc != CSM_OK) {
    give_back();
    return rc;
  }
  {
    std::vector<uint16_t*> cells(num_grids);
    std::vector<uint32_t*> marks(num_grids);
    for (int g = 0; g < num_grids; ++g) {
      cells[g] = grids[g]->cells.as<uint16_t>();
      marks[g] = grids[g]->marks.as<uint32_t>();
    }
    ScanDev* hd = slot->buf.as<ScanDev>();
    for (int i = 0; i < num_scans; ++i) {
      const int s = order[i];
      ScanPlan& p = plan[s];
      if (p.grew) {
        cells[p.grid] = p.cells.as<uint16_t>();
        marks[p.grid] = p.marks.as<uint32_t>();
      }
      descs[s].cells = cells[p.grid];
      descs[s].marks = marks[p.grid];
      hd[i] = descs[s];
    }
    char* h = slot->buf.as<char>();
    if (total_ret) std::memcpy(h + desc_bytes, returns, sizeof(float) * 3 * total_ret);
    if (total_miss) std::memcpy(h + desc_bytes + ret_bytes, misses, miss_bytes);
  }
  hipStream_t st = ctx->stream;
  // From here on a failure is a HIP error: the stream's state is unknown and
  // the grids keep their old buffers and limits.
  if (hipMemcpyAsync(ctx->ins_dev.ptr, slot->buf.ptr, bytes, hipMemcpyHostToDevice, st) !=
          hipSuccess ||
      hipEventRecord(slot->copied, st) != hipSuccess) {
    give_back();
    return CSM_EHIP;
  }
  const ScanDev* dd = ctx->ins_dev.as<ScanDev>();
  const float* dret = reinterpret_cast<const float*>(ctx->ins_dev.as<char>() + desc_bytes);
  const float* dmiss =
      reinterpret_cast<const float*>(ctx->ins_dev.as<char>() + desc_bytes + ret_bytes);
  std::deque<DevBuf> retired;
  int i0 = 0;
  for (int r = 0; r < num_rounds; ++r) {
    int i1 = i0;
    int64_t max_rays = 1, max_words = 1;
    for (; i1 < num_scans && plan[order[i1]].round == r; ++i1) {
      const int s = order[i1];
      ScanPlan& p = plan[s];
      csm_probability_grid* g = grids[p.grid];
      if (p.grew) {
        const size_t nx = p.after.num_x_cells, ny = p.after.num_y_cells;
        CSM_HIP(hipMemsetAsync(p.cells.ptr, 0, nx * ny * sizeof(uint16_t), st));
        CSM_HIP(hipMemsetAsync(p.marks.ptr, 0, MarkWords(nx) * ny * sizeof(uint32_t), st));
        const int ow = p.before.num_x_cells, oh = p.before.num_y_cells;
        hipLaunchKernelGGL(insert2d_copy_rect, dim3(Blocks(int64_t{ow} * oh, 256, 4096)),
                           dim3(256), 0, st, g->cells.as<uint16_t>(), ow, 0, 0,
                           p.cells.as<uint16_t>(), static_cast<int>(nx), p.off_x, p.off_y, ow, oh);
        CSM_HIP(hipGetLastError());
        retired.emplace_back();
        MoveBuf(&g->cells, &retired.back());
        retired.emplace_back();
        MoveBuf(&g->marks, &retired.back());
        MoveBuf(&p.cells, &g->cells);
        MoveBuf(&p.marks, &g->marks);
      }
      g->limits = p.after;
      ++g->generation;
      const ScanDev& d = descs[s];
      max_rays = std::max<int64_t>(max_rays, o->insert_free_space
                                                 ? int64_t{d.num_returns} + d.num_misses
                                                 : (d.num_returns + 63) / 64);
      max_words = std::max<int64_t>(
          max_words, int64_t{(d.box_x1 >> 4) - (d.box_x0 >> 4) + 1} * (d.box_y1 - d.box_y0 + 1));
    }
    const unsigned ny = static_cast<unsigned>(i1 - i0);
    // 65535 scans per launch (gridDim.y).
    for (unsigned y0 = 0; y0 < ny; y0 += 65535) {
      const unsigned nyy = std::min(65535u, ny - y0);
      hipLaunchKernelGGL(insert2d_mark, dim3(Blocks(max_rays, 4, 1024), nyy), dim3(256), 0, st,
                         dd + i0 + y0, dret, dmiss, o->insert_free_space ? 1 : 0);
      CSM_HIP(hipGetLastError());
      hipLaunchKernelGGL(insert2d_apply, dim3(Blocks(max_words, 256, 1024), nyy), dim3(256), 0,
                         st, dd + i0 + y0, ctx->ins_tabs.as<uint16_t>());
      CSM_HIP(hipGetLastError());
    }
    i0 = i1;
  }
  // The old buffers of grown grids: reused by later takes on this stream.
  for (DevBuf& b : retired)
    if (b.ptr) ctx->pool.Give(&b);
  return CSM_OK;
}

}  // namespace
}  // namespace csm

using namespace csm;

extern "C" {

int csm_inserter2d_lookup_table(float probability, uint16_t* out) {
  if (!out || !(probability > 0.f && probability < 1.f)) return CSM_EINVAL;
  LookupTable(Odds(probability), out);
  return CSM_OK;
}

int csm_probability_grid_create(csm_context* ctx, const csm_map_limits* limits,
                                const uint16_t* cells, csm_probability_grid** out) {
  if (!ctx || !limits || !out) return CSM_EINVAL;
  if (limits->num_x_cells < 1 || limits->num_y_cells < 1 || !(limits->resolution > 0.) ||
      !std::isfinite(limits->resolution) || !std::isfinite(limits->max_x) ||
      !std::isfinite(limits->max_y))
    return CSM_EINVAL;
  if (limits->num_x_cells > kMaxSide || limits->num_y_cells > kMaxSide) return CSM_ERANGE;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;
  auto g = std::make_unique<csm_probability_grid>();
  g->ctx = ctx;
  g->limits = *limits;
  g->id = g_next_grid_id.fetch_add(1);
  const size_t nx = limits->num_x_cells, ny = limits->num_y_cells;
  const size_t mark_bytes = static_cast<size_t>(MarkWords(nx)) * ny * sizeof(uint32_t);
  int rc;
  if ((rc = ctx->pool.Take(nx * ny * sizeof(uint16_t), &g->cells)) ||
      (rc = ctx->pool.Take(mark_bytes, &g->marks))) {
    if (g->cells.ptr) ctx->pool.Give(&g->cells);
    return rc;
  }
  hipStream_t st = ctx->stream;
  bool ok = hipMemsetAsync(g->marks.ptr, 0, mark_bytes, st) == hipSuccess;
  if (cells) {
    // The caller's memory is read: finish before returning.
    ok = ok && hipMemcpyAsync(g->cells.ptr, cells, nx * ny * sizeof(uint16_t),
                              hipMemcpyHostToDevice, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
  } else {
    ok = ok && hipMemsetAsync(g->cells.ptr, 0, nx * ny * sizeof(uint16_t), st) == hipSuccess;
  }
  if (!ok) {
    ctx->pool.Give(&g->cells);
    ctx->pool.Give(&g->marks);
    return CSM_EHIP;
  }
  *out = g.release();
  return CSM_OK;
}

void csm_probability_grid_destroy(csm_probability_grid* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  if (g->cells.ptr) g->ctx->pool.Give(&g->cells);
  if (g->marks.ptr) g->ctx->pool.Give(&g->marks);
  delete g;
}

int csm_probability_grid_limits(const csm_probability_grid* g, csm_map_limits* out) {
  if (!g || !out) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(g->ctx->mu);
  *out = g->limits;
  return CSM_OK;
}

int csm_probability_grid_read(const csm_probability_grid* g, uint16_t* out, int64_t capacity) {
  if (!g || !out) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(g->ctx->mu);
  const int64_t n = static_cast<int64_t>(g->limits.num_x_cells) * g->limits.num_y_cells;
  if (capacity < n) return CSM_EINVAL;
  if (EnsureDevice(g->ctx)) return CSM_EHIP;
  CSM_HIP(hipMemcpyAsync(out, g->cells.ptr, n * sizeof(uint16_t), hipMemcpyDeviceToHost,
                         g->ctx->stream));
  CSM_HIP(hipStreamSynchronize(g->ctx->stream));
  return CSM_OK;
}

int csm_probability_grid_insert(csm_probability_grid* g, const csm_inserter2d_options* o,
                                const float* origin, const float* returns, int32_t num_returns,
                                const float* misses, int32_t num_misses) {
  if (!g || !o || !origin || num_returns < 0 || num_misses < 0) return CSM_EINVAL;
  if ((num_returns > 0 && !returns) || (num_misses > 0 && !misses)) return CSM_EINVAL;
  // The points are checked before the handle is read.
  if (!Finite3(origin)) return CSM_EINVAL;
  for (int32_t i = 0; i < num_returns; ++i)
    if (!Finite3(returns + 3 * i)) return CSM_EINVAL;
  for (int32_t i = 0; i < num_misses; ++i)
    if (!Finite3(misses + 3 * i)) return CSM_EINVAL;
  const int32_t zero = 0;
  const int64_t ro[2] = {0, num_returns}, mo[2] = {0, num_misses};
  csm_probability_grid* const grids[1] = {g};
  return InsertBatch(g->ctx, grids, 1, o, 1, &zero, origin, returns, ro,
                     num_misses > 0 ? misses : nullptr, num_misses > 0 ? mo : nullptr);
}

int csm_probability_grid_insert_batch(csm_context* ctx, csm_probability_grid* const* grids,
                                      int32_t num_grids, const csm_inserter2d_options* o,
                                      int32_t num_scans, const int32_t* grid_of_scan,
                                      const float* origins, const float* returns,
                                      const int64_t* ret_off, const float* misses,
                                      const int64_t* miss_off) {
  return InsertBatch(ctx, grids, num_grids, o, num_scans, grid_of_scan, origins, returns, ret_off,
                     misses, miss_off);
}

int csm_probability_grid_finish(csm_probability_grid* g) {
  if (!g) return CSM_EINVAL;
  csm_context* ctx = g->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (g->finished) return CSM_OK;  // Submap2D::Finish runs once; a second call changes nothing
  if (EnsureDevice(ctx)) return CSM_EHIP;
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = ctx->ins_box.Reserve(4 * sizeof(int))) ||
      (rc = ctx->ins_box_host.Reserve(4 * sizeof(int))))
    return rc;
  int* hb = ctx->ins_box_host.as<int>();
  hb[0] = hb[1] = INT_MAX;
  hb[2] = hb[3] = -1;
  const int nx = g->limits.num_x_cells, ny = g->limits.num_y_cells;
  CSM_HIP(hipMemcpyAsync(ctx->ins_box.ptr, hb, 4 * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(insert2d_box, dim3(Blocks(int64_t{nx} * ny, 1024, 1024)), dim3(256), 0, st,
                     g->cells.as<uint16_t>(), nx, ny, ctx->ins_box.as<int>());
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(hb, ctx->ins_box.ptr, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  // Grid2D::ComputeCroppedLimits (grid_2d.cc:121-132) and the new max
  // (probability_grid.cc:95-99).
  const bool empty = hb[2] < 0;
  const int ox = empty ? 0 : hb[0], oy = empty ? 0 : hb[1];
  const int cnx = empty ? 1 : hb[2] - hb[0] + 1, cny = empty ? 1 : hb[3] - hb[1] + 1;
  DevBuf cropped;
  if ((rc = ctx->pool.Take(static_cast<size_t>(cnx) * cny * sizeof(uint16_t), &cropped))) return rc;
  if (empty) {
    CSM_HIP(hipMemsetAsync(cropped.ptr, 0, sizeof(uint16_t), st));
  } else {
    hipLaunchKernelGGL(insert2d_copy_rect, dim3(Blocks(int64_t{cnx} * cny, 256, 4096)), dim3(256),
                       0, st, g->cells.as<uint16_t>(), nx, ox, oy, cropped.as<uint16_t>(), cnx, 0,
                       0, cnx, cny);
    CSM_HIP(hipGetLastError());
  }
  ctx->pool.Give(&g->cells);  // reused by later takes on this stream
  ctx->pool.Give(&g->marks);
  MoveBuf(&cropped, &g->cells);
  g->limits.max_x = g->limits.max_x - g->limits.resolution * static_cast<double>(oy);
  g->limits.max_y = g->limits.max_y - g->limits.resolution * static_cast<double>(ox);
  g->limits.num_x_cells = cnx;
  g->limits.num_y_cells = cny;
  g->finished = true;
  ++g->generation;
  return CSM_OK;
}

int csm_rt2d_match_grid(csm_context* ctx, const csm_rt_options* options,
                        const csm_probability_grid* grid, const csm_pose2d* initial,
                        const float* points_xyz, int32_t n, double* score, csm_pose2d* pose) {
  if (!ctx || !grid || grid->ctx != ctx) return CSM_EINVAL;
  return Rt2dMatchGrid(ctx, options, grid, initial, points_xyz, n, score, pose);
}

int csm_ray_to_pixel_mask(csm_context* ctx, const int32_t* rays, int32_t num_rays, int32_t scale,
                          int32_t* cells_xy, int64_t capacity, int64_t* ray_offsets) {
  if (!ctx || num_rays < 0 || scale < 1 || !ray_offsets || (num_rays > 0 && !rays))
    return CSM_EINVAL;
  for (int64_t i = 0; i < int64_t{4} * num_rays; ++i)
    if (rays[i] < 0 || rays[i] >= kMaxCoord) return CSM_EINVAL;
  ray_offsets[0] = 0;
  if (num_rays == 0) return CSM_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;
  hipStream_t st = ctx->stream;
  int rc;
  const size_t n = num_rays;
  if ((rc = ctx->ins_rays.Reserve(n * sizeof(int4))) ||
      (rc = ctx->ins_count.Reserve(n * sizeof(long long))))
    return rc;
  CSM_HIP(hipMemcpyAsync(ctx->ins_rays.ptr, rays, n * sizeof(int4), hipMemcpyHostToDevice, st));
  const dim3 blocks(static_cast<unsigned>((n + 255) / 256));
  hipLaunchKernelGGL(ray_mask_count, blocks, dim3(256), 0, st, ctx->ins_rays.as<int4>(), num_rays,
                     scale, ctx->ins_count.as<long long>());
  CSM_HIP(hipGetLastError());
  std::vector<long long> counts(n);
  CSM_HIP(hipMemcpyAsync(counts.data(), ctx->ins_count.ptr, n * sizeof(long long),
                         hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  for (size_t r = 0; r < n; ++r) ray_offsets[r + 1] = ray_offsets[r] + counts[r];
  if (!cells_xy) return CSM_OK;
  const int64_t total = ray_offsets[n];
  if (capacity < total) return CSM_EINVAL;
  if (total > (int64_t{1} << 28)) return CSM_ERANGE;
  for (size_t r = 0; r < n; ++r) counts[r] = ray_offsets[r];
  if ((rc = ctx->ins_mask.Reserve(static_cast<size_t>(total) * sizeof(int2)))) return rc;
  CSM_HIP(hipMemcpyAsync(ctx->ins_count.ptr, counts.data(), n * sizeof(long long),
                         hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ray_mask_write, blocks, dim3(256), 0, st, ctx->ins_rays.as<int4>(), num_rays,
                     scale, ctx->ins_count.as<long long>(), ctx->ins_mask.as<int2>());
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(cells_xy, ctx->ins_mask.ptr, static_cast<size_t>(total) * sizeof(int2),
                         hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

}  // extern "C"
