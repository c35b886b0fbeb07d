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
// The column walk (RayWalk, ColumnRun), the copy_rect / box kernels and the
// host steps of growth, create and crop over a grid's list of planes are
// shared with the TSDF inserter (insert2d_common.h); the steps of an insert
// call around the kernels with all three inserters (insert_host.h).
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

size_t CellBytes(size_t nx, size_t ny) { return nx * ny * sizeof(uint16_t); }
size_t MarkBytes(size_t nx, size_t ny) {
  return static_cast<size_t>(MarkWords(static_cast<int>(nx))) * ny * sizeof(uint32_t);
}
// The planes of a ProbabilityGrid as growth sees them (insert2d_common.h).
const Plane2<csm_probability_grid> kPlanes[] = {
    {&csm_probability_grid::cells, CellBytes, 0, true},
    {&csm_probability_grid::marks, MarkBytes, 0, false}};

// One scan's plan on the host's copy of its grid's limits: its growth
// (GrowAsNeeded, :35-50: the float bounding box of origin, returns and
// misses), its round, and the cells it can touch. False past kMaxSide.
bool PlanScan(int grid, const float* org, const float* returns, int num_returns,
              const float* misses, int num_misses, std::vector<csm_map_limits>* limits,
              std::vector<int>* rounds, GrowPlan2* p, ScanDev* out) {
  float bmin_x = org[0], bmax_x = org[0], bmin_y = org[1], bmax_y = org[1];
  auto extend = [&](const float* q) {
    bmin_x = std::min(bmin_x, q[0]);
    bmax_x = std::max(bmax_x, q[0]);
    bmin_y = std::min(bmin_y, q[1]);
    bmax_y = std::max(bmax_y, q[1]);
  };
  for (int i = 0; i < num_returns; ++i) extend(returns + 3 * i);
  for (int i = 0; i < num_misses; ++i) extend(misses + 3 * i);
  const float box[4] = {bmin_x, bmin_y, bmax_x, bmax_y};
  if (!PlanGrowth2(grid, box, limits, rounds, p)) return false;
  const csm_map_limits& l = p->after;
  // The fine index falls as the coordinate rises, so the box corners bound
  // every point's cell; one cell of slack, clamped to the grid.
  ScanDev& d = *out;
  d.nx = l.num_x_cells;
  d.ny = l.num_y_cells;
  d.max_x = l.max_x;
  d.max_y = l.max_y;
  d.fine_resolution = l.resolution / kSubpixelScale;
  d.ox = org[0];
  d.oy = org[1];
  d.num_returns = num_returns;
  d.num_misses = num_misses;
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
  return true;
}

int InsertBatch(csm_context* ctx, csm_probability_grid* const* grids, int32_t num_grids,
                const csm_inserter2d_options* o, int32_t num_scans, const int32_t* grid_of_scan,
                const float* origins, const float* returns, const int64_t* ret_off,
                const float* misses, const int64_t* miss_off) {
  if (!ctx || !grids || !o || num_grids < 1 || num_scans < 0) return CSM_EINVAL;
  if (num_scans > 0 && (!grid_of_scan || !origins || !ret_off)) return CSM_EINVAL;
  if (!(o->hit_probability > 0.f && o->hit_probability < 1.f && o->miss_probability > 0.f &&
        o->miss_probability < 1.f))
    return CSM_EINVAL;
  for (int g = 0; g < num_grids; ++g)
    if (!grids[g]) return CSM_EINVAL;
  if (num_scans == 0) return CSM_OK;
  if (!ValidScans(num_scans, origins, ret_off, returns) ||
      (miss_off && !ValidPoints(num_scans, miss_off, misses)))
    return CSM_EINVAL;
  for (int s = 0; s < num_scans; ++s)
    if (grid_of_scan[s] < 0 || grid_of_scan[s] >= num_grids) return CSM_EINVAL;
  const int64_t total_ret = ret_off[num_scans], total_miss = miss_off ? miss_off[num_scans] : 0;
  // The points are checked before any handle is read.
  if (!ValidHandles(ctx, grids, num_grids)) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;
  for (int g = 0; g < num_grids; ++g)
    if (grids[g]->finished) return CSM_EINVAL;

  std::vector<GrowPlan2> plan(num_scans);
  std::vector<csm_map_limits> cur(num_grids);
  std::vector<int> rounds(num_grids, 0);
  std::vector<ScanDev> descs(num_scans);
  for (int g = 0; g < num_grids; ++g) cur[g] = grids[g]->limits;
  for (int s = 0; s < num_scans; ++s) {
    ScanDev& d = descs[s];
    d.ret_begin = ret_off[s];
    d.miss_begin = miss_off ? miss_off[s] : 0;
    if (!PlanScan(grid_of_scan[s], origins + 3 * s, returns + 3 * d.ret_begin,
                  static_cast<int>(ret_off[s + 1] - ret_off[s]), misses + 3 * d.miss_begin,
                  miss_off ? static_cast<int>(miss_off[s + 1] - miss_off[s]) : 0, &cur, &rounds,
                  &plan[s], &d))
      return CSM_ERANGE;
  }
  // Scans in round order (stable).
  std::vector<int> order(num_scans);
  for (int s = 0; s < num_scans; ++s) order[s] = s;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return plan[a].round < plan[b].round; });

  // Everything that can fail cleanly, before anything is enqueued: a failure
  // leaves the grids as they were. One upload: descriptors, returns, misses.
  const size_t desc_bytes = Align(sizeof(ScanDev) * num_scans);
  const size_t ret_bytes = Align(sizeof(float) * 3 * total_ret);
  const size_t miss_bytes = sizeof(float) * 3 * total_miss;
  const size_t bytes = desc_bytes + ret_bytes + miss_bytes;
  StageRing::Slot* slot = nullptr;
  int rc = EnsureOddsTables(ctx, o->hit_probability, o->miss_probability, LookupTable,
                            &ctx->ins_tabs, ctx->ins_tab_key);
  if (rc == CSM_OK) rc = TakeGrown2(ctx, grids, num_grids, kPlanes, &plan);
  if (rc == CSM_OK) rc = ReserveUpload(ctx, &ctx->ins_stage, &ctx->ins_dev, bytes, &slot);
  if (rc != CSM_OK) {
    GiveBackGrown2(ctx, &plan);
    return rc;
  }
  char* h = slot->buf.as<char>();
  ScanDev* hd = slot->buf.as<ScanDev>();
  for (int i = 0; i < num_scans; ++i) {
    hd[i] = descs[order[i]];
    hd[i].cells = static_cast<uint16_t*>(plan[order[i]].seen[0]);
    hd[i].marks = static_cast<uint32_t*>(plan[order[i]].seen[1]);
  }
  if (total_ret) std::memcpy(h + desc_bytes, returns, sizeof(float) * 3 * total_ret);
  if (total_miss) std::memcpy(h + desc_bytes + ret_bytes, misses, miss_bytes);
  // From here on a failure is a HIP error (insert_host.h): the grids keep what
  // they had when it struck.
  if ((rc = Upload(ctx, slot, &ctx->ins_dev, bytes))) return rc;
  hipStream_t st = ctx->stream;
  const ScanDev* dd = ctx->ins_dev.as<ScanDev>();
  const float* dret = reinterpret_cast<const float*>(ctx->ins_dev.as<char>() + desc_bytes);
  const float* dmiss =
      reinterpret_cast<const float*>(ctx->ins_dev.as<char>() + desc_bytes + ret_bytes);
  std::deque<DevBuf> retired;
  for (int i0 = 0, i1 = 0; i0 < num_scans; i0 = i1) {  // a round: [i0, i1)
    int64_t max_rays = 1, max_words = 1;
    for (; i1 < num_scans && plan[order[i1]].round == plan[order[i0]].round; ++i1) {
      const int s = order[i1];
      if ((rc = CommitScan2(ctx, grids[plan[s].grid], kPlanes, &plan[s], &retired))) return rc;
      const ScanDev& d = descs[s];
      max_rays = std::max<int64_t>(max_rays, o->insert_free_space
                                                 ? int64_t{d.num_returns} + d.num_misses
                                                 : (d.num_returns + 63) / 64);
      max_words = std::max<int64_t>(
          max_words, int64_t{(d.box_x1 >> 4) - (d.box_x0 >> 4) + 1} * (d.box_y1 - d.box_y0 + 1));
    }
    for (int y0 = i0; y0 < i1; y0 += kMaxGridY) {
      const unsigned nyy = ChunkOf(y0, i1);
      hipLaunchKernelGGL(insert2d_mark, dim3(Blocks(max_rays, 4, 1024), nyy), dim3(256), 0, st,
                         dd + y0, dret, dmiss, o->insert_free_space ? 1 : 0);
      CSM_HIP(hipGetLastError());
      hipLaunchKernelGGL(insert2d_apply, dim3(Blocks(max_words, 256, 1024), nyy), dim3(256), 0,
                         st, dd + y0, ctx->ins_tabs.as<uint16_t>());
      CSM_HIP(hipGetLastError());
    }
  }
  // The old buffers of grown grids: reused by later takes on this stream.
  for (DevBuf& b : retired) ctx->pool.Give(&b);
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
  if (int rc = CheckLimits2(limits)) return rc;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;
  auto g = std::make_unique<csm_probability_grid>();
  g->ctx = ctx;
  g->limits = *limits;
  g->id = g_next_grid_id.fetch_add(1);
  const uint16_t* const host[] = {cells, nullptr};
  if (int rc = NewPlanes2(g.get(), kPlanes, host)) return rc;
  *out = g.release();
  return CSM_OK;
}

void csm_probability_grid_destroy(csm_probability_grid* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  GivePlanes2(g, kPlanes);
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
  const int32_t zero = 0;
  const int64_t ro[2] = {0, num_returns}, mo[2] = {0, num_misses};
  // The points are checked before the handle is read.
  if (!ValidScans(1, origin, ro, returns) || !ValidPoints(1, mo, misses)) return CSM_EINVAL;
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
  const int nx = g->limits.num_x_cells, ny = g->limits.num_y_cells;
  int rc;
  Crop2 c;
  if ((rc = CropBox2(ctx, g->cells.as<uint16_t>(), nx, ny, &c))) return rc;
  DevBuf cropped;
  if ((rc = ctx->pool.Take(CellBytes(c.nx, c.ny), &cropped))) return rc;
  if (c.empty) {
    CSM_HIP(hipMemsetAsync(cropped.ptr, 0, sizeof(uint16_t), st));
  } else {
    hipLaunchKernelGGL(insert2d_copy_rect, dim3(Blocks(int64_t{c.nx} * c.ny, 256, 4096)),
                       dim3(256), 0, st, g->cells.as<uint16_t>(), nx, c.ox, c.oy,
                       cropped.as<uint16_t>(), c.nx, 0, 0, c.nx, c.ny);
    CSM_HIP(hipGetLastError());
  }
  GivePlanes2(g, kPlanes);  // reused by later takes on this stream
  g->cells = std::move(cropped);
  FinishCrop2(g, c);
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
