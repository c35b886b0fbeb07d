// RangeDataInserter3D::Insert on the device brick of a csm_hybrid_grid, on
// gfx950 (range_data_inserter_3d.cc:44-74, :109-137; hybrid_grid.h
// ApplyLookupTable / FinishUpdate :497-521, DynamicGrid::Grow :384-399;
// submap_3d.cc:91-99; probability_values.cc:76-87), and the host pieces of
// Submap3D next to it (rotational_scan_matcher.cc:138-158).
//
// Why the result does not depend on thread order. Within one Insert the
// update marker admits one table lookup per cell and every hit is applied
// before any miss, so a cell ends as hit_table[old] if a return lands in it,
// else miss_table[old] if it lies on a ray's miss span, else old. The device
// keeps the reference's own marker: bit 15 of the cell's value. A thread that
// wants to update a cell sets the bit with an atomicOr on the 32-bit word that
// holds the cell and its neighbour; exactly one thread sees the bit clear in
// the value the atomic returns, and that thread alone replaces the low 15
// bits (an atomicXor of old ^ table[old], which leaves the neighbour's half
// as it is). Which thread wins does not matter: every contender would write
// the same table[old]. Hits and misses are separate launches, so every hit
// cell carries the marker before the first miss is tried. A third launch
// walks the same points and spans, clears each marker with an atomicAnd (one
// thread per cell sees it set in the returned value) and that thread writes
// the cell's float probability. No side buffer exists, so nothing has to be
// cleared between calls, and every pass costs returns x touched cells.
//
// Kernels. blockIdx.y is the job (one scan into one grid) of a round.
//   insert3d_hits  one thread per return: transform, range filter, cell, hit.
//   insert3d_rays  <false>: the miss span of every ray; a group of G lanes
//                  (G a power of two near num_free_space_voxels, at most 64)
//                  shares a ray. <true>: FinishUpdate over the hit cell and
//                  the same span, with the probability brick's update.
//   insert3d_grow  a grown grid's new bricks: the old cells at their offset,
//                  unknown (0, kMinProbability) elsewhere.
//
// Intensities (InsertIntensitiesIntoGrid, :76-89, into a csm_intensity_grid).
// cell->sum += intensity is a float sum in returns order, so a cell that
// several returns of a scan share must take them in index order, continued
// from its old sum. No float atomic touches the sums:
//   insert3d_intensity_keys  one thread per return writes (job of the round,
//                  cell index in the brick) as a 64-bit key and the return's
//                  index as the value; a return that is filtered out, above
//                  the threshold or of a job without intensities gets a key
//                  past every real one.
//   rocprim::radix_sort_pairs  stable, so equal keys keep index order.
//   insert3d_intensity_sums  one thread per sorted pair; the one at the head
//                  of a run of equal keys (found in an LDS tile of the
//                  block's keys) walks the run, adds in index order, stores
//                  the sum once and adds the run's length to the count.
// Work is proportional to the returns; the bricks are touched only at the
// cells that change.
//
// The host steps of an insert call around the kernels are insert_host.h's.
#include <hip/hip_runtime.h>
// The radix sort alone: rocprim.hpp also pulls in texture iterators.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <vector>

#include "csm_internal.h"
#include "insert_host.h"

namespace csm {
namespace {

constexpr uint32_t kMarker = 0x8000u;  // kUpdateMarker (probability_values.h:94)
constexpr int kMaxSamples = 1 << 15;   // CHECK_LT(num_samples, 1 << 15), :58
constexpr float kMaxCell = 1.0e9f;     // |coordinate / resolution| the index arithmetic takes

// One (grid, scan) job of a round, as the kernels see it. The origin is
// already in the grid's frame; the returns are transformed on the device.
struct Job3 {
  uint32_t* words;  // the value brick, two cells per word
  float* prob;
  unsigned long long* stats;  // [0] cells visited by the finish pass, [1] cells updated
  Brick3 b;
  float resolution;
  float ox, oy, oz;     // origin (range_data.origin after the transform)
  int cx, cy, cz;       // its cell
  int has_transform;
  float t[3], q[4];     // submap from local: translation, rotation (w, x, y, z)
  float max_range;      // <= 0: none
  int64_t begin;        // first return in the points array
  int num_returns;
};

// Rigid3f * Vector3f (rigid_transform.h:191-196) with Eigen's
// Quaternion::_transformVector: uv = 2 q.vec x v, v + w uv + q.vec x uv.
__host__ __device__ inline void Apply3(const float* t, const float* q, float* p) {
#ifdef __HIP_DEVICE_COMPILE__
#define CSM_MUL(a, b) __fmul_rn(a, b)
#define CSM_ADD(a, b) __fadd_rn(a, b)
#define CSM_SUB(a, b) __fsub_rn(a, b)
#else
#define CSM_MUL(a, b) ((a) * (b))
#define CSM_ADD(a, b) ((a) + (b))
#define CSM_SUB(a, b) ((a) - (b))
#endif
  const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float vx = p[0], vy = p[1], vz = p[2];
  float ux = CSM_SUB(CSM_MUL(qy, vz), CSM_MUL(qz, vy));
  float uy = CSM_SUB(CSM_MUL(qz, vx), CSM_MUL(qx, vz));
  float uz = CSM_SUB(CSM_MUL(qx, vy), CSM_MUL(qy, vx));
  ux = CSM_ADD(ux, ux);
  uy = CSM_ADD(uy, uy);
  uz = CSM_ADD(uz, uz);
  const float cx = CSM_SUB(CSM_MUL(qy, uz), CSM_MUL(qz, uy));
  const float cy = CSM_SUB(CSM_MUL(qz, ux), CSM_MUL(qx, uz));
  const float cz = CSM_SUB(CSM_MUL(qx, uy), CSM_MUL(qy, ux));
  p[0] = CSM_ADD(CSM_ADD(CSM_ADD(vx, CSM_MUL(qw, ux)), cx), t[0]);
  p[1] = CSM_ADD(CSM_ADD(CSM_ADD(vy, CSM_MUL(qw, uy)), cy), t[1]);
  p[2] = CSM_ADD(CSM_ADD(CSM_ADD(vz, CSM_MUL(qw, uz)), cz), t[2]);
}

// (p - origin).norm() as Eigen sums three squares: x0 + (x1 + x2).
__host__ __device__ inline float RangeOf(const float* p, float ox, float oy, float oz) {
  const float dx = CSM_SUB(p[0], ox), dy = CSM_SUB(p[1], oy), dz = CSM_SUB(p[2], oz);
  const float s = CSM_ADD(CSM_MUL(dx, dx), CSM_ADD(CSM_MUL(dy, dy), CSM_MUL(dz, dz)));
#ifdef __HIP_DEVICE_COMPILE__
  return __fsqrt_rn(s);
#else
  return std::sqrt(s);
#endif
}

// HybridGrid::GetCellIndex (hybrid_grid.h:428-433): float division, lround.
__device__ inline float CellF(float v, float resolution) {
  return roundf(__fdiv_rn(v, resolution));
}

// The return's position in the grid's frame and whether the job keeps it
// (FilterRangeDataByMaxRange, submap_3d.cc:91-99).
__host__ __device__ inline bool JobPoint(const Job3& j, const float* src, float* p) {
  p[0] = src[0];
  p[1] = src[1];
  p[2] = src[2];
  if (j.has_transform) Apply3(j.t, j.q, p);
  if (j.max_range > 0.f && !(RangeOf(p, j.ox, j.oy, j.oz) <= j.max_range)) return false;
  return true;
}

// The miss span of a ray (InsertMissesIntoGrid, :44-74).
struct Span3 {
  int dx, dy, dz, num_samples, first;
};
__host__ __device__ inline Span3 MakeSpan(int cx, int cy, int cz, int hx, int hy, int hz,
                                          int free_voxels) {
  Span3 s;
  s.dx = hx - cx;
  s.dy = hy - cy;
  s.dz = hz - cz;
  const int ax = s.dx < 0 ? -s.dx : s.dx, ay = s.dy < 0 ? -s.dy : s.dy,
            az = s.dz < 0 ? -s.dz : s.dz;
  s.num_samples = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
  s.first = s.num_samples > free_voxels ? s.num_samples - free_voxels : 0;
  return s;
}
// origin_cell + delta * position / num_samples, C++ integer division;
// num_samples > 0, |delta| and position < 2^15.
__host__ __device__ inline void SpanCell(int cx, int cy, int cz, const Span3& s, int position,
                                         int* x, int* y, int* z) {
  *x = cx + s.dx * position / s.num_samples;
  *y = cy + s.dy * position / s.num_samples;
  *z = cz + s.dz * position / s.num_samples;
}

// The cell's index in the brick, -1 outside it.
__device__ inline int64_t BrickIndex(const Brick3& b, int x, int y, int z) {
  const unsigned ux = static_cast<unsigned>(x - b.ox), uy = static_cast<unsigned>(y - b.oy),
                 uz = static_cast<unsigned>(z - b.oz);
  if (ux >= static_cast<unsigned>(b.nx) || uy >= static_cast<unsigned>(b.ny) ||
      uz >= static_cast<unsigned>(b.nz))
    return -1;
  return (static_cast<int64_t>(uz) * b.ny + uy) * b.nx + ux;
}

// ApplyLookupTable: table[old] for the one thread that sets the marker.
__device__ inline void ApplyCell(const Job3& j, int x, int y, int z,
                                 const uint16_t* __restrict__ table) {
  const int64_t i = BrickIndex(j.b, x, y, z);
  if (i < 0) return;
  uint32_t* w = j.words + (i >> 1);
  const int shift = (i & 1) * 16;
  const uint32_t m = kMarker << shift;
  // The marker only rises during these passes: a stale zero costs one
  // redundant atomic, never a lost update. Rays of one scan share the cells
  // near the origin and near each other's hits; this keeps them off the word.
  if (__atomic_load_n(w, __ATOMIC_RELAXED) & m) return;
  const uint32_t old = atomicOr(w, m);
  if (old & m) return;
  const uint32_t v = (old >> shift) & 0x7fffu;
  atomicXor(w, (v ^ table[v]) << shift);
}

// FinishUpdate for one cell: the thread that clears the marker also writes
// the probability. Returns 1 when this thread was the one.
__device__ inline int FinishCell(const Job3& j, int x, int y, int z,
                                 const float* __restrict__ ptab) {
  const int64_t i = BrickIndex(j.b, x, y, z);
  if (i < 0) return 0;
  uint32_t* w = j.words + (i >> 1);
  const int shift = (i & 1) * 16;
  const uint32_t m = kMarker << shift;
  if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & m)) return 0;
  const uint32_t old = atomicAnd(w, ~m);
  if (!(old & m)) return 0;
  j.prob[i] = ptab[(old >> shift) & 0x7fffu];
  return 1;
}

__device__ inline bool HitCellOf(const Job3& j, const float* __restrict__ points, int i, int* hx,
                                 int* hy, int* hz) {
  float p[3];
  if (!JobPoint(j, points + 3 * (j.begin + i), p)) return false;
  *hx = static_cast<int>(CellF(p[0], j.resolution));
  *hy = static_cast<int>(CellF(p[1], j.resolution));
  *hz = static_cast<int>(CellF(p[2], j.resolution));
  return true;
}

// tabs: hit table then miss table, 32768 entries each, update marker removed.
__global__ void __launch_bounds__(256)
insert3d_hits(const Job3* __restrict__ jobs, const float* __restrict__ points,
              const uint16_t* __restrict__ tabs) {
  const Job3 j = jobs[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < j.num_returns;
       i += gridDim.x * blockDim.x) {
    int hx, hy, hz;
    if (HitCellOf(j, points, i, &hx, &hy, &hz)) ApplyCell(j, hx, hy, hz, tabs);
  }
}

template <bool kFinish>
__global__ void __launch_bounds__(256)
insert3d_rays(const Job3* __restrict__ jobs, const float* __restrict__ points,
              const uint16_t* __restrict__ tabs, const float* __restrict__ ptab, int free_voxels,
              int group_bits) {
  const Job3 j = jobs[blockIdx.y];
  const int group = 1 << group_bits;
  const int sub = threadIdx.x & (group - 1);
  const int rays_per_block = blockDim.x >> group_bits;
  int visited = 0, updated = 0;
  for (int ray = blockIdx.x * rays_per_block + (threadIdx.x >> group_bits); ray < j.num_returns;
       ray += gridDim.x * rays_per_block) {
    int hx, hy, hz;
    if (!HitCellOf(j, points, ray, &hx, &hy, &hz)) continue;
    if (kFinish && sub == 0) {
      ++visited;
      updated += FinishCell(j, hx, hy, hz, ptab);
    }
    const Span3 s = MakeSpan(j.cx, j.cy, j.cz, hx, hy, hz, free_voxels);
    if (s.num_samples >= kMaxSamples) continue;  // the host refuses these
    for (int position = s.first + sub; position < s.num_samples; position += group) {
      int x, y, z;
      SpanCell(j.cx, j.cy, j.cz, s, position, &x, &y, &z);
      if (kFinish) {
        ++visited;
        updated += FinishCell(j, x, y, z, ptab);
      } else {
        ApplyCell(j, x, y, z, tabs + 32768);
      }
    }
  }
  if (kFinish) {
    // One atomic pair per wave.
    for (int o = 32; o > 0; o >>= 1) {
      visited += __shfl_xor(visited, o);
      updated += __shfl_xor(updated, o);
    }
    if ((threadIdx.x & 63) == 0 && visited) {
      atomicAdd(j.stats, static_cast<unsigned long long>(visited));
      if (updated) atomicAdd(j.stats + 1, static_cast<unsigned long long>(updated));
    }
  }
}

// A: uint16 values, B: float probabilities (HybridGrid); A: float sums,
// B: int32 counts (IntensityHybridGrid).
template <typename A, typename B>
__global__ void __launch_bounds__(256)
insert3d_grow(const A* __restrict__ old_values, const B* __restrict__ old_prob, Brick3 ob,
              A* __restrict__ values, B* __restrict__ prob, Brick3 nb, B unknown) {
  const int64_t total = static_cast<int64_t>(nb.nx) * nb.ny * nb.nz;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int x = static_cast<int>(i % nb.nx) + nb.ox;
    const int y = static_cast<int>(i / nb.nx % nb.ny) + nb.oy;
    const int z = static_cast<int>(i / nb.nx / nb.ny) + nb.oz;
    const int64_t k = BrickIndex(ob, x, y, z);
    values[i] = k < 0 ? A{0} : old_values[k];
    prob[i] = k < 0 ? unknown : old_prob[k];
  }
}

// The intensity half of a job: the Job3 gives the returns, their transform
// and the range filter; the cell is the intensity grid's own GetCellIndex.
struct IJob3 {
  float* sum;
  int32_t* count;
  Brick3 b;
  float resolution;
  float threshold;
  int job;       // the Job3, as an index into the call's descriptors
  int64_t slot;  // the job's first pair in the launch set's key array
};

__global__ void __launch_bounds__(256)
insert3d_intensity_keys(const IJob3* __restrict__ ijobs, const Job3* __restrict__ jobs,
                        const float* __restrict__ points, const float* __restrict__ intensities,
                        uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const IJob3 ij = ijobs[blockIdx.y];
  const Job3 j = jobs[ij.job];
  const uint64_t none = static_cast<uint64_t>(gridDim.y) << 32;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < j.num_returns;
       i += gridDim.x * blockDim.x) {
    uint64_t key = none;
    float p[3];
    if (JobPoint(j, points + 3 * (j.begin + i), p) &&
        !(intensities[j.begin + i] > ij.threshold)) {
      const int64_t c = BrickIndex(ij.b, static_cast<int>(CellF(p[0], ij.resolution)),
                                   static_cast<int>(CellF(p[1], ij.resolution)),
                                   static_cast<int>(CellF(p[2], ij.resolution)));
      // The host sized the brick from these very cells; a cell outside it is
      // dropped, never written.
      if (c >= 0) key = static_cast<uint64_t>(blockIdx.y) << 32 | static_cast<uint64_t>(c);
    }
    keys[ij.slot + i] = key;
    vals[ij.slot + i] = static_cast<uint32_t>(i);
  }
}

// keys sorted, n of them, `none` and above are not cells. Jobs of a launch
// set write different grids and one thread owns a (job, cell) run, so the
// plain stores do not race.
__global__ void __launch_bounds__(256)
insert3d_intensity_sums(const IJob3* __restrict__ ijobs, const Job3* __restrict__ jobs,
                        const float* __restrict__ intensities,
                        const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                        int64_t n, uint64_t none) {
  __shared__ uint64_t tile[257];  // the key before the block's first, then the block's
  const int64_t base = static_cast<int64_t>(blockIdx.x) * 256;
  const int64_t s = base + threadIdx.x;
  tile[threadIdx.x + 1] = s < n ? keys[s] : none;
  if (threadIdx.x == 0) tile[0] = base > 0 ? keys[base - 1] : none;
  __syncthreads();
  const uint64_t key = tile[threadIdx.x + 1];
  if (key >= none || key == tile[threadIdx.x]) return;  // not the head of a run
  const IJob3 ij = ijobs[key >> 32];
  const float* __restrict__ v = intensities + jobs[ij.job].begin;
  const int64_t cell = static_cast<int64_t>(key & 0xffffffffu);
  float sum = ij.sum[cell];
  int32_t count = 0;
  for (int64_t t = s;;) {
    sum = __fadd_rn(sum, v[vals[t]]);
    ++count;
    if (++t >= n) break;
    const uint64_t next = t - base < 256 ? tile[t - base + 1] : keys[t];
    if (next != key) break;
  }
  ij.sum[cell] = sum;
  ij.count[cell] += count;
}

// IntensityHybridGrid::GetIntensity (hybrid_grid.h:563-570).
__global__ void intensity_grid_lookup(const float* __restrict__ sum,
                                      const int32_t* __restrict__ count, Brick3 b,
                                      const int32_t* __restrict__ ijk, int64_t n,
                                      float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t k = BrickIndex(b, ijk[3 * i], ijk[3 * i + 1], ijk[3 * i + 2]);
  const int32_t c = k < 0 ? 0 : count[k];
  out[i] = c == 0 ? 0.f : __fdiv_rn(sum[k], static_cast<float>(c));
}

// ---------------------------------------------------------------- host -----

// probability_values.h:32-45, :37-43 and common/math.h Clamp, in float.
constexpr float kMinP = 0.1f, kMaxP = 1.f - kMinP;
uint16_t ProbabilityToValue(float p) {
  const float c = p > kMaxP ? kMaxP : (p < kMinP ? kMinP : p);
  return static_cast<uint16_t>(
      static_cast<int>(std::lround((c - kMinP) * (32766.f / (kMaxP - kMinP)))) + 1);
}

// ComputeLookupTableToApplyOdds (probability_values.cc:76-87).
void LookupTable3(float odds, uint16_t* out) {
  std::vector<float> ptab(32768);
  ConversionTable(kMinP, kMinP, kMaxP, ptab.data());  // kValueToProbability (:26-66)
  constexpr uint16_t kUpdateMarker = 1u << 15;
  out[0] = ProbabilityToValue(ProbabilityFromOdds(odds)) + kUpdateMarker;
  for (int cell = 1; cell < 32768; ++cell)
    out[cell] = ProbabilityToValue(ProbabilityFromOdds(odds * Odds(ptab[cell]))) + kUpdateMarker;
}

int EnsureTables3(csm_context* ctx, const csm_inserter3d_options* o) {
  int rc;
  if (!ctx->ins3_ptab.ptr) {
    // kValueToProbability, the table csm_hybrid_grid_create fills the
    // probability brick from.
    std::vector<float> ptab(32768);
    ConversionTable(kMinP, kMinP, kMaxP, ptab.data());
    if ((rc = ctx->ins3_ptab.Reserve(sizeof(float) * 32768))) return rc;
    CSM_HIP(hipMemcpy(ctx->ins3_ptab.ptr, ptab.data(), sizeof(float) * 32768,
                      hipMemcpyHostToDevice));
  }
  return EnsureOddsTables(ctx, o->hit_probability, o->miss_probability, LookupTable3,
                          &ctx->ins3_tabs, ctx->ins3_tab_key);
}

// Bytes of a value brick of n cells: the kernels address it in 32-bit words.
size_t ValueBytes(int64_t n) {
  return static_cast<size_t>((n + 1) & ~int64_t{1}) * sizeof(uint16_t);
}

struct Box3 {
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  bool empty() const { return hi[0] < lo[0]; }
  void Add(int x, int y, int z) {
    const int c[3] = {x, y, z};
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], c[a]);
      hi[a] = std::max(hi[a], c[a]);
    }
  }
  void Add(const Box3& o) {
    if (o.empty()) return;
    Add(o.lo[0], o.lo[1], o.lo[2]);
    Add(o.hi[0], o.hi[1], o.hi[2]);
  }
};

// GetCellIndex on the host without a libm call per axis: truncate, then step
// away from zero when the remainder reaches a half (the subtraction is exact).
// False when the quotient is past kMaxCell.
bool HostCell(float v, float resolution, int* out) {
  const float q = v / resolution;
  if (!(std::fabs(q) < kMaxCell)) return false;
  int t = static_cast<int>(q);
  const float d = q - static_cast<float>(t);
  if (d >= 0.5f) ++t;
  else if (d <= -0.5f) --t;
  *out = t;
  return true;
}

// A chunk of one job's returns for the planning pass.
constexpr int kPlanChunk = 8192;
struct PlanTask {
  int job, i0, i1;
  Box3 box;
  int rc;
  Box3 ibox;  // the cells of the job's intensity grid that gain a return
};

// The box of the cells returns [i0, i1) of job j touch: per ray the hit cell
// and the first miss cell. CSM_ERANGE for a ray the reference would
// CHECK-fail on or a coordinate past the index arithmetic.
int PlanReturns(const Job3& j, const float* returns, int i0, int i1, int free_voxels, Box3* box) {
  for (int i = i0; i < i1; ++i) {
    float p[3];
    if (!JobPoint(j, returns + 3 * (j.begin + i), p)) continue;
    int hx, hy, hz;
    if (!HostCell(p[0], j.resolution, &hx) || !HostCell(p[1], j.resolution, &hy) ||
        !HostCell(p[2], j.resolution, &hz))
      return CSM_ERANGE;
    const Span3 sp = MakeSpan(j.cx, j.cy, j.cz, hx, hy, hz, free_voxels);
    if (sp.num_samples >= kMaxSamples) return CSM_ERANGE;
    box->Add(hx, hy, hz);
    if (sp.first < sp.num_samples) {
      int x, y, z;
      SpanCell(j.cx, j.cy, j.cz, sp, sp.first, &x, &y, &z);
      box->Add(x, y, z);
    }
  }
  return CSM_OK;
}

// The intensity half of a call (csm_hybrid_grid_insert_intensities*); null
// for the entry points without one.
struct Intens3 {
  csm_intensity_grid* const* grids;
  int32_t num_grids;
  const int32_t* grid_of_job;            // -1: the job has none
  const float* const* scan_intensities;  // per scan, null: the scan has none
  float threshold;
};

// The box of the cells of job j's intensity grid that returns [i0, i1) add to
// (InsertIntensitiesIntoGrid, :76-89).
int PlanIntensities(const Job3& j, const float* returns, const float* intensities, float resolution,
                    float threshold, int i0, int i1, Box3* box) {
  for (int i = i0; i < i1; ++i) {
    float p[3];
    if (intensities[i] > threshold || !JobPoint(j, returns + 3 * (j.begin + i), p)) continue;
    int x, y, z;
    if (!HostCell(p[0], resolution, &x) || !HostCell(p[1], resolution, &y) ||
        !HostCell(p[2], resolution, &z))
      return CSM_ERANGE;
    box->Add(x, y, z);
  }
  return CSM_OK;
}

// DynamicGrid::Grow (hybrid_grid.h:283-296, :384-399) and the brick over the
// old box united with `box`. CSM_ERANGE past 2^31 cells.
int GrownBrick(const Brick3& b, const Box3& box, Brick3* after, int* grid_size) {
  const bool had = b.nx > 0;
  const int olo[3] = {b.ox, b.oy, b.oz};
  const int ohi[3] = {b.ox + b.nx - 1, b.oy + b.ny - 1, b.oz + b.nz - 1};
  int lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = had ? std::min(olo[a], box.lo[a]) : box.lo[a];
    hi[a] = had ? std::max(ohi[a], box.hi[a]) : box.hi[a];
    while (box.lo[a] < -(*grid_size / 2) || box.hi[a] >= *grid_size / 2) *grid_size *= 2;
  }
  *after = Brick3{lo[0], lo[1], lo[2], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1, 0};
  const int64_t n = static_cast<int64_t>(after->nx) * after->ny * after->nz;
  return n > (int64_t{1} << 31) ? CSM_ERANGE : CSM_OK;
}

// The intensity jobs of one keys / sort / sums launch set.
struct IntensSet3 {
  int round, first, num;
  int64_t pairs;    // the jobs' returns: one pair each
  int max_returns;
  int end_bit = 0;  // of the key: 32 bits of cell, then the job and `none`
};

// What a call does to one grid of either kind: a csm_hybrid_grid (a: values,
// b: prob) or a csm_intensity_grid (a: sum, b: count).
struct BrickPlan3 {
  Box3 box;        // the cells this call touches
  Brick3 after{};  // the brick once the call is done
  int grid_size = 0;
  bool touched = false, grew = false;
  DevBuf a, b;  // a grown grid's new bricks
  int64_t cells() const { return static_cast<int64_t>(after.nx) * after.ny * after.nz; }
};

// The grid's brick and DynamicGrid size after the call, from p->box.
template <typename Grid>
int PlanBrick(const Grid* g, BrickPlan3* p) {
  p->after = g->brick;
  p->grid_size = g->grid_size;
  p->touched = !p->box.empty();
  if (!p->touched) return CSM_OK;
  if (GrownBrick(g->brick, p->box, &p->after, &p->grid_size) != CSM_OK) return CSM_ERANGE;
  p->grew = p->after.nx != g->brick.nx || p->after.ny != g->brick.ny || p->after.nz != g->brick.nz;
  return CSM_OK;
}

// A grown grid's new bricks, and the event consumers on other streams wait on.
int ReserveBrick(csm_context* ctx, BrickPlan3* p, size_t bytes_a, size_t bytes_b,
                 hipEvent_t* ready) {
  if (!*ready) CSM_HIP(hipEventCreateWithFlags(ready, hipEventDisableTiming));
  if (!p->grew) return CSM_OK;
  const int rc = ctx->pool.Take(bytes_a, &p->a);
  return rc != CSM_OK ? rc : ctx->pool.Take(bytes_b, &p->b);
}

void GiveBackBricks(csm_context* ctx, std::vector<BrickPlan3>* plan) {
  for (BrickPlan3& p : *plan) {
    ctx->pool.Give(&p.a);
    ctx->pool.Give(&p.b);
  }
}

// Enqueues a touched grid's growth (the old cells at their offset, `unknown`
// in b elsewhere), swaps the new bricks in and moves the grid's host state on.
template <typename A, typename B, typename Grid>
int CommitBrick(csm_context* ctx, Grid* g, DevBuf Grid::*a, DevBuf Grid::*b, B unknown,
                BrickPlan3* p, std::deque<DevBuf>* retired) {
  if (p->grew) {
    hipLaunchKernelGGL(insert3d_grow, dim3(Blocks(p->cells(), 1024, 8192)), dim3(256), 0,
                       ctx->stream, (g->*a).template as<A>(), (g->*b).template as<B>(), g->brick,
                       p->a.as<A>(), p->b.as<B>(), p->after, unknown);
    CSM_HIP(hipGetLastError());
    retired->push_back(std::move(g->*a));
    retired->push_back(std::move(g->*b));
    g->*a = std::move(p->a);
    g->*b = std::move(p->b);
  }
  g->brick = p->after;
  g->grid_size = p->grid_size;
  ++g->generation;
  return CSM_OK;
}

int InsertBatch3(csm_context* ctx, csm_hybrid_grid* const* grids, int32_t num_grids,
                 const csm_inserter3d_options* o, int32_t num_scans, const float* origins,
                 const float* returns, const int64_t* ret_off, int32_t num_jobs,
                 const int32_t* grid_of_job, const int32_t* scan_of_job, const float* transforms,
                 int32_t num_transforms, const int32_t* transform_of_job,
                 const float* max_ranges, bool ctx_of_grid, const Intens3* in = nullptr) {
  if ((!ctx && !ctx_of_grid) || !grids || !o || num_grids < 1 || num_scans < 0 || num_jobs < 0 ||
      num_transforms < 0)
    return CSM_EINVAL;
  if (num_scans > 0 && (!origins || !ret_off)) return CSM_EINVAL;
  if (num_jobs > 0 && (!grid_of_job || !scan_of_job)) return CSM_EINVAL;
  if (num_transforms > 0 && !transforms) return CSM_EINVAL;
  if (!(o->hit_probability > 0.f && o->hit_probability < 1.f && o->miss_probability > 0.f &&
        o->miss_probability < 1.f) ||
      o->num_free_space_voxels < 0)
    return CSM_EINVAL;
  for (int g = 0; g < num_grids; ++g)
    if (!grids[g]) return CSM_EINVAL;
  if (num_jobs == 0) return CSM_OK;
  if (num_scans == 0 || !ValidScans(num_scans, origins, ret_off, returns)) return CSM_EINVAL;
  const int64_t total_ret = ret_off[num_scans];
  for (int64_t i = 0; i < int64_t{7} * num_transforms; ++i)
    if (!std::isfinite(transforms[i])) return CSM_EINVAL;
  for (int k = 0; k < num_jobs; ++k) {
    if (grid_of_job[k] < 0 || grid_of_job[k] >= num_grids || scan_of_job[k] < 0 ||
        scan_of_job[k] >= num_scans)
      return CSM_EINVAL;
    if (transform_of_job && transform_of_job[k] >= num_transforms) return CSM_EINVAL;
    if (max_ranges && std::isnan(max_ranges[k])) return CSM_EINVAL;
  }
  // ipair[i]: the HybridGrid intensity grid i is filled with. Its jobs run in
  // that grid's rounds, so one call pairs it with one HybridGrid only.
  std::vector<int> ipair;
  if (in) {
    if (in->num_grids < 0 || (in->num_grids > 0 && !in->grids) || std::isnan(in->threshold))
      return CSM_EINVAL;
    for (int g = 0; g < in->num_grids; ++g)
      if (!in->grids[g]) return CSM_EINVAL;
    for (int s = 0; s < num_scans && in->scan_intensities; ++s) {
      const float* v = in->scan_intensities[s];
      for (int64_t i = 0, n = ret_off[s + 1] - ret_off[s]; v && i < n; ++i)
        if (!std::isfinite(v[i])) return CSM_EINVAL;
    }
    ipair.assign(in->num_grids, -1);
    for (int k = 0; k < num_jobs && in->grid_of_job; ++k) {
      const int ig = in->grid_of_job[k];
      if (ig < 0) continue;
      if (ig >= in->num_grids) return CSM_EINVAL;
      if (ipair[ig] >= 0 && ipair[ig] != grid_of_job[k]) return CSM_EINVAL;
      ipair[ig] = grid_of_job[k];
    }
  }
  // The points are checked before any handle is read.
  if (ctx_of_grid) ctx = grids[0]->ctx;
  if (!ctx) return CSM_EINVAL;
  if (!ValidHandles(ctx, grids, num_grids) || (in && !ValidHandles(ctx, in->grids, in->num_grids)))
    return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;

  // Plan on the host, before any launch: every job's origin cell and the box
  // of the cells it touches. Per ray the first miss cell and the hit cell
  // bound the span (each axis is monotone in `position`), and every touched
  // cell ends nonzero (table[0] is nonzero), so the known-cell box afterwards
  // is the old box united with the touched one.
  const int free_voxels = o->num_free_space_voxels;
  std::vector<Job3> jobs(num_jobs);
  std::vector<BrickPlan3> plan(num_grids), iplan(in ? in->num_grids : 0);
  std::vector<DevBuf> stats(num_grids);  // the first insert's counters
  std::vector<int> rounds(num_grids, 0);
  std::vector<int> round_of(num_jobs);
  std::vector<PlanTask> tasks;
  // The job's intensity grid, -1 where it has none or its scan carries no
  // intensities (:79), and that scan's intensities.
  std::vector<int> igrid_of(num_jobs, -1);
  auto intensities_of = [&](int k) { return in->scan_intensities[scan_of_job[k]]; };
  for (int k = 0; in && in->grid_of_job && in->scan_intensities && k < num_jobs; ++k)
    if (in->grid_of_job[k] >= 0 && intensities_of(k)) igrid_of[k] = in->grid_of_job[k];
  int64_t planned = 0;
  int num_rounds = 0;
  for (int k = 0; k < num_jobs; ++k) {
    Job3& j = jobs[k];
    csm_hybrid_grid* g = grids[grid_of_job[k]];
    round_of[k] = rounds[grid_of_job[k]]++;
    num_rounds = std::max(num_rounds, round_of[k] + 1);
    const int s = scan_of_job[k];
    j.resolution = g->resolution;
    j.has_transform = transform_of_job && transform_of_job[k] >= 0;
    float org[3] = {origins[3 * s], origins[3 * s + 1], origins[3 * s + 2]};
    if (j.has_transform) {
      const float* tf = transforms + 7 * transform_of_job[k];
      for (int a = 0; a < 3; ++a) j.t[a] = tf[a];
      for (int a = 0; a < 4; ++a) j.q[a] = tf[3 + a];
      Apply3(j.t, j.q, org);
    } else {
      j.t[0] = j.t[1] = j.t[2] = 0.f;
      j.q[0] = 1.f;
      j.q[1] = j.q[2] = j.q[3] = 0.f;
    }
    j.ox = org[0];
    j.oy = org[1];
    j.oz = org[2];
    j.max_range = max_ranges ? max_ranges[k] : 0.f;
    j.begin = ret_off[s];
    j.num_returns = static_cast<int>(ret_off[s + 1] - ret_off[s]);
    if (!HostCell(org[0], j.resolution, &j.cx) || !HostCell(org[1], j.resolution, &j.cy) ||
        !HostCell(org[2], j.resolution, &j.cz))
      return CSM_ERANGE;
    for (int i0 = 0; i0 < j.num_returns; i0 += kPlanChunk)
      tasks.push_back(
          PlanTask{k, i0, std::min(j.num_returns, i0 + kPlanChunk), Box3{}, CSM_OK, Box3{}});
    planned += j.num_returns;
  }
  // Large scans are planned on a few threads, a chunk of returns at a time.
  RunPlanTasks(tasks.size(), planned, [&](size_t t) {
    PlanTask& task = tasks[t];
    // The boxes grow in locals and are stored once: neighbouring tasks
    // share cache lines, and a store per return from every thread made
    // the 55 000-return plan two to three times slower.
    Box3 box, ibox;
    int rc = PlanReturns(jobs[task.job], returns, task.i0, task.i1, free_voxels, &box);
    const int ig = igrid_of[task.job];
    if (rc == CSM_OK && ig >= 0)
      rc = PlanIntensities(jobs[task.job], returns, intensities_of(task.job),
                           in->grids[ig]->resolution, in->threshold, task.i0, task.i1, &ibox);
    task.box = box;
    task.ibox = ibox;
    task.rc = rc;
  });
  for (const PlanTask& task : tasks) {
    if (task.rc != CSM_OK) return task.rc;
    plan[grid_of_job[task.job]].box.Add(task.box);
    if (!task.ibox.empty()) iplan[igrid_of[task.job]].box.Add(task.ibox);
  }
  for (size_t gi = 0; gi < iplan.size(); ++gi)
    if (PlanBrick(in->grids[gi], &iplan[gi])) return CSM_ERANGE;
  for (int gi = 0; gi < num_grids; ++gi) {
    BrickPlan3& p = plan[gi];
    if (PlanBrick(grids[gi], &p)) return CSM_ERANGE;
    // A brick csm_hybrid_grid_create sized to an odd cell count is moved once
    // so that its last cell has a whole word.
    if (p.touched && grids[gi]->values.bytes < ValueBytes(p.cells())) p.grew = true;
  }

  // Allocate before anything is enqueued: a failure leaves the grids as they
  // were.
  int rc = EnsureTables3(ctx, o);
  auto give_back = [&] {
    GiveBackBricks(ctx, &plan);
    GiveBackBricks(ctx, &iplan);
    for (DevBuf& b : stats) ctx->pool.Give(&b);
  };
  for (int gi = 0; gi < num_grids && rc == CSM_OK; ++gi) {
    BrickPlan3& p = plan[gi];
    if (!p.touched) continue;
    if (!grids[gi]->insert_stats.ptr)
      rc = ctx->pool.Take(2 * sizeof(unsigned long long), &stats[gi]);
    if (rc == CSM_OK)
      rc = ReserveBrick(ctx, &p, ValueBytes(p.cells()), sizeof(float) * p.cells(),
                        &grids[gi]->ready);
  }
  // Jobs in round order (stable), then one upload: descriptors and returns.
  std::vector<int> order;
  for (int k = 0; k < num_jobs; ++k)
    if (jobs[k].num_returns > 0) order.push_back(k);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return round_of[a] < round_of[b]; });
  const int live = static_cast<int>(order.size());
  const size_t desc_bytes = Align(sizeof(Job3) * std::max(live, 1));
  size_t bytes = desc_bytes + sizeof(float) * 3 * total_ret;
  // The intensity halves, in the same order: a launch set is the jobs of one
  // round (at most gridDim.y of them) whose intensity grid gains a return.
  std::vector<IJob3> ijobs;
  std::vector<IntensSet3> isets;
  for (int i = 0; i < live; ++i) {
    const int k = order[i], ig = igrid_of[k];
    if (ig < 0 || !iplan[ig].touched) continue;
    if (isets.empty() || isets.back().round != round_of[k] || isets.back().num == 65535)
      isets.push_back(IntensSet3{round_of[k], static_cast<int>(ijobs.size()), 0, 0, 1});
    IntensSet3& set = isets.back();
    IJob3 ij{};
    ij.resolution = in->grids[ig]->resolution;
    ij.threshold = in->threshold;
    ij.job = i;
    ij.slot = set.pairs;
    ijobs.push_back(ij);
    ++set.num;
    set.pairs += jobs[k].num_returns;
    set.max_returns = std::max(set.max_returns, jobs[k].num_returns);
  }
  size_t idesc_at = 0, ival_at = 0, sort_bytes = 0, pair_cap = 0, scratch_bytes = 256;
  if (!ijobs.empty()) {
    idesc_at = Align(bytes);
    ival_at = idesc_at + Align(sizeof(IJob3) * ijobs.size());
    bytes = ival_at + sizeof(float) * total_ret;
    for (IntensSet3& set : isets) {
      if (set.pairs >= (int64_t{1} << 31)) rc = CSM_ERANGE;  // the sort counts in 32 bits
      set.end_bit = 33;
      while ((1u << (set.end_bit - 32)) <= static_cast<unsigned>(set.num)) ++set.end_bit;
      size_t need = 0;
      if (rc == CSM_OK &&
          rocprim::radix_sort_pairs(nullptr, need, static_cast<uint64_t*>(nullptr),
                                    static_cast<uint64_t*>(nullptr),
                                    static_cast<uint32_t*>(nullptr),
                                    static_cast<uint32_t*>(nullptr),
                                    static_cast<unsigned>(set.pairs), 0u,
                                    static_cast<unsigned>(set.end_bit), ctx->stream) != hipSuccess)
        rc = CSM_EHIP;
      scratch_bytes = std::max(scratch_bytes, need);
      pair_cap = std::max(pair_cap, static_cast<size_t>(set.pairs));
    }
    // keys, sorted keys, indices, sorted indices, scratch.
    sort_bytes = 2 * Align(8 * pair_cap) + 2 * Align(4 * pair_cap) + Align(scratch_bytes);
  }
  for (size_t gi = 0; gi < iplan.size() && rc == CSM_OK; ++gi) {
    BrickPlan3& p = iplan[gi];
    if (p.touched)
      rc = ReserveBrick(ctx, &p, sizeof(float) * p.cells(), sizeof(int32_t) * p.cells(),
                        &in->grids[gi]->ready);
  }
  if (rc == CSM_OK && ctx->ins3_sort.bytes < sort_bytes) {
    // As ins3_dev below: an earlier insert may still sort in it.
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = CSM_EHIP;
    else rc = ctx->ins3_sort.Reserve(sort_bytes + sort_bytes / 2);
  }
  StageRing::Slot* slot = nullptr;
  if (rc == CSM_OK && live > 0)
    rc = ReserveUpload(ctx, &ctx->ins3_stage, &ctx->ins3_dev, bytes, &slot);
  if (rc != CSM_OK) {
    give_back();
    return rc;
  }
  hipStream_t st = ctx->stream;
  // From here on a failure is a HIP error (insert_host.h).
  std::deque<DevBuf> retired;
  for (int gi = 0; gi < num_grids; ++gi) {
    csm_hybrid_grid* g = grids[gi];
    if (!plan[gi].touched) continue;
    if (stats[gi].ptr) {
      CSM_HIP(hipMemsetAsync(stats[gi].ptr, 0, 2 * sizeof(unsigned long long), st));
      g->insert_stats = std::move(stats[gi]);
    }
    if ((rc = CommitBrick<uint16_t>(ctx, g, &csm_hybrid_grid::values, &csm_hybrid_grid::prob,
                                    kMinP, &plan[gi], &retired)))
      return rc;
  }
  for (size_t gi = 0; gi < iplan.size(); ++gi)
    if (iplan[gi].touched &&
        (rc = CommitBrick<float>(ctx, in->grids[gi], &csm_intensity_grid::sum,
                                 &csm_intensity_grid::count, int32_t{0}, &iplan[gi], &retired)))
      return rc;
  if (live > 0) {
    Job3* hd = slot->buf.as<Job3>();
    for (int i = 0; i < live; ++i) {
      Job3& j = jobs[order[i]];
      csm_hybrid_grid* g = grids[grid_of_job[order[i]]];
      j.words = g->values.as<uint32_t>();
      j.prob = g->prob.as<float>();
      j.stats = g->insert_stats.as<unsigned long long>();
      j.b = g->brick;
      hd[i] = j;
    }
    if (total_ret)
      std::memcpy(slot->buf.as<char>() + desc_bytes, returns, sizeof(float) * 3 * total_ret);
    if (!ijobs.empty()) {
      for (IJob3& ij : ijobs) {
        const int k = order[ij.job];
        const csm_intensity_grid* g = in->grids[igrid_of[k]];
        ij.sum = g->sum.as<float>();
        ij.count = g->count.as<int32_t>();
        ij.b = g->brick;
        // The scan's intensities lie where its returns do.
        std::memcpy(slot->buf.as<char>() + ival_at + sizeof(float) * jobs[k].begin,
                    intensities_of(k), sizeof(float) * jobs[k].num_returns);
      }
      std::memcpy(slot->buf.as<char>() + idesc_at, ijobs.data(), sizeof(IJob3) * ijobs.size());
    }
    if ((rc = Upload(ctx, slot, &ctx->ins3_dev, bytes))) return rc;
    const Job3* dd = ctx->ins3_dev.as<Job3>();
    const float* dpts = reinterpret_cast<const float*>(ctx->ins3_dev.as<char>() + desc_bytes);
    const uint16_t* tabs = ctx->ins3_tabs.as<uint16_t>();
    const float* ptab = ctx->ins3_ptab.as<float>();
    // Lanes per ray: the power of two at or above the span length, at most a
    // wave.
    int group_bits = 0;
    while (group_bits < 6 && (1 << group_bits) < free_voxels) ++group_bits;
    const int rays_per_block = 256 >> group_bits;
    const IJob3* dij = reinterpret_cast<const IJob3*>(ctx->ins3_dev.as<char>() + idesc_at);
    const float* dval = reinterpret_cast<const float*>(ctx->ins3_dev.as<char>() + ival_at);
    char* sort_at = ctx->ins3_sort.as<char>();
    uint64_t* keys = reinterpret_cast<uint64_t*>(sort_at);
    uint64_t* sorted_keys = reinterpret_cast<uint64_t*>(sort_at + Align(8 * pair_cap));
    uint32_t* vals = reinterpret_cast<uint32_t*>(sort_at + 2 * Align(8 * pair_cap));
    uint32_t* sorted_vals = vals + Align(4 * pair_cap) / sizeof(uint32_t);
    void* scratch = sorted_vals + Align(4 * pair_cap) / sizeof(uint32_t);
    size_t next_set = 0;
    int i0 = 0;
    for (int r = 0; r < num_rounds && i0 < live; ++r) {
      int i1 = i0;
      int64_t max_returns = 1;
      for (; i1 < live && round_of[order[i1]] == r; ++i1)
        max_returns = std::max<int64_t>(max_returns, jobs[order[i1]].num_returns);
      const unsigned ny = static_cast<unsigned>(i1 - i0);
      for (unsigned y0 = 0; y0 < ny; y0 += 65535) {  // gridDim.y
        const unsigned nyy = std::min(65535u, ny - y0);
        const dim3 ray_blocks(Blocks(max_returns, rays_per_block, 4096), nyy);
        hipLaunchKernelGGL(insert3d_hits, dim3(Blocks(max_returns, 256, 1024), nyy), dim3(256), 0,
                           st, dd + i0 + y0, dpts, tabs);
        CSM_HIP(hipGetLastError());
        if (free_voxels > 0) {
          hipLaunchKernelGGL(insert3d_rays<false>, ray_blocks, dim3(256), 0, st, dd + i0 + y0,
                             dpts, tabs, ptab, free_voxels, group_bits);
          CSM_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(insert3d_rays<true>, ray_blocks, dim3(256), 0, st, dd + i0 + y0, dpts,
                           tabs, ptab, free_voxels, group_bits);
        CSM_HIP(hipGetLastError());
      }
      for (; next_set < isets.size() && isets[next_set].round == r; ++next_set) {
        const IntensSet3& set = isets[next_set];
        const IJob3* dset = dij + set.first;
        hipLaunchKernelGGL(insert3d_intensity_keys,
                           dim3(Blocks(set.max_returns, 256, 1024), set.num), dim3(256), 0, st,
                           dset, dd, dpts, dval, keys, vals);
        CSM_HIP(hipGetLastError());
        size_t scratch_size = scratch_bytes;
        CSM_HIP(rocprim::radix_sort_pairs(scratch, scratch_size, keys, sorted_keys, vals,
                                          sorted_vals, static_cast<unsigned>(set.pairs), 0u,
                                          static_cast<unsigned>(set.end_bit), st));
        hipLaunchKernelGGL(insert3d_intensity_sums,
                           dim3(static_cast<unsigned>((set.pairs + 255) / 256)), dim3(256), 0, st,
                           dset, dd, dval, sorted_keys, sorted_vals, set.pairs,
                           static_cast<uint64_t>(set.num) << 32);
        CSM_HIP(hipGetLastError());
      }
      i0 = i1;
    }
  }
  // Consumers on other streams wait for the last insert.
  for (int gi = 0; gi < num_grids; ++gi)
    if (plan[gi].touched) CSM_HIP(hipEventRecord(grids[gi]->ready, st));
  for (size_t gi = 0; gi < iplan.size(); ++gi)
    if (iplan[gi].touched) CSM_HIP(hipEventRecord(in->grids[gi]->ready, st));
  // The old bricks of grown grids: reused by later takes on this stream.
  for (DevBuf& b : retired) ctx->pool.Give(&b);
  return CSM_OK;
}

}  // namespace
}  // namespace csm

using namespace csm;

// RotationalScanMatcher::ComputeHistogram's host steps
// (rotational_scan_matcher.cc:34-117), float arithmetic in the reference's order.
namespace csm {
namespace {

constexpr float kHistMinDistance = 0.2f, kHistMaxDistance = 0.9f, kHistSliceHeight = 0.2f;

struct HistPoint {
  float x, y, z;
};
using HistSlice = std::vector<HistPoint>;

int HistRoundToInt(float v) { return static_cast<int>(std::lround(v)); }
float HistNorm2(float x, float y) { return std::sqrt(x * x + y * y); }

// AddValueToHistogram (:34-49).
void HistAddValue(float angle, float value, int size, float* histogram) {
  const float pi = static_cast<float>(M_PI);
  while (angle > pi) angle -= pi;
  while (angle < 0.f) angle += pi;
  const float zero_to_one = angle / pi;
  const int bucket = std::min(
      std::max(HistRoundToInt(static_cast<float>(size) * zero_to_one - 0.5f), 0), size - 1);
  histogram[bucket] += value;
}

// ComputeCentroid (:51-58): the sum in point order, then one division each.
HistPoint HistCentroid(const HistSlice& slice) {
  HistPoint sum{0.f, 0.f, 0.f};
  for (const HistPoint& p : slice) {
    sum.x += p.x;
    sum.y += p.y;
    sum.z += p.z;
  }
  const float n = static_cast<float>(slice.size());
  return HistPoint{sum.x / n, sum.y / n, sum.z / n};
}

// SortSlice (:92-117): by the angle about the centroid, points near it dropped.
HistSlice HistSortSlice(const HistSlice& slice) {
  struct ByAngle {
    bool operator<(const ByAngle& other) const { return angle < other.angle; }
    float angle;
    HistPoint point;
  };
  const HistPoint centroid = HistCentroid(slice);
  std::vector<ByAngle> by_angle;
  by_angle.reserve(slice.size());
  for (const HistPoint& p : slice) {
    const float dx = p.x - centroid.x, dy = p.y - centroid.y;
    if (HistNorm2(dx, dy) < kHistMinDistance) continue;
    by_angle.push_back(ByAngle{std::atan2(dy, dx), p});
  }
  std::sort(by_angle.begin(), by_angle.end());
  HistSlice sorted;
  sorted.reserve(by_angle.size());
  for (const ByAngle& e : by_angle) sorted.push_back(e.point);
  return sorted;
}

// AddPointCloudSliceToHistogram (:60-88).
void HistAddSlice(const HistSlice& slice, int size, float* histogram) {
  if (slice.empty()) return;
  const HistPoint centroid = HistCentroid(slice);
  HistPoint last = slice.front();
  for (const HistPoint& p : slice) {
    const float dx = p.x - last.x, dy = p.y - last.y;
    const float cx = p.x - centroid.x, cy = p.y - centroid.y;
    const float distance = HistNorm2(dx, dy);
    if (distance < kHistMinDistance || HistNorm2(cx, cy) < kHistMinDistance) continue;
    if (distance > kHistMaxDistance) {
      last = p;
      continue;
    }
    const float angle = std::atan2(dy, dx);
    const float dn = HistNorm2(dx, dy), cn = HistNorm2(cx, cy);
    const float dot = (dx / dn) * (cx / cn) + (dy / dn) * (cy / cn);
    HistAddValue(angle, std::max(0.f, 1.f - std::abs(dot)), size, histogram);
  }
}

}  // namespace
}  // namespace csm

extern "C" {

int csm_inserter3d_lookup_table(float probability, uint16_t* out) {
  if (!out || !(probability > 0.f && probability < 1.f)) return CSM_EINVAL;
  LookupTable3(Odds(probability), out);
  return CSM_OK;
}

int csm_rotate_histogram(const float* histogram, int32_t size, float angle, float* out) {
  if (size < 0 || (size > 0 && (!histogram || !out)) || !std::isfinite(angle)) return CSM_EINVAL;
  if (size == 0) return CSM_OK;
  const float rotate_by_buckets =
      static_cast<float>(static_cast<double>(-angle * static_cast<float>(size)) / M_PI);
  if (!(std::fabs(rotate_by_buckets) < 1.0e9f)) return CSM_ERANGE;
  int full_buckets = static_cast<int>(std::lround(rotate_by_buckets - 0.5f));
  const float fraction = rotate_by_buckets - static_cast<float>(full_buckets);
  full_buckets %= size;  // `while (full_buckets < 0) full_buckets += size`, then % size below
  if (full_buckets < 0) full_buckets += size;
  std::vector<float> in(histogram, histogram + size);  // out may alias histogram
  for (int i = 0; i != size; ++i) {
    const float r0 = in[(i + full_buckets) % size];
    const float r1 = in[(i + 1 + full_buckets) % size];
    out[i] = fraction * r1 + (1.f - fraction) * r0;
  }
  return CSM_OK;
}

int csm_compute_histogram(const float* points_xyz, int64_t n, int32_t histogram_size, float* out) {
  if (n < 0 || histogram_size <= 0 || !out || (n > 0 && !points_xyz)) return CSM_EINVAL;
  std::fill(out, out + histogram_size, 0.f);
  std::map<int, csm::HistSlice> slices;  // :160-171
  for (int64_t i = 0; i < n; ++i) {
    const csm::HistPoint p{points_xyz[3 * i], points_xyz[3 * i + 1], points_xyz[3 * i + 2]};
    slices[csm::HistRoundToInt(p.z / csm::kHistSliceHeight)].push_back(p);
  }
  for (const auto& slice : slices)
    csm::HistAddSlice(csm::HistSortSlice(slice.second), histogram_size, out);
  return CSM_OK;
}

int csm_hybrid_grid_insert_batch(csm_context* ctx, csm_hybrid_grid* const* grids,
                                 int32_t num_grids, const csm_inserter3d_options* options,
                                 int32_t num_scans, const float* origins_xyz,
                                 const float* returns_xyz, const int64_t* return_offsets,
                                 int32_t num_jobs, const int32_t* grid_of_job,
                                 const int32_t* scan_of_job, const float* transforms,
                                 int32_t num_transforms, const int32_t* transform_of_job,
                                 const float* max_ranges) {
  return InsertBatch3(ctx, grids, num_grids, options, num_scans, origins_xyz, returns_xyz,
                      return_offsets, num_jobs, grid_of_job, scan_of_job, transforms,
                      num_transforms, transform_of_job, max_ranges, false);
}

int csm_hybrid_grid_insert(csm_hybrid_grid* g, const csm_inserter3d_options* options,
                           const float* origin, const float* returns, int32_t n) {
  if (!g || !options || !origin || n < 0 || (n > 0 && !returns)) return CSM_EINVAL;
  const int32_t zero = 0;
  const int64_t off[2] = {0, n};
  csm_hybrid_grid* const grids[1] = {g};
  return InsertBatch3(nullptr, grids, 1, options, 1, origin, returns, off, 1, &zero, &zero,
                      nullptr, 0, nullptr, nullptr, true);
}

int csm_hybrid_grid_insert_intensities_batch(
    csm_context* ctx, csm_hybrid_grid* const* grids, int32_t num_grids,
    csm_intensity_grid* const* intensity_grids, int32_t num_intensity_grids,
    const csm_inserter3d_options* options, float intensity_threshold, int32_t num_scans,
    const float* origins_xyz, const float* returns_xyz, const int64_t* return_offsets,
    const float* const* scan_intensities, int32_t num_jobs, const int32_t* grid_of_job,
    const int32_t* scan_of_job, const int32_t* intensity_grid_of_job, const float* transforms,
    int32_t num_transforms, const int32_t* transform_of_job, const float* max_ranges) {
  const Intens3 in{intensity_grids, num_intensity_grids, intensity_grid_of_job, scan_intensities,
                   intensity_threshold};
  return InsertBatch3(ctx, grids, num_grids, options, num_scans, origins_xyz, returns_xyz,
                      return_offsets, num_jobs, grid_of_job, scan_of_job, transforms,
                      num_transforms, transform_of_job, max_ranges, false, &in);
}

int csm_hybrid_grid_insert_intensities(csm_hybrid_grid* g, csm_intensity_grid* intensity_grid,
                                       const csm_inserter3d_options* options,
                                       float intensity_threshold, const float* origin,
                                       const float* returns, const float* intensities,
                                       int32_t n) {
  if (!g || !options || !origin || n < 0 || (n > 0 && !returns)) return CSM_EINVAL;
  const int32_t zero = 0;
  const int64_t off[2] = {0, n};
  csm_hybrid_grid* const grids[1] = {g};
  csm_intensity_grid* const igrids[1] = {intensity_grid};
  const Intens3 in{igrids, intensity_grid ? 1 : 0, intensity_grid ? &zero : nullptr, &intensities,
                   intensity_threshold};
  return InsertBatch3(nullptr, grids, 1, options, 1, origin, returns, off, 1, &zero, &zero,
                      nullptr, 0, nullptr, nullptr, true, &in);
}

int csm_intensity_grid_create(csm_context* ctx, float resolution, csm_intensity_grid** out) {
  if (!ctx || !out || !(resolution > 0.f) || !std::isfinite(resolution)) return CSM_EINVAL;
  csm_intensity_grid* g = new csm_intensity_grid;
  g->ctx = ctx;
  g->resolution = resolution;
  *out = g;
  return CSM_OK;
}

void csm_intensity_grid_destroy(csm_intensity_grid* g) {
  if (!g) return;
  if (g->sum.ptr || g->ready) (void)hipSetDevice(g->ctx->device);
  g->ctx->pool.Give(&g->sum);  // reused by the next grid
  g->ctx->pool.Give(&g->count);
  if (g->ready) (void)hipEventDestroy(g->ready);
  delete g;
}

int csm_intensity_grid_info(const csm_intensity_grid* g, int32_t* origin3, int32_t* dims3,
                            int32_t* grid_size) {
  if (!g) return CSM_EINVAL;
  if (origin3) {
    origin3[0] = g->brick.ox;
    origin3[1] = g->brick.oy;
    origin3[2] = g->brick.oz;
  }
  if (dims3) {
    dims3[0] = g->brick.nx;
    dims3[1] = g->brick.ny;
    dims3[2] = g->brick.nz;
  }
  if (grid_size) *grid_size = g->grid_size;
  return CSM_OK;
}

int64_t csm_intensity_grid_device_bytes(const csm_intensity_grid* g) {
  return g ? static_cast<int64_t>(g->sum.bytes + g->count.bytes) : 0;
}

int csm_intensity_grid_read(const csm_intensity_grid* g, float* sums_out, int32_t* counts_out,
                            int64_t capacity) {
  if (!g || capacity < 0) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(g->ctx->mu);
  const int64_t n = static_cast<int64_t>(g->brick.nx) * g->brick.ny * g->brick.nz;
  if (capacity < n || (n > 0 && (!sums_out || !counts_out))) return CSM_EINVAL;
  if (n == 0) return CSM_OK;  // nothing was ever enqueued for this grid
  if (EnsureDevice(g->ctx)) return CSM_EHIP;
  CSM_HIP(hipMemcpyAsync(sums_out, g->sum.ptr, n * sizeof(float), hipMemcpyDeviceToHost,
                         g->ctx->stream));
  CSM_HIP(hipMemcpyAsync(counts_out, g->count.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost,
                         g->ctx->stream));
  CSM_HIP(hipStreamSynchronize(g->ctx->stream));
  return CSM_OK;
}

int csm_intensity_grid_get_intensity(const csm_intensity_grid* g, const int32_t* xyz_indices,
                                     int64_t n, float* out) {
  if (!g || n < 0 || (n > 0 && (!xyz_indices || !out))) return CSM_EINVAL;
  if (n == 0) return CSM_OK;
  csm_context* ctx = g->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  DevBuf din, dout;
  int rc;
  if ((rc = din.Reserve(sizeof(int32_t) * 3 * n)) || (rc = dout.Reserve(sizeof(float) * n)))
    return rc;
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(din.ptr, xyz_indices, sizeof(int32_t) * 3 * n, hipMemcpyHostToDevice,
                         st));
  hipLaunchKernelGGL(intensity_grid_lookup, dim3(static_cast<unsigned>((n + 255) / 256)),
                     dim3(256), 0, st, g->sum.as<float>(), g->count.as<int32_t>(), g->brick,
                     din.as<int32_t>(), n, dout.as<float>());
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(out, dout.ptr, sizeof(float) * n, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

int csm_hybrid_grid_read(const csm_hybrid_grid* g, uint16_t* out, int64_t capacity) {
  if (!g || capacity < 0) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(g->ctx->mu);
  const int64_t n = static_cast<int64_t>(g->brick.nx) * g->brick.ny * g->brick.nz;
  if (capacity < n || (n > 0 && !out)) return CSM_EINVAL;
  if (EnsureDevice(g->ctx)) return CSM_EHIP;
  if (n > 0)
    CSM_HIP(hipMemcpyAsync(out, g->values.ptr, n * sizeof(uint16_t), hipMemcpyDeviceToHost,
                           g->ctx->stream));
  CSM_HIP(hipStreamSynchronize(g->ctx->stream));
  return CSM_OK;
}

int csm_hybrid_grid_insert_stats(const csm_hybrid_grid* g, int64_t* cells_visited,
                                 int64_t* cells_updated) {
  if (!g) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(g->ctx->mu);
  unsigned long long s[2] = {0, 0};
  if (g->insert_stats.ptr) {
    if (EnsureDevice(g->ctx)) return CSM_EHIP;
    CSM_HIP(hipMemcpyAsync(s, g->insert_stats.ptr, sizeof(s), hipMemcpyDeviceToHost,
                           g->ctx->stream));
    CSM_HIP(hipStreamSynchronize(g->ctx->stream));
  }
  if (cells_visited) *cells_visited = static_cast<int64_t>(s[0]);
  if (cells_updated) *cells_updated = static_cast<int64_t>(s[1]);
  return CSM_OK;
}

}  // extern "C"
