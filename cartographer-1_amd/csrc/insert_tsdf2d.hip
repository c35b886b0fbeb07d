// Device-resident TSDF2D and TSDFRangeDataInserter2D on gfx950
// (tsdf_range_data_inserter_2d.cc:33-240, normal_estimation_2d.cc:23-109,
// tsdf_2d.cc:23-135, tsd_value_converter.{h,cc}, ray_to_pixel_mask.cc:29-159).
//
// Why this inserter has to reproduce an ORDER. TSDF2D::SetCell refuses a cell
// that already carries the update marker (tsdf_2d.cc:56-69) and UpdateCell
// returns before SetCell when the update weight is 0.f (:230), so within one
// Insert a cell is written by the first ray, in the reference's iteration
// order, whose pixel mask holds it with a non-zero weight — and different rays
// would write different values. The ray order is the RangeDataSorter's
// (std::sort, not stable: the permutation among equivalent returns shows in
// the cells), so the host computes it with std::sort itself on an index array
// with the same comparator: the same algorithm fed the same comparison results
// moves the same positions.
//
// Host plan per scan (PlanScan). Everything that goes through libm or
// std::sort stays on the host, where the reference runs it: the sort, the
// normals (std::atan2), cos / sin of each normal, the range weight factor
// (std::pow in double), the angle weight factor (std::exp in double) and
// their float product; then, once the grown limits are known, the x1000
// subpixel indices of each ray's begin and end (SuperscaleRay, :53-67).
//
// First-writer rule on the device. Each grid keeps a rank plane, one 32-bit
// word per cell, all ones at rest.
//   tsdf2d_claim  one wave per ray k, lanes over the pixel columns of its
//                 mask (ColumnRun, insert2d_common.h). For every cell of the
//                 mask the update weight w(k, c) is computed, and when it is
//                 not 0.f, atomicMin(rank[c], k). A relaxed read first skips
//                 the atomic when the stored rank is already <= k (ranks only
//                 fall during the pass, so a stale value costs one redundant
//                 atomic, never a lost claim).
//   tsdf2d_apply  walks the same masks; the one thread with rank[c] == k (a
//                 ray's mask holds a cell at most once) reads the old TSD and
//                 weight through the converter's tables, computes UpdateCell
//                 (:227-239), writes TSDToValue / WeightToValue without the
//                 marker and stores all ones back to rank[c].
// Every cell has one writer, the result is the same from run to run, and the
// plane is clean when the call ends. The update marker never exists on the
// device; FinishUpdate is implicit. Work is proportional to the touched cells.
//
// Per (k, c) arithmetic follows the reference's expressions term by term:
// cell centre in double cast to float, correctly rounded float sqrt and
// division, the distance GaussianKernel in double with the device's exp. That
// exp is the one place where host and device libraries can differ; its result
// is multiplied by a double constant and rounded to float, so a last-place
// difference survives only on a float rounding boundary. f32 denormals are
// kept (the compiler's default for gfx950): narrow bandwidths produce denormal
// weights, and w == 0.f decides who claims a cell.
//
// The host steps of an insert call around the kernels are insert_host.h's;
// growth, create and crop over the three planes are insert2d_common.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <vector>

#include "csm_internal.h"
#include "insert2d_common.h"

namespace csm {
namespace {

constexpr uint32_t kNoRank = 0xffffffffu;

// One ray of a scan, in the reference's iteration order.
struct TsdfRay {
  int bx, by, ex, ey;  // begin and end, x1000 subpixel indices (SuperscaleRay)
  float hx, hy;        // the hit
  float range;
  float cosn, sinn;    // of the normal (unused without projection)
  float w;             // weight_factor_range * weight_factor_angle_ray_normal
  int cast;            // 0: range < truncation distance, or outside the limits
  int pad;
};

// One scan of a batch, as the kernels see it.
struct TsdfScanDev {
  uint16_t* tsd;
  uint16_t* weight;
  uint32_t* rank;
  const float* to_float;  // value -> TSD (32768), value -> weight (32768)
  int nx, ny;
  double max_x, max_y, resolution;
  float ox, oy;
  int num_rays;
  int64_t ray_begin;
  // The grid's TSDValueConverter (tsd_value_converter.cc:22-33).
  float min_tsd, max_tsd, tsd_resolution, conv_max_weight, weight_resolution;
};

// The options the kernels need, casts done where the reference casts.
struct TsdfOptsDev {
  float truncation;      // static_cast<float>(truncation_distance)
  float maximum_weight;  // static_cast<float>(maximum_weight)
  int project;
  int distance_kernel;   // distance bandwidth != 0
  double dist_pre;       // 1.0 / (kSqrtTwoPi * sigma)
  double dist_sigma2;    // sigma * sigma (a float product)
};

__device__ inline float ClampDev(float v, float lo, float hi) {  // common/math.h:32-40
  if (v > hi) return hi;
  if (v < lo) return lo;
  return v;
}

// update_tsd and update_weight of ray r at cell (x, y) (:204-222).
__device__ inline void CellUpdate(const TsdfScanDev& d, const TsdfOptsDev& o, const TsdfRay& r,
                                  int x, int y, float* tsd_out, float* w_out) {
  // MapLimits::GetCellCenter (map_limits.h:79-82): double, cast to float.
  const float cx = static_cast<float>(__dsub_rn(d.max_x, __dmul_rn(d.resolution, y + 0.5)));
  const float cy = static_cast<float>(__dsub_rn(d.max_y, __dmul_rn(d.resolution, x + 0.5)));
  float tsd;
  if (o.project) {
    tsd = __fadd_rn(__fmul_rn(__fsub_rn(cx, r.hx), r.cosn), __fmul_rn(__fsub_rn(cy, r.hy), r.sinn));
  } else {
    const float dx = __fsub_rn(cx, d.ox), dy = __fsub_rn(cy, d.oy);
    // sqrtf, not __fsqrt_rn: the latter is not correctly rounded on this
    // toolchain (see kernels3d.hip), sqrtf and __fdiv_rn are.
    tsd = __fsub_rn(r.range, sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))));
  }
  tsd = ClampDev(tsd, -o.truncation, o.truncation);
  float w = r.w;
  if (o.distance_kernel) {
    // GaussianKernel (:49-51): double arithmetic, float result.
    const double t = static_cast<double>(tsd);
    const double e = exp(__ddiv_rn(__dmul_rn(__dmul_rn(-0.5, t), t), o.dist_sigma2));
    w = __fmul_rn(w, static_cast<float>(__dmul_rn(o.dist_pre, e)));
  }
  *tsd_out = tsd;
  *w_out = w;
}

template <bool kApply>
__device__ inline void VisitCell(const TsdfScanDev& d, const TsdfOptsDev& o, const TsdfRay& r,
                                 uint32_t k, int x, int y) {
  if (static_cast<unsigned>(x) >= static_cast<unsigned>(d.nx) ||
      static_cast<unsigned>(y) >= static_cast<unsigned>(d.ny))
    return;
  const size_t c = static_cast<size_t>(y) * d.nx + x;
  uint32_t* rk = d.rank + c;
  if (!kApply) {
    if (__atomic_load_n(rk, __ATOMIC_RELAXED) <= k) return;
    float tsd, w;
    CellUpdate(d, o, r, x, y, &tsd, &w);
    if (w == 0.f) return;  // UpdateCell returns before SetCell (:230)
    atomicMin(rk, k);
    return;
  }
  if (__atomic_load_n(rk, __ATOMIC_RELAXED) != k) return;
  float tsd, w;
  CellUpdate(d, o, r, x, y, &tsd, &w);
  // UpdateCell (:227-239) on GetTSDAndWeight (tsdf_2d.cc:89-99).
  const float old_tsd = d.to_float[d.tsd[c] & 0x7fff];
  const float old_w = d.to_float[32768 + (d.weight[c] & 0x7fff)];
  float new_w = __fadd_rn(old_w, w);
  const float new_tsd =
      __fdiv_rn(__fadd_rn(__fmul_rn(old_tsd, old_w), __fmul_rn(tsd, w)), new_w);
  new_w = o.maximum_weight < new_w ? o.maximum_weight : new_w;  // std::min
  // TSDToValue / WeightToValue (tsd_value_converter.h:33-50), no marker.
  const float ct = ClampDev(new_tsd, d.min_tsd, d.max_tsd);
  const float cw = ClampDev(new_w, 0.f, d.conv_max_weight);
  d.tsd[c] = static_cast<uint16_t>(
      static_cast<int>(lroundf(__fmul_rn(__fsub_rn(ct, d.min_tsd), d.tsd_resolution))) + 1);
  d.weight[c] = static_cast<uint16_t>(
      static_cast<int>(lroundf(__fmul_rn(__fsub_rn(cw, 0.f), d.weight_resolution))) + 1);
  __atomic_store_n(rk, kNoRank, __ATOMIC_RELAXED);
}

// blockIdx.y is the scan; a wave takes one ray, lane k the runs of pixel
// columns k, k + 64, ...
template <bool kApply>
__device__ inline void WalkScan(const TsdfScanDev* __restrict__ scans,
                                const TsdfRay* __restrict__ rays, const TsdfOptsDev& o) {
  const TsdfScanDev d = scans[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int waves = blockDim.x >> 6;
  for (int ray = blockIdx.x * waves + (threadIdx.x >> 6); ray < d.num_rays;
       ray += gridDim.x * waves) {
    const TsdfRay r = rays[d.ray_begin + ray];
    if (!r.cast) continue;  // wave-uniform
    const RayWalk w = MakeRayWalk(r.bx, r.by, r.ex, r.ey, kSubpixelScale);
    const uint32_t k = static_cast<uint32_t>(ray);
    if (w.K == 0) {  // one column: lanes across its rows
      for (int y = w.ylo + lane; y <= w.yhi; y += 64) VisitCell<kApply>(d, o, r, k, w.col0, y);
      continue;
    }
    for (int col = lane; col <= w.K; col += 64) {
      int lo, hi;
      ColumnRun(w, col, &lo, &hi);
      for (int y = lo; y <= hi; ++y) VisitCell<kApply>(d, o, r, k, w.col0 + col, y);
    }
  }
}

__global__ void __launch_bounds__(256)
tsdf2d_claim(const TsdfScanDev* __restrict__ scans, const TsdfRay* __restrict__ rays,
             TsdfOptsDev o) {
  WalkScan<false>(scans, rays, o);
}

__global__ void __launch_bounds__(256)
tsdf2d_apply(const TsdfScanDev* __restrict__ scans, const TsdfRay* __restrict__ rays,
             TsdfOptsDev o) {
  WalkScan<true>(scans, rays, o);
}

// ComputeCroppedGrid's copy (tsdf_2d.cc:128-132): a known cell goes through
// SetCell(GetTSD, GetWeight), i.e. the two round-trip tables; unknown cells
// stay (0, 0). rt: TSD table then weight table.
__global__ void __launch_bounds__(256)
tsdf2d_crop(const uint16_t* __restrict__ tsd, const uint16_t* __restrict__ weight, int snx, int sx,
            int sy, uint16_t* __restrict__ tsd_out, uint16_t* __restrict__ weight_out, int w,
            int h, const uint16_t* __restrict__ rt) {
  const int64_t total = static_cast<int64_t>(w) * h;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int y = static_cast<int>(i / w), x = static_cast<int>(i % w);
    const size_t s = static_cast<size_t>(sy + y) * snx + sx + x;
    const uint16_t t = tsd[s] & 0x7fff;
    tsd_out[i] = t ? rt[t] : 0;
    weight_out[i] = t ? rt[32768 + (weight[s] & 0x7fff)] : 0;
  }
}

// ---------------------------------------------------------------- host -----

float ClampHost(float v, float lo, float hi) {
  if (v > hi) return hi;
  if (v < lo) return lo;
  return v;
}

// TSDValueConverter (tsd_value_converter.{h,cc}).
struct Converter {
  float min_tsd, max_tsd, max_weight, tsd_resolution, weight_resolution;
  Converter(float truncation, float max_w)
      : min_tsd(-truncation),
        max_tsd(truncation),
        max_weight(max_w),
        tsd_resolution(32766.f / (max_tsd - min_tsd)),
        weight_resolution(32766.f / (max_weight - 0.f)) {}
  uint16_t TSDToValue(float tsd) const {
    return static_cast<uint16_t>(
        static_cast<int>(std::lround((ClampHost(tsd, min_tsd, max_tsd) - min_tsd) * tsd_resolution)) +
        1);
  }
  uint16_t WeightToValue(float w) const {
    return static_cast<uint16_t>(
        static_cast<int>(std::lround((ClampHost(w, 0.f, max_weight) - 0.f) * weight_resolution)) + 1);
  }
};

// to_float: value -> TSD then value -> weight; round_trip likewise.
void MakeTables(float truncation, float max_weight, float* to_float, uint16_t* round_trip) {
  ConversionTable(-truncation, -truncation, truncation, to_float);
  ConversionTable(0.f, 0.f, max_weight, to_float + 32768);
  const Converter conv(truncation, max_weight);
  for (int v = 0; v < 32768; ++v) {
    round_trip[v] = conv.TSDToValue(to_float[v]);
    round_trip[32768 + v] = conv.WeightToValue(to_float[32768 + v]);
  }
}

// The context's tables of one (truncation, max weight) pair, made on first
// use (caller holds ctx->mu).
int EnsureTables(csm_context* ctx, float truncation, float max_weight, TsdfTables** out) {
  TsdfTables& t = ctx->tsdf_tabs[{truncation, max_weight}];
  *out = &t;
  if (t.to_float.ptr && t.round_trip.ptr) return CSM_OK;
  std::vector<float> f(2 * 32768);
  std::vector<uint16_t> rt(2 * 32768);
  MakeTables(truncation, max_weight, f.data(), rt.data());
  int rc;
  if ((rc = t.to_float.Reserve(f.size() * sizeof(float))) ||
      (rc = t.round_trip.Reserve(rt.size() * sizeof(uint16_t))))
    return rc;
  CSM_HIP(hipMemcpy(t.to_float.ptr, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
  CSM_HIP(hipMemcpy(t.round_trip.ptr, rt.data(), rt.size() * sizeof(uint16_t),
                    hipMemcpyHostToDevice));
  return CSM_OK;
}

float Norm3(float x, float y, float z) { return std::sqrt(x * x + (y * y + z * z)); }

// common/math.h:62-67 in float.
float NormalizeAngleDifference(float d) {
  const float kPi = static_cast<float>(M_PI);
  while (d > kPi) d -= 2. * kPi;
  while (d < -kPi) d += 2. * kPi;
  return d;
}

const float kSqrtTwoPi = std::sqrt(2.0 * M_PI);  // :31

// :49-51 (double arithmetic, float result).
float GaussianKernel(float x, float sigma) {
  return 1.0 / (kSqrtTwoPi * sigma) * std::exp(-0.5 * x * x / (sigma * sigma));
}

// :90-97 (std::pow(float, int) is evaluated in double).
float RangeWeightFactor(float range, int exponent) {
  constexpr float kMinRangeMeters = 1e-6f;
  float weight = 0.f;
  if (std::abs(range) > kMinRangeMeters) weight = 1.f / std::pow(range, exponent);
  return weight;
}

// normal_estimation_2d.cc:23-58 over p[3 * i ..], in float; Eigen's
// 3-element norm() reduces as x0 + (x1 + x2) (Norm3).
float EstimateNormal(const float* p, size_t est, size_t begin, size_t end, const float* origin) {
  const float* e = p + 3 * est;
  if (end - begin < 2) return std::atan2(origin[1] - e[1], origin[0] - e[0]);
  const float ox = origin[0] - e[0], oy = origin[1] - e[1], oz = origin[2] - e[2];
  float mx = 0.f, my = 0.f;
  for (size_t s = begin; s < end; ++s) {
    if (s == est) continue;
    const float* q = p + 3 * s;
    const float tx = e[0] - q[0], ty = e[1] - q[1];
    float nx = -ty, ny = tx;
    const float nz = 0.f;
    constexpr float kMinNormalLength = 1e-6f;
    if (Norm3(nx, ny, nz) < kMinNormalLength) continue;
    if (nx * ox + ny * oy + nz * oz < 0) {
      nx = -nx;
      ny = -ny;
    }
    const float sq = nx * nx + ny * ny + nz * nz;
    if (sq > 0.f) {  // Eigen's normalize()
      const float n = std::sqrt(sq);
      nx /= n;
      ny /= n;
    }
    mx += nx;
    my += ny;
  }
  return std::atan2(my, mx);
}

// normal_estimation_2d.cc:74-109 over the sorted returns.
void EstimateNormals(const float* p, size_t n, const float* origin, int num_samples, float radius,
                     float* normals) {
  const size_t max_num_samples = static_cast<size_t>(num_samples);
  auto dist = [&](size_t a, size_t b) {
    return Norm3(p[3 * a] - p[3 * b], p[3 * a + 1] - p[3 * b + 1], p[3 * a + 2] - p[3 * b + 2]);
  };
  for (size_t cur = 0; cur < n; ++cur) {
    size_t wb = cur;
    for (; wb > 0 && cur - wb < max_num_samples / 2 && dist(cur, wb - 1) < radius; --wb) {
    }
    size_t we = cur;
    for (; we < n && we - cur < std::ceil(max_num_samples / 2.0) + 1 && dist(cur, we) < radius;
         ++we) {
    }
    normals[cur] = EstimateNormal(p, cur, wb, we, origin);
  }
}

// One ray before the limits are known.
struct RayPlan {
  float bx, by, ex, ey;  // ray_begin, ray_end (:177-180)
  float hx, hy, range, cosn, sinn, w;
  bool cast;
};

// What one Insert needs that does not depend on the grid: the growth box, the
// ray order, the normals and the per-ray terms.
struct ScanPlanHost {
  float bmin_x, bmin_y, bmax_x, bmax_y;  // GrowAsNeeded's box (:33-47), unpadded
  std::vector<int32_t> order;
  std::vector<float> normals;
  std::vector<RayPlan> rays;
};

bool NeedsNormals(const csm_tsdf_inserter_options& o) {
  return o.project_sdf_distance_to_scan_normal != 0 ||
         o.update_weight_angle_scan_normal_to_ray_kernel_bandwidth != 0.f;
}

void PlanScan(const csm_tsdf_inserter_options& o, const float* origin, const float* returns,
              int32_t n, ScanPlanHost* out) {
  const float trunc = static_cast<float>(o.truncation_distance);
  // GrowAsNeeded: the origin and each hit pushed `trunc` along its ray
  // (normalized in 3D).
  float bmin_x = origin[0], bmax_x = origin[0], bmin_y = origin[1], bmax_y = origin[1];
  for (int32_t i = 0; i < n; ++i) {
    const float* h = returns + 3 * i;
    float dx = h[0] - origin[0], dy = h[1] - origin[1];
    const float dz = h[2] - origin[2];
    const float sq = dx * dx + dy * dy + dz * dz;
    if (sq > 0.f) {
      const float len = std::sqrt(sq);
      dx /= len;
      dy /= len;
    }
    const float ex = h[0] + trunc * dx, ey = h[1] + trunc * dy;
    bmin_x = std::min(bmin_x, ex);
    bmax_x = std::max(bmax_x, ex);
    bmin_y = std::min(bmin_y, ey);
    bmax_y = std::max(bmax_y, ey);
  }
  out->bmin_x = bmin_x;
  out->bmin_y = bmin_y;
  out->bmax_x = bmax_x;
  out->bmax_y = bmax_y;

  out->order.resize(n);
  for (int32_t i = 0; i < n; ++i) out->order[i] = i;
  const bool normals = NeedsNormals(o);
  out->normals.assign(n, std::numeric_limits<float>::quiet_NaN());
  std::vector<float> sorted;
  const float* pts = returns;
  if (normals && n > 0) {
    // RangeDataSorter (:69-88): the deltas to the origin, normalized in float
    // (Eigen's normalized(): divided by the norm when it is positive).
    std::vector<float> dir(2 * static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) {
      float x = returns[3 * i] - origin[0], y = returns[3 * i + 1] - origin[1];
      const float sq = x * x + y * y;
      if (sq > 0.f) {
        const float len = std::sqrt(sq);
        x /= len;
        y /= len;
      }
      dir[2 * i] = x;
      dir[2 * i + 1] = y;
    }
    std::sort(out->order.begin(), out->order.end(), [&](int32_t l, int32_t r) {
      const float lx = dir[2 * l], ly = dir[2 * l + 1], rx = dir[2 * r], ry = dir[2 * r + 1];
      if ((ly < 0.f) != (ry < 0.f)) return ly < 0.f;
      if (ly < 0.f) return lx < rx;
      return lx > rx;
    });
    sorted.resize(3 * static_cast<size_t>(n));
    for (int32_t k = 0; k < n; ++k) std::memcpy(&sorted[3 * k], returns + 3 * out->order[k], 12);
    pts = sorted.data();
    EstimateNormals(pts, n, origin, o.num_normal_samples, static_cast<float>(o.sample_radius),
                    out->normals.data());
  }

  out->rays.resize(n);
  const float ox = origin[0], oy = origin[1];
  for (int32_t k = 0; k < n; ++k) {
    RayPlan& r = out->rays[k];
    r = RayPlan{};
    r.hx = pts[3 * k];
    r.hy = pts[3 * k + 1];
    const float normal = out->normals[k];
    const float rx = r.hx - ox, ry = r.hy - oy;
    r.range = std::sqrt(rx * rx + ry * ry);
    r.cast = !(r.range < trunc);
    const float ratio = trunc / r.range;
    r.bx = ox;
    r.by = oy;
    if (!o.update_free_space) {
      const float f = 1.0f - ratio;
      r.bx = ox + f * rx;
      r.by = oy + f * ry;
    }
    const float fe = 1.0f + ratio;
    r.ex = ox + fe * rx;
    r.ey = oy + fe * ry;
    float wf_angle = 1.f;
    if (o.update_weight_angle_scan_normal_to_ray_kernel_bandwidth != 0.f) {
      const float angle = NormalizeAngleDifference(normal - std::atan2(-ry, -rx));
      wf_angle = GaussianKernel(
          angle, static_cast<float>(o.update_weight_angle_scan_normal_to_ray_kernel_bandwidth));
    }
    float wf_range = 1.f;
    if (o.update_weight_range_exponent != 0)
      wf_range = RangeWeightFactor(r.range, o.update_weight_range_exponent);
    r.w = wf_range * wf_angle;
    r.cosn = std::cos(normal);
    r.sinn = std::sin(normal);
  }
}

bool ValidOptions(const csm_tsdf_inserter_options* o) {
  return o && o->truncation_distance > 0. && o->maximum_weight > 0. &&
         static_cast<float>(o->truncation_distance) > 0.f &&
         static_cast<float>(o->maximum_weight) > 0.f && o->num_normal_samples >= 0 &&
         std::isfinite(o->truncation_distance) && std::isfinite(o->maximum_weight) &&
         std::isfinite(o->sample_radius) &&
         std::isfinite(o->update_weight_angle_scan_normal_to_ray_kernel_bandwidth) &&
         std::isfinite(o->update_weight_distance_cell_to_hit_kernel_bandwidth);
}

size_t CellBytes(size_t nx, size_t ny) { return nx * ny * sizeof(uint16_t); }
size_t RankBytes(size_t nx, size_t ny) { return nx * ny * sizeof(uint32_t); }
// The planes of a TSDF2D as growth sees them (insert2d_common.h).
const Plane2<csm_tsdf_grid> kPlanes[] = {{&csm_tsdf_grid::tsd, CellBytes, 0, true},
                                         {&csm_tsdf_grid::weight, CellBytes, 0, true},
                                         {&csm_tsdf_grid::rank, RankBytes, 0xff, false}};

// A scan's descriptor in limits `l`, without the planes.
TsdfScanDev ScanDesc(const csm_tsdf_grid* g, const TsdfTables* tabs, const csm_map_limits& l,
                     const float* origin, int num_rays, int64_t ray_begin) {
  const Converter conv(g->truncation, g->max_weight);
  TsdfScanDev d{};
  d.to_float = tabs->to_float.as<float>();
  d.nx = l.num_x_cells;
  d.ny = l.num_y_cells;
  d.max_x = l.max_x;
  d.max_y = l.max_y;
  d.resolution = l.resolution;
  d.ox = origin[0];
  d.oy = origin[1];
  d.num_rays = num_rays;
  d.ray_begin = ray_begin;
  d.min_tsd = conv.min_tsd;
  d.max_tsd = conv.max_tsd;
  d.tsd_resolution = conv.tsd_resolution;
  d.conv_max_weight = conv.max_weight;
  d.weight_resolution = conv.weight_resolution;
  return d;
}

// A scan's rays in the grown limits `l`. SuperscaleRay (:53-67): GetCellIndex
// on the x1000 limits, in double.
void SuperscaleRays(const csm_map_limits& l, const std::vector<RayPlan>& rays, TsdfRay* out) {
  const double fine = l.resolution / kSubpixelScale;
  const long fnx = static_cast<long>(l.num_x_cells) * kSubpixelScale;
  const long fny = static_cast<long>(l.num_y_cells) * kSubpixelScale;
  for (size_t k = 0; k < rays.size(); ++k) {
    const RayPlan& r = rays[k];
    TsdfRay& q = out[k];
    q = TsdfRay{};
    if (!r.cast) continue;
    long bx, by, ex, ey;
    CellIndex(l, fine, r.bx, r.by, &bx, &by);
    CellIndex(l, fine, r.ex, r.ey, &ex, &ey);
    // Outside the limits the reference CHECK-fails; such a ray is dropped.
    if (bx < 0 || by < 0 || ex < 0 || ey < 0 || bx >= fnx || ex >= fnx || by >= fny ||
        ey >= fny)
      continue;
    q.bx = static_cast<int>(bx);
    q.by = static_cast<int>(by);
    q.ex = static_cast<int>(ex);
    q.ey = static_cast<int>(ey);
    q.hx = r.hx;
    q.hy = r.hy;
    q.range = r.range;
    q.cosn = r.cosn;
    q.sinn = r.sinn;
    q.w = r.w;
    q.cast = 1;
  }
}

TsdfOptsDev OptsDev(const csm_tsdf_inserter_options* o) {
  TsdfOptsDev od{};
  od.truncation = static_cast<float>(o->truncation_distance);
  od.maximum_weight = static_cast<float>(o->maximum_weight);
  od.project = o->project_sdf_distance_to_scan_normal != 0;
  od.distance_kernel = o->update_weight_distance_cell_to_hit_kernel_bandwidth != 0.f;
  if (od.distance_kernel) {
    const float sigma = static_cast<float>(o->update_weight_distance_cell_to_hit_kernel_bandwidth);
    od.dist_pre = 1.0 / (kSqrtTwoPi * sigma);
    od.dist_sigma2 = sigma * sigma;
  }
  return od;
}

int InsertBatch(csm_context* ctx, csm_tsdf_grid* const* grids, int32_t num_grids,
                const csm_tsdf_inserter_options* o, int32_t num_scans,
                const int32_t* grid_of_scan, const float* origins, const float* returns,
                const int64_t* ret_off) {
  if (!ctx || !grids || !o || num_grids < 1 || num_scans < 0) return CSM_EINVAL;
  if (num_scans > 0 && (!grid_of_scan || !origins || !ret_off)) return CSM_EINVAL;
  if (!ValidOptions(o)) return CSM_EINVAL;
  for (int g = 0; g < num_grids; ++g)
    if (!grids[g]) return CSM_EINVAL;
  if (num_scans == 0) return CSM_OK;
  if (!ValidScans(num_scans, origins, ret_off, returns)) return CSM_EINVAL;
  for (int s = 0; s < num_scans; ++s)
    if (grid_of_scan[s] < 0 || grid_of_scan[s] >= num_grids) return CSM_EINVAL;
  const int64_t total_ret = ret_off[num_scans];
  // The points are checked before any handle is read.
  if (!ValidHandles(ctx, grids, num_grids)) return CSM_EINVAL;

  // The part of the plan that needs no grid, before the lock; batches of many
  // returns on a few threads, a scan at a time.
  std::vector<ScanPlanHost> host(num_scans);
  RunPlanTasks(num_scans, total_ret, [&](size_t s) {
    PlanScan(*o, origins + 3 * s, returns + 3 * ret_off[s],
             static_cast<int32_t>(ret_off[s + 1] - ret_off[s]), &host[s]);
  });

  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;
  for (int g = 0; g < num_grids; ++g)
    if (grids[g]->finished) return CSM_EINVAL;

  // On the host's copy of the limits: each scan's growth and its round.
  std::vector<GrowPlan2> plan(num_scans);
  std::vector<csm_map_limits> cur(num_grids);
  std::vector<int> rounds(num_grids, 0);
  std::vector<TsdfScanDev> descs(num_scans);
  std::vector<TsdfTables*> tabs(num_grids);
  int rc;
  for (int g = 0; g < num_grids; ++g) {
    cur[g] = grids[g]->limits;
    if ((rc = EnsureTables(ctx, grids[g]->truncation, grids[g]->max_weight, &tabs[g]))) return rc;
  }
  for (int s = 0; s < num_scans; ++s) {
    const ScanPlanHost& hp = host[s];
    const int g = grid_of_scan[s];
    const float box[4] = {hp.bmin_x, hp.bmin_y, hp.bmax_x, hp.bmax_y};
    if (!PlanGrowth2(g, box, &cur, &rounds, &plan[s])) return CSM_ERANGE;
    descs[s] = ScanDesc(grids[g], tabs[g], plan[s].after, origins + 3 * s,
                        static_cast<int>(hp.rays.size()), ret_off[s]);
  }
  // Scans in round order (stable).
  std::vector<int> order(num_scans);
  for (int s = 0; s < num_scans; ++s) order[s] = s;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return plan[a].round < plan[b].round; });

  // Everything that can fail cleanly, before anything is enqueued: a failure
  // leaves the grids as they were. One upload: descriptors, rays.
  const size_t desc_bytes = Align(sizeof(TsdfScanDev) * num_scans);
  const size_t bytes = desc_bytes + sizeof(TsdfRay) * static_cast<size_t>(total_ret);
  StageRing::Slot* slot = nullptr;
  if ((rc = TakeGrown2(ctx, grids, num_grids, kPlanes, &plan)) == CSM_OK)
    rc = ReserveUpload(ctx, &ctx->tsdf_stage, &ctx->tsdf_dev, bytes, &slot);
  if (rc != CSM_OK) {
    GiveBackGrown2(ctx, &plan);
    return rc;
  }
  TsdfScanDev* hd = slot->buf.as<TsdfScanDev>();
  TsdfRay* hr = reinterpret_cast<TsdfRay*>(slot->buf.as<char>() + desc_bytes);
  for (int i = 0; i < num_scans; ++i) {
    const int s = order[i];
    hd[i] = descs[s];
    hd[i].tsd = static_cast<uint16_t*>(plan[s].seen[0]);
    hd[i].weight = static_cast<uint16_t*>(plan[s].seen[1]);
    hd[i].rank = static_cast<uint32_t*>(plan[s].seen[2]);
    SuperscaleRays(plan[s].after, host[s].rays, hr + ret_off[s]);
  }
  const TsdfOptsDev od = OptsDev(o);
  // From here on a failure is a HIP error (insert_host.h): the grids keep what
  // they had when it struck.
  if ((rc = Upload(ctx, slot, &ctx->tsdf_dev, bytes))) return rc;
  hipStream_t st = ctx->stream;
  const TsdfScanDev* dd = ctx->tsdf_dev.as<TsdfScanDev>();
  const TsdfRay* dr = reinterpret_cast<const TsdfRay*>(ctx->tsdf_dev.as<char>() + desc_bytes);
  std::deque<DevBuf> retired;
  for (int i0 = 0, i1 = 0; i0 < num_scans; i0 = i1) {  // a round: [i0, i1)
    int64_t max_rays = 1;
    for (; i1 < num_scans && plan[order[i1]].round == plan[order[i0]].round; ++i1) {
      const int s = order[i1];
      if ((rc = CommitScan2(ctx, grids[plan[s].grid], kPlanes, &plan[s], &retired))) return rc;
      max_rays = std::max<int64_t>(max_rays, descs[s].num_rays);
    }
    for (int y0 = i0; y0 < i1; y0 += kMaxGridY) {
      const dim3 blocks(Blocks(max_rays, 4, 1024), ChunkOf(y0, i1));
      hipLaunchKernelGGL(tsdf2d_claim, blocks, dim3(256), 0, st, dd + y0, dr, od);
      CSM_HIP(hipGetLastError());
      hipLaunchKernelGGL(tsdf2d_apply, blocks, dim3(256), 0, st, dd + y0, dr, od);
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

int csm_tsdf_round_trip_tables(float truncation_distance, float max_weight, uint16_t* tsd_out,
                               uint16_t* weight_out) {
  if (!tsd_out || !weight_out || !(truncation_distance > 0.f) || !(max_weight > 0.f) ||
      !std::isfinite(truncation_distance) || !std::isfinite(max_weight))
    return CSM_EINVAL;
  std::vector<float> f(2 * 32768);
  std::vector<uint16_t> rt(2 * 32768);
  MakeTables(truncation_distance, max_weight, f.data(), rt.data());
  std::memcpy(tsd_out, rt.data(), 32768 * sizeof(uint16_t));
  std::memcpy(weight_out, rt.data() + 32768, 32768 * sizeof(uint16_t));
  return CSM_OK;
}

int csm_tsdf_plan_scan(const csm_tsdf_inserter_options* o, const float* origin,
                       const float* returns, int32_t n, int32_t* order_out, float* normals_out,
                       float* ray_weight_out, uint8_t* cast_out) {
  if (!ValidOptions(o) || !origin || n < 0 || (n > 0 && !returns) || n > (1 << 24))
    return CSM_EINVAL;
  const int64_t ro[2] = {0, n};
  if (!ValidScans(1, origin, ro, returns)) return CSM_EINVAL;
  ScanPlanHost plan;
  PlanScan(*o, origin, returns, n, &plan);
  for (int32_t k = 0; k < n; ++k) {
    if (order_out) order_out[k] = plan.order[k];
    if (normals_out) normals_out[k] = plan.normals[k];
    if (ray_weight_out) ray_weight_out[k] = plan.rays[k].w;
    if (cast_out) cast_out[k] = plan.rays[k].cast ? 1 : 0;
  }
  return CSM_OK;
}

int csm_tsdf_grid_create(csm_context* ctx, const csm_map_limits* limits, float truncation_distance,
                         float max_weight, const uint16_t* tsd_cells, const uint16_t* weight_cells,
                         csm_tsdf_grid** out) {
  if (!ctx || !limits || !out) return CSM_EINVAL;
  if ((tsd_cells == nullptr) != (weight_cells == nullptr)) return CSM_EINVAL;
  if (!(truncation_distance > 0.f) || !(max_weight > 0.f) || !std::isfinite(truncation_distance) ||
      !std::isfinite(max_weight))
    return CSM_EINVAL;
  int rc;
  if ((rc = CheckLimits2(limits))) return rc;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (EnsureDevice(ctx)) return CSM_EHIP;
  TsdfTables* tabs;
  if ((rc = EnsureTables(ctx, truncation_distance, max_weight, &tabs))) return rc;
  auto g = std::make_unique<csm_tsdf_grid>();
  g->ctx = ctx;
  g->limits = *limits;
  g->truncation = truncation_distance;
  g->max_weight = max_weight;
  g->id = g_next_grid_id.fetch_add(1);
  const uint16_t* const host[] = {tsd_cells, weight_cells, nullptr};
  if ((rc = NewPlanes2(g.get(), kPlanes, host))) return rc;
  *out = g.release();
  return CSM_OK;
}

void csm_tsdf_grid_destroy(csm_tsdf_grid* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  GivePlanes2(g, kPlanes);
  delete g;
}

int csm_tsdf_grid_limits(const csm_tsdf_grid* g, csm_map_limits* out) {
  if (!g || !out) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(g->ctx->mu);
  *out = g->limits;
  return CSM_OK;
}

int csm_tsdf_grid_read(const csm_tsdf_grid* g, uint16_t* tsd_out, uint16_t* weight_out,
                       int64_t capacity) {
  if (!g || !tsd_out || !weight_out) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(g->ctx->mu);
  const int64_t n = static_cast<int64_t>(g->limits.num_x_cells) * g->limits.num_y_cells;
  if (capacity < n) return CSM_EINVAL;
  if (EnsureDevice(g->ctx)) return CSM_EHIP;
  hipStream_t st = g->ctx->stream;
  CSM_HIP(hipMemcpyAsync(tsd_out, g->tsd.ptr, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  CSM_HIP(
      hipMemcpyAsync(weight_out, g->weight.ptr, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

int csm_tsdf_grid_insert(csm_tsdf_grid* g, const csm_tsdf_inserter_options* o, const float* origin,
                         const float* returns, int32_t num_returns) {
  if (!g || !o || !origin || num_returns < 0 || (num_returns > 0 && !returns)) return CSM_EINVAL;
  if (!ValidOptions(o)) return CSM_EINVAL;
  const int32_t zero = 0;
  const int64_t ro[2] = {0, num_returns};
  // The points are checked before the handle is read.
  if (!ValidScans(1, origin, ro, returns)) return CSM_EINVAL;
  csm_tsdf_grid* const grids[1] = {g};
  return InsertBatch(g->ctx, grids, 1, o, 1, &zero, origin, returns, ro);
}

int csm_tsdf_grid_insert_batch(csm_context* ctx, csm_tsdf_grid* const* grids, int32_t num_grids,
                               const csm_tsdf_inserter_options* o, int32_t num_scans,
                               const int32_t* grid_of_scan, const float* origins,
                               const float* returns, const int64_t* ret_off) {
  return InsertBatch(ctx, grids, num_grids, o, num_scans, grid_of_scan, origins, returns, ret_off);
}

int csm_tsdf_grid_finish(csm_tsdf_grid* g) {
  if (!g) return CSM_EINVAL;
  csm_context* ctx = g->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (g->finished) return CSM_OK;  // Submap2D::Finish runs once; a second call changes nothing
  if (EnsureDevice(ctx)) return CSM_EHIP;
  hipStream_t st = ctx->stream;
  int rc;
  TsdfTables* tabs;
  Crop2 c;
  const int nx = g->limits.num_x_cells, ny = g->limits.num_y_cells;
  if ((rc = EnsureTables(ctx, g->truncation, g->max_weight, &tabs)) ||
      (rc = CropBox2(ctx, g->tsd.as<uint16_t>(), nx, ny, &c)))
    return rc;
  const size_t cn = static_cast<size_t>(c.nx) * c.ny;
  DevBuf tsd, weight;
  if ((rc = ctx->pool.Take(cn * sizeof(uint16_t), &tsd)) ||
      (rc = ctx->pool.Take(cn * sizeof(uint16_t), &weight))) {
    if (tsd.ptr) ctx->pool.Give(&tsd);
    return rc;
  }
  // An all-unknown grid's single cell is (0, 0) in the source as well.
  hipLaunchKernelGGL(tsdf2d_crop, dim3(Blocks(static_cast<int64_t>(cn), 256, 4096)), dim3(256), 0,
                     st, g->tsd.as<uint16_t>(), g->weight.as<uint16_t>(), nx, c.ox, c.oy,
                     tsd.as<uint16_t>(), weight.as<uint16_t>(), c.nx, c.ny,
                     tabs->round_trip.as<uint16_t>());
  CSM_HIP(hipGetLastError());
  GivePlanes2(g, kPlanes);  // reused by later takes on this stream
  g->tsd = std::move(tsd);
  g->weight = std::move(weight);
  FinishCrop2(g, c);
  return CSM_OK;
}

int csm_rt2d_match_tsdf_grid(csm_context* ctx, const csm_rt_options* options,
                             const csm_tsdf_grid* grid, const csm_pose2d* initial,
                             const float* points_xyz, int32_t n, double* score, csm_pose2d* pose) {
  if (!ctx || !grid || grid->ctx != ctx) return CSM_EINVAL;
  return Rt2dMatchTsdfGrid(ctx, options, grid, initial, points_xyz, n, score, pose);
}

}  // extern "C"
