// CeresScanMatcher2D::Match (mapping/internal/2d/scan_matching/
// ceres_scan_matcher_2d.cc:64-105), batched on gfx950: the refinement
// ConstraintBuilder2D::ComputeConstraint runs on every accepted branch-and-bound
// match (constraint_builder_2d.cc:245-249).
//
// One workgroup per pair. The residuals are the reference's three blocks:
// OccupiedSpaceCostFunction2D (occupied_space_cost_function_2d.cc:30-91: a
// ceres::BiCubicInterpolator over the submap's correspondence costs, padded by
// kPadding = INT_MAX / 4 cells of max cost, scaled by w / sqrt(N)), the
// translation delta to the match and the rotation delta to its angle. Each
// iteration the workgroup evaluates the N residual rows and their analytic
// Jacobian (what AutoDiff computes) in double, reduces J^T J and J^T r, and
// every lane takes the same Levenberg-Marquardt trust-region step with Ceres
// 1.13's defaults (Jacobi scaling from the initial Jacobian, radius 1e4,
// diagonal clamp [1e-6, 1e32], min relative decrease 1e-3, tolerances 1e-6 /
// 1e-10 / 1e-8, non-monotonic steps as pose_graph.lua:35 sets them). Ceres is
// absent from this image: the solver follows oracle/ceres2d.cc's restatement,
// which the reference's ceres_scan_matcher_2d_test.cc pins.
//
// csm_ceres2d_refine_batch sends each item to the kernel of its handle's kind:
// this one for probability grids, ceres2d_tsdf.hip's for TSDF handles. The
// single-call entry points csm_ceres2d_match_grid / _match_tsdf_grid run the
// same kernels on a device-resident grid's uint16 cells (kU16), for
// LocalTrajectoryBuilder2D::ScanMatch's call on the active submap.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "ceres2d_common.h"
#include "ceres_lm.h"
#include "csm_internal.h"

namespace csm {
namespace {

constexpr int kPadding = INT_MAX / 4;

// kU16: the cells of a device-resident grid through their value table
// (oracle/ceres2d.cc:50) instead of a handle's float plane.
template <bool kU16>
__device__ __forceinline__ double CostAt(const RefineDesc& d, int row, int col) {
  if (row < kPadding || col < kPadding || row >= d.ny + kPadding || col >= d.nx + kPadding)
    return d.max_cost;
  const int64_t at = static_cast<int64_t>(row - kPadding) * d.nx + (col - kPadding);
  if (kU16) return static_cast<double>(d.table[d.cells16[at] & 0x7fff]);
  return static_cast<double>(d.cost[at]);
}

// ceres::CubicHermiteSpline.
__device__ __forceinline__ void Hermite(double p0, double p1, double p2, double p3, double x,
                                        double* f, double* dfdx) {
  const double a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3);
  const double b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3);
  const double c = 0.5 * (-p0 + p2);
  const double d = p1;
  *f = d + x * (c + x * (b + x * a));
  if (dfdx) *dfdx = c + x * (2.0 * b + 3.0 * a * x);
}

// Residual row i (and its Jacobian row when J != nullptr) at pose x.
template <bool kU16>
__device__ void Row(const RefineDesc& d, const float* pts, double scale, const double* x, double s,
                    double c, int i, double* r, double* J) {
  const double px = static_cast<double>(pts[3 * i]), py = static_cast<double>(pts[3 * i + 1]);
  const double wx = c * px + (-s * py + x[0] * 1.);
  const double wy = s * px + (c * py + x[1] * 1.);
  const double rr = (d.max_x - wx) / d.resolution - 0.5 + static_cast<double>(kPadding);
  const double cc = (d.max_y - wy) / d.resolution - 0.5 + static_cast<double>(kPadding);
  const int row = static_cast<int>(floor(rr)), col = static_cast<int>(floor(cc));
  double fr[4], dfr[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int q = row - 1 + k;
    Hermite(CostAt<kU16>(d, q, col - 1), CostAt<kU16>(d, q, col), CostAt<kU16>(d, q, col + 1),
            CostAt<kU16>(d, q, col + 2),
            cc - col, &fr[k], &dfr[k]);
  }
  double f, dfdr, dfdc;
  Hermite(fr[0], fr[1], fr[2], fr[3], rr - row, &f, &dfdr);
  Hermite(dfr[0], dfr[1], dfr[2], dfr[3], rr - row, &dfdc, nullptr);
  *r = scale * f;
  if (J) {
    const double dwx_dt = -s * px - c * py, dwy_dt = c * px - s * py;
    J[0] = scale * (dfdr * (-1. / d.resolution));
    J[1] = scale * (dfdc * (-1. / d.resolution));
    J[2] = scale * (dfdr * (-dwx_dt / d.resolution) + dfdc * (-dwy_dt / d.resolution));
  }
}

// Pass over the N occupied-space rows plus the 3 delta rows at pose x:
// out[0] = sum r^2, and with jac, out[1..6] = Ju^T Ju (upper), out[7..9] = Ju^T r.
// kRows (csm_ceres2d_evaluate only): also writes residual i to rows_r[i] and
// its Jacobian row to rows_j[3 * i], n + 3 rows.
template <bool kU16, bool kJac, bool kRows = false>
__device__ void Pass(const RefineDesc& d, const float* pts, double scale, const RefineOpts& o,
                     const double* x, double* out, double (*red)[10], double* rows_r = nullptr,
                     double* rows_j = nullptr) {
  const double s = sin(x[2]), c = cos(x[2]);
  double acc[10] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  for (int i = threadIdx.x; i < d.n + 3; i += kRefineThreads) {
    double r, J[3] = {0., 0., 0.};
    if (i < d.n) {
      Row<kU16>(d, pts, scale, x, s, c, i, &r, kJac ? J : nullptr);
    } else if (i == d.n) {
      r = o.wt * (x[0] - d.target[0]);
      J[0] = o.wt;
    } else if (i == d.n + 1) {
      r = o.wt * (x[1] - d.target[1]);
      J[1] = o.wt;
    } else {
      r = o.wr * (x[2] - d.initial[2]);
      J[2] = o.wr;
    }
    if (kRows) {
      rows_r[i] = r;
      for (int a = 0; a < 3; ++a) rows_j[3 * i + a] = J[a];
    }
    acc[0] += r * r;
    if (kJac) {
      acc[1] += J[0] * J[0];
      acc[2] += J[0] * J[1];
      acc[3] += J[0] * J[2];
      acc[4] += J[1] * J[1];
      acc[5] += J[1] * J[2];
      acc[6] += J[2] * J[2];
      acc[7] += J[0] * r;
      acc[8] += J[1] * r;
      acc[9] += J[2] * r;
    }
  }
  BlockSum<10>(acc, red);
  for (int k = 0; k < 10; ++k) out[k] = acc[k];
}

// The minimizer loop is Ceres' TrustRegionMinimizer::Minimize: LM step
// (invalid when the model decrease is not positive), candidate cost,
// parameter then function tolerance (both end the solve without taking the
// candidate), acceptance by step quality > 1e-3; the lowest-cost accepted
// point is returned. Every thread runs the (scalar) step logic on the same
// block-reduced sums, so all of them hold the same state.
// Workgroup b refines items[order[b]] (order == nullptr: items[b]) and writes
// the result at that index.
template <bool kU16>
__global__ void __launch_bounds__(kRefineThreads)
ceres2d_refine(const RefineDesc* __restrict__ items, const int32_t* __restrict__ order,
               const float* __restrict__ points, RefineOpts o, double* __restrict__ out_pose,
               int32_t* __restrict__ out_iters) {
  __shared__ double red[kRefineThreads / 64][10];
  const int item = order ? order[blockIdx.x] : static_cast<int>(blockIdx.x);
  const RefineDesc d = items[item];
  const float* pts = points + 3 * d.point_offset;
  const double scale = o.occupied / sqrt(static_cast<double>(d.n));
  double x[3] = {d.initial[0], d.initial[1], d.initial[2]};
  double S[10];
  Pass<kU16, true>(d, pts, scale, o, x, S, red);
  double cost = 0.5 * S[0];
  // Jacobi scaling from the initial Jacobian.
  const double js[3] = {1. / (1. + sqrt(S[1])), 1. / (1. + sqrt(S[4])), 1. / (1. + sqrt(S[6]))};
  StepEvaluator ev(cost, o.nonmonotonic != 0);
  double best[3] = {x[0], x[1], x[2]}, best_cost = cost;
  LmRadius lm;
  int iter = 0, invalid = 0;
  auto gradient_small = [&]() {
    return fmax(fabs(S[7]), fmax(fabs(S[8]), fabs(S[9]))) <= 1e-10;
  };
  bool go = o.max_iterations > 0 && !gradient_small();
  while (go) {
    ++iter;
    const double Au[3][3] = {{S[1], S[2], S[3]}, {S[2], S[4], S[5]}, {S[3], S[5], S[6]}};
    double A[3][3], g[3], M[3][4], ds[3] = {0., 0., 0.};
    for (int a = 0; a < 3; ++a) {
      g[a] = S[7 + a] * js[a];
      for (int b = 0; b < 3; ++b) A[a][b] = Au[a][b] * js[a] * js[b];
    }
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) M[a][b] = A[a][b];
      M[a][a] += fmin(fmax(A[a][a], 1e-6), 1e32) / lm.radius;
      M[a][3] = -g[a];
    }
    const bool solved = Solve3(M, ds);
    double gd = 0., dad = 0.;
    for (int a = 0; a < 3; ++a) {
      gd += g[a] * ds[a];
      for (int b = 0; b < 3; ++b) dad += ds[a] * A[a][b] * ds[b];
    }
    const double model = -(gd + 0.5 * dad);
    if (!solved || !(model > 0.)) {
      if (++invalid > 5) break;  // HandleInvalidStep: LM rejects the step
      lm.Rejected();
    } else {
      invalid = 0;
      double xn[3], step_norm = 0., x_norm = 0.;
      for (int a = 0; a < 3; ++a) {
        const double step = ds[a] * js[a];
        xn[a] = x[a] + step;
        step_norm += step * step;
        x_norm += x[a] * x[a];
      }
      double T[10];
      Pass<kU16, false>(d, pts, scale, o, xn, T, red);
      const double new_cost = 0.5 * T[0];
      if (sqrt(step_norm) <= (sqrt(x_norm) + 1e-8) * 1e-8) break;  // parameter tolerance
      if (fabs(cost - new_cost) <= 1e-6 * cost) break;             // function tolerance
      const double quality = ev.Quality(new_cost, model);
      if (quality > 1e-3) {
        for (int a = 0; a < 3; ++a) x[a] = xn[a];
        Pass<kU16, true>(d, pts, scale, o, x, S, red);
        cost = 0.5 * S[0];
        lm.Accepted(quality);
        ev.Accepted(new_cost, model);
        if (cost < best_cost) {
          best_cost = cost;
          for (int a = 0; a < 3; ++a) best[a] = x[a];
        }
      } else {
        lm.Rejected();
      }
    }
    go = iter < o.max_iterations && lm.radius >= 1e-32 && !gradient_small();
  }
  if (threadIdx.x == 0) {
    out_pose[3 * item + 0] = best[0];
    out_pose[3 * item + 1] = best[1];
    out_pose[3 * item + 2] = best[2];
    if (out_iters) out_iters[item] = iter;
  }
}

// csm_ceres2d_evaluate / _evaluate_grid: one Pass<kU16, true> at pose x, the
// solver's own, which also writes its n + 3 rows; sums receives the 10
// block-reduced sums as the solver reads them. d.initial[2] is the target
// angle of the rotation delta row.
template <bool kU16>
__global__ void __launch_bounds__(kRefineThreads)
ceres2d_evaluate(RefineDesc d, const float* __restrict__ pts, RefineOpts o, double x0, double x1,
                 double x2, double* __restrict__ residuals, double* __restrict__ jacobian,
                 double* __restrict__ sums) {
  __shared__ double red[kRefineThreads / 64][10];
  const double scale = o.occupied / sqrt(static_cast<double>(d.n));
  const double x[3] = {x0, x1, x2};
  double S[10];
  Pass<kU16, true, true>(d, pts, scale, o, x, S, red, residuals, jacobian);
  if (threadIdx.x == 0)
    for (int k = 0; k < 10; ++k) sums[k] = S[k];
}

// Uploads the items, runs each through its grid kind's kernel and reads the
// results back in item order. u16: the items read device grids' uint16 cells.
// The caller holds ctx->mu.
int RunRefine2d(csm_context* ctx, const std::vector<RefineDesc>& desc,
                const std::vector<uint8_t>& tsdf, bool u16, const float* dpoints,
                const csm_ceres2d_options* options, csm_pose2d* out, int32_t* iterations) {
  const size_t n = desc.size();
  // Item indices by grid kind, probability items first. A batch of one kind
  // needs no index list: workgroup b takes item b.
  std::vector<int32_t> order;
  order.reserve(n);
  for (size_t i = 0; i < n; ++i)
    if (!tsdf[i]) order.push_back(static_cast<int32_t>(i));
  const int num_prob = static_cast<int>(order.size()), num_tsdf = static_cast<int>(n) - num_prob;
  for (size_t i = 0; i < n; ++i)
    if (tsdf[i]) order.push_back(static_cast<int32_t>(i));
  const bool mixed = num_prob > 0 && num_tsdf > 0;
  int rc;
  const size_t desc_bytes = sizeof(RefineDesc) * n;
  if ((rc = ctx->cr_items.Reserve(desc_bytes + (mixed ? sizeof(int32_t) * n : 0)))) return rc;
  if ((rc = ctx->cr_out.Reserve(sizeof(double) * 3 * n + sizeof(int32_t) * n))) return rc;
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(ctx->cr_items.ptr, desc.data(), desc_bytes, hipMemcpyHostToDevice, st));
  const RefineDesc* ditems = ctx->cr_items.as<RefineDesc>();
  const int32_t* dorder = nullptr;
  if (mixed) {
    dorder = reinterpret_cast<const int32_t*>(ctx->cr_items.as<char>() + desc_bytes);
    CSM_HIP(hipMemcpyAsync(const_cast<int32_t*>(dorder), order.data(), sizeof(int32_t) * n,
                           hipMemcpyHostToDevice, st));
  }
  const RefineOpts o{options->occupied_space_weight, options->translation_weight,
                     options->rotation_weight, options->max_num_iterations,
                     options->use_nonmonotonic_steps ? 1 : 0};
  double* dpose = ctx->cr_out.as<double>();
  int32_t* diters = reinterpret_cast<int32_t*>(dpose + 3 * n);
  if (num_prob > 0) {
    if (u16)
      hipLaunchKernelGGL(ceres2d_refine<true>, dim3(static_cast<unsigned>(num_prob)),
                         dim3(kRefineThreads), 0, st, ditems, dorder, dpoints, o, dpose, diters);
    else
      hipLaunchKernelGGL(ceres2d_refine<false>, dim3(static_cast<unsigned>(num_prob)),
                         dim3(kRefineThreads), 0, st, ditems, dorder, dpoints, o, dpose, diters);
    CSM_HIP(hipGetLastError());
  }
  if (num_tsdf > 0)
    CSM_HIP(LaunchCeres2dTsdfRefine(ditems, mixed ? dorder + num_prob : nullptr, num_tsdf, u16,
                                    dpoints, o, dpose, diters, st));
  std::vector<double> pose(3 * n);
  CSM_HIP(hipMemcpyAsync(pose.data(), dpose, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
  if (iterations)
    CSM_HIP(hipMemcpyAsync(iterations, diters, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; ++i) out[i] = csm_pose2d{pose[3 * i], pose[3 * i + 1], pose[3 * i + 2]};
  return CSM_OK;
}

int CheckCeres2dOptions(const csm_ceres2d_options* options) {
  if (!(options->occupied_space_weight > 0.) || !(options->translation_weight > 0.) ||
      !(options->rotation_weight > 0.) || options->max_num_iterations < 0)
    return CSM_EINVAL;  // the reference CHECKs the weights (ceres_scan_matcher_2d.cc:74-97)
  return CSM_OK;
}

int UploadSingleCloud(csm_context* ctx, const float* points_xyz, int32_t n) {
  if (!points_xyz || n < 1) return CSM_EINVAL;
  for (int64_t i = 0; i < 3 * static_cast<int64_t>(n); ++i)
    if (!std::isfinite(points_xyz[i])) return CSM_EINVAL;
  int rc;
  if ((rc = ctx->cr_points.Reserve(sizeof(float) * 3 * n))) return rc;
  CSM_HIP(hipMemcpyAsync(ctx->cr_points.ptr, points_xyz, sizeof(float) * 3 * n,
                         hipMemcpyHostToDevice, ctx->stream));
  return CSM_OK;
}

void FillSingleItem(const csm_map_limits& limits, const double target_xy[2],
                    const csm_pose2d* initial, int32_t n, RefineDesc* d) {
  d->max_x = limits.max_x;
  d->max_y = limits.max_y;
  d->resolution = limits.resolution;
  d->nx = limits.num_x_cells;
  d->ny = limits.num_y_cells;
  d->point_offset = 0;
  d->n = n;
  d->initial[0] = initial->x;
  d->initial[1] = initial->y;
  d->initial[2] = initial->theta;
  d->target[0] = target_xy[0];
  d->target[1] = target_xy[1];
}

// The evaluate entries' launch and read-back; the cloud is in ctx->cr_points
// and the caller holds ctx->mu.
int RunEvaluate2d(csm_context* ctx, const RefineDesc& d, bool u16,
                  const csm_ceres2d_options* options, const csm_pose2d* pose, double* residuals,
                  double* jacobian, double* sums) {
  const size_t rows = static_cast<size_t>(d.n) + 3;
  int rc;
  if ((rc = ctx->cr_out.Reserve(sizeof(double) * (4 * rows + 10)))) return rc;
  const RefineOpts o{options->occupied_space_weight, options->translation_weight,
                     options->rotation_weight, options->max_num_iterations,
                     options->use_nonmonotonic_steps ? 1 : 0};
  hipStream_t st = ctx->stream;
  double* dres = ctx->cr_out.as<double>();
  double* djac = dres + rows;
  double* dsums = djac + 3 * rows;
  if (u16)
    hipLaunchKernelGGL(ceres2d_evaluate<true>, dim3(1), dim3(kRefineThreads), 0, st, d,
                       ctx->cr_points.as<float>(), o, pose->x, pose->y, pose->theta, dres, djac,
                       dsums);
  else
    hipLaunchKernelGGL(ceres2d_evaluate<false>, dim3(1), dim3(kRefineThreads), 0, st, d,
                       ctx->cr_points.as<float>(), o, pose->x, pose->y, pose->theta, dres, djac,
                       dsums);
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(residuals, dres, sizeof(double) * rows, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipMemcpyAsync(jacobian, djac, sizeof(double) * 3 * rows, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipMemcpyAsync(sums, dsums, sizeof(double) * 10, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

bool FinitePose2d(const double target_xy[2], double target_theta, const csm_pose2d* pose) {
  return std::isfinite(target_xy[0]) && std::isfinite(target_xy[1]) &&
         std::isfinite(target_theta) && std::isfinite(pose->x) && std::isfinite(pose->y) &&
         std::isfinite(pose->theta);
}

}  // namespace
}  // namespace csm

extern "C" {

int csm_ceres2d_refine_batch(csm_context* ctx, csm_fast2d* const* submaps, int32_t num_submaps,
                             const csm_scan_set* scans, const csm_refine2d* items, int64_t n,
                             const csm_ceres2d_options* options, csm_pose2d* out,
                             int32_t* iterations) {
  using namespace csm;
  if (!ctx || !scans || !options || (n > 0 && (!items || !out || !submaps))) return CSM_EINVAL;
  if (n == 0) return CSM_OK;
  if (CheckCeres2dOptions(options)) return CSM_EINVAL;
  if (n > 0x7fffffff) return CSM_ERANGE;
  const int64_t num_scans = static_cast<int64_t>(scans->offsets.size()) - 1;
  std::vector<RefineDesc> desc(static_cast<size_t>(n));
  std::vector<uint8_t> tsdf(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    const csm_refine2d& it = items[i];
    if (it.submap < 0 || it.submap >= num_submaps || !submaps[it.submap] || it.scan < 0 ||
        it.scan >= num_scans)
      return CSM_EINVAL;
    const csm_fast2d* m = submaps[it.submap];
    if (m->ctx != ctx || !m->cost.ptr || (m->tsdf && !m->weight.ptr)) return CSM_EINVAL;
    RefineDesc& d = desc[i];
    d = RefineDesc{};
    d.cost = m->cost.as<float>();
    d.weight = m->tsdf ? m->weight.as<float>() : nullptr;
    tsdf[i] = m->tsdf ? 1 : 0;
    d.max_x = m->limits.max_x;
    d.max_y = m->limits.max_y;
    d.resolution = m->limits.resolution;
    d.nx = m->limits.num_x_cells;
    d.ny = m->limits.num_y_cells;
    d.max_cost = static_cast<double>(m->max_cc);
    d.point_offset = scans->offsets[it.scan];
    d.n = static_cast<int32_t>(scans->offsets[it.scan + 1] - scans->offsets[it.scan]);
    if (d.n <= 0) return CSM_EINVAL;
    d.initial[0] = it.initial.x;
    d.initial[1] = it.initial.y;
    d.initial[2] = it.initial.theta;
    d.target[0] = it.target_x;
    d.target[1] = it.target_y;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  return RunRefine2d(ctx, desc, tsdf, false, scans->points.as<float>(), options, out, iterations);
}

int csm_ceres2d_match_grid(csm_context* ctx, const csm_ceres2d_options* options,
                           const csm_probability_grid* grid, const double target_xy[2],
                           const csm_pose2d* initial, const float* points_xyz, int32_t n,
                           csm_pose2d* pose_out, int32_t* iterations_out) {
  using namespace csm;
  if (!ctx || !options || !grid || !target_xy || !initial || !pose_out) return CSM_EINVAL;
  if (grid->ctx != ctx || CheckCeres2dOptions(options)) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  int rc;
  if ((rc = UploadSingleCloud(ctx, points_xyz, n))) return rc;
  // ProbabilityGrid's bounds are the library constants (probability_values.h).
  const float min_cc = 1.f - (1.f - 0.1f), max_cc = 1.f - 0.1f;
  const float* table;
  if ((rc = EnsureValueTable(ctx, max_cc, min_cc, max_cc, &table))) return rc;
  std::vector<RefineDesc> desc(1);
  FillSingleItem(grid->limits, target_xy, initial, n, &desc[0]);
  desc[0].max_cost = static_cast<double>(max_cc);
  desc[0].cells16 = grid->cells.as<uint16_t>();
  desc[0].table = table;
  return RunRefine2d(ctx, desc, {0}, true, ctx->cr_points.as<float>(), options, pose_out,
                     iterations_out);
}

int csm_ceres2d_match_tsdf_grid(csm_context* ctx, const csm_ceres2d_options* options,
                                const csm_tsdf_grid* grid, const double target_xy[2],
                                const csm_pose2d* initial, const float* points_xyz, int32_t n,
                                csm_pose2d* pose_out, int32_t* iterations_out) {
  using namespace csm;
  if (!ctx || !options || !grid || !target_xy || !initial || !pose_out) return CSM_EINVAL;
  if (grid->ctx != ctx || CheckCeres2dOptions(options)) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  int rc;
  if ((rc = UploadSingleCloud(ctx, points_xyz, n))) return rc;
  // Grid2D's table of a TSDF2D (tsdf_2d.cc:24-27, grid_2d.cc:69-71) and
  // TSDValueConverter::ValueToWeight.
  const float *table, *wtable;
  if ((rc = EnsureValueTable(ctx, grid->truncation, -grid->truncation, grid->truncation, &table)) ||
      (rc = EnsureValueTable(ctx, 0.f, 0.f, grid->max_weight, &wtable)))
    return rc;
  std::vector<RefineDesc> desc(1);
  FillSingleItem(grid->limits, target_xy, initial, n, &desc[0]);
  desc[0].max_cost = static_cast<double>(grid->truncation);
  desc[0].cells16 = grid->tsd.as<uint16_t>();
  desc[0].table = table;
  desc[0].weight16 = grid->weight.as<uint16_t>();
  desc[0].wtable = wtable;
  return RunRefine2d(ctx, desc, {1}, true, ctx->cr_points.as<float>(), options, pose_out,
                     iterations_out);
}

int csm_ceres2d_evaluate(csm_context* ctx, const csm_fast2d* m, const csm_ceres2d_options* options,
                         const double target_xy[2], double target_theta, const csm_pose2d* pose,
                         const float* points_xyz, int32_t n, double* residuals, double* jacobian,
                         double* sums) {
  using namespace csm;
  if (!ctx || !m || !options || !target_xy || !pose || !residuals || !jacobian || !sums)
    return CSM_EINVAL;
  if (m->ctx != ctx || m->tsdf || !m->cost.ptr || CheckCeres2dOptions(options)) return CSM_EINVAL;
  if (!FinitePose2d(target_xy, target_theta, pose)) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  int rc;
  if ((rc = UploadSingleCloud(ctx, points_xyz, n))) return rc;
  RefineDesc d{};
  const csm_pose2d target{target_xy[0], target_xy[1], target_theta};
  FillSingleItem(m->limits, target_xy, &target, n, &d);
  d.cost = m->cost.as<float>();
  d.max_cost = static_cast<double>(m->max_cc);
  return RunEvaluate2d(ctx, d, false, options, pose, residuals, jacobian, sums);
}

int csm_ceres2d_evaluate_grid(csm_context* ctx, const csm_probability_grid* grid,
                              const csm_ceres2d_options* options, const double target_xy[2],
                              double target_theta, const csm_pose2d* pose, const float* points_xyz,
                              int32_t n, double* residuals, double* jacobian, double* sums) {
  using namespace csm;
  if (!ctx || !grid || !options || !target_xy || !pose || !residuals || !jacobian || !sums)
    return CSM_EINVAL;
  if (grid->ctx != ctx || !grid->cells.ptr || CheckCeres2dOptions(options)) return CSM_EINVAL;
  if (!FinitePose2d(target_xy, target_theta, pose)) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  int rc;
  if ((rc = UploadSingleCloud(ctx, points_xyz, n))) return rc;
  // The bounds and table of csm_ceres2d_match_grid.
  const float min_cc = 1.f - (1.f - 0.1f), max_cc = 1.f - 0.1f;
  const float* table;
  if ((rc = EnsureValueTable(ctx, max_cc, min_cc, max_cc, &table))) return rc;
  RefineDesc d{};
  const csm_pose2d target{target_xy[0], target_xy[1], target_theta};
  FillSingleItem(grid->limits, target_xy, &target, n, &d);
  d.max_cost = static_cast<double>(max_cc);
  d.cells16 = grid->cells.as<uint16_t>();
  d.table = table;
  return RunEvaluate2d(ctx, d, true, options, pose, residuals, jacobian, sums);
}

}  // extern "C"
