// CeresScanMatcher2D::Match on a TSDF2D (ceres_scan_matcher_2d.cc:74-91, the
// GridType::TSDF branch), on gfx950: ceres2d.hip's Levenberg-Marquardt
// refinement with TSDFMatchCostFunction2D (tsdf_match_cost_function_2d.cc:
// 39-66) over InterpolatedTSDF2D (interpolated_tsdf_2d.h:41-121) as its first
// residual block, scaled by occupied_space_weight / sqrt(N).
//
// Residual i is N s c_i w_i / W: c_i the bilinearly interpolated TSD at the
// transformed point (the constant +truncation, with zero gradient, when one of
// its four cells has weight 0), w_i the interpolated weight, W the sum of the
// w_j. The functor fails when W == 0. Each evaluation makes two passes over
// the points: W and dW/dpose first, then the rows with the quotient rule
// AutoDiff applies. The float / double mix of the interpolation (cell centres
// and differences of samples in float, everything else in double) is the
// reference's.
//
// A failed evaluation at the initial pose ends the solve there (Ceres:
// FAILURE, parameters untouched; the item returns its initial pose and 0
// iterations). A failed evaluation at a candidate gives the step the cost
// DBL_MAX, as Ceres 1.13's TrustRegionMinimizer does: the parameter-tolerance
// test still runs, the function-tolerance test cannot pass, the step quality
// is negative and the radius shrinks (restated from memory,
// unpinned).

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <vector>

#include "ceres2d_common.h"
#include "ceres_lm.h"
#include "csm_internal.h"
#include "geom2d_dev.h"

namespace csm {
namespace {

// The two planes of a csm_fast2d handle made from a TSDF.
struct PlaneCells {
  __device__ static float Tsd(const RefineDesc& d, int64_t at) { return d.cost[at]; }
  __device__ static float Weight(const RefineDesc& d, int64_t at) { return d.weight[at]; }
};

// The uint16 cells of a device-resident TSDF2D through the value tables
// (Grid2D::GetCorrespondenceCost, grid_2d.h:53-57; TSDF2D::GetWeight,
// tsdf_2d.cc:81-87), update marker masked off.
struct U16Cells {
  __device__ static float Tsd(const RefineDesc& d, int64_t at) {
    return d.table[d.cells16[at] & 0x7fff];
  }
  __device__ static float Weight(const RefineDesc& d, int64_t at) {
    return d.wtable[d.weight16[at] & 0x7fff];
  }
};

// InterpolatedTSDF2D::InterpolateBilinear (:95-104) and its gradient by (x, y).
__device__ __forceinline__ void Bilinear(double nx, double ny, double inv_dx, double inv_dy,
                                         float q11, float q12, float q21, float q22, double* f,
                                         double* dfdx, double* dfdy) {
  const double d1 = static_cast<double>(q12 - q11), d2 = static_cast<double>(q22 - q21);
  const double q1 = d1 * ny + static_cast<double>(q11);
  const double q2 = d2 * ny + static_cast<double>(q21);
  *f = (q2 - q1) * nx + q1;
  *dfdx = (q2 - q1) * inv_dx;
  const double dq1 = d1 * inv_dy, dq2 = d2 * inv_dy;
  *dfdy = (dq2 - dq1) * nx + dq1;
}

// GetCorrespondenceCost and GetWeight (:41-82) at the world point (x, y):
// c, w and their gradients by (x, y).
template <class Cells>
__device__ void Interpolate(const RefineDesc& d, double x, double y, double* c, double* dc,
                            double* w, double* dw) {
  // CenterOfLowerPixel (:109-121).
  const float fx = static_cast<float>(x), fy = static_cast<float>(y);
  const double cell_x = CellCoord(d.max_y, fy, d.resolution);
  const double cell_y = CellCoord(d.max_x, fx, d.resolution);
  float x1 = static_cast<float>(d.max_x - d.resolution * (cell_y + 0.5));
  float y1 = static_cast<float>(d.max_y - d.resolution * (cell_x + 0.5));
  if (static_cast<double>(x1) > x) x1 = static_cast<float>(static_cast<double>(x1) - d.resolution);
  if (static_cast<double>(y1) > y) y1 = static_cast<float>(static_cast<double>(y1) - d.resolution);
  const float fres = static_cast<float>(d.resolution);
  const float x2 = __fadd_rn(x1, fres), y2 = __fadd_rn(y1, fres);
  // index1 and its three neighbours (:46-52): Array2i(-1, 0) is one cell in x.
  const double ix = CellCoord(d.max_y, y1, d.resolution);
  const double iy = CellCoord(d.max_x, x1, d.resolution);
  float q[4], wt[4];
  bool all_weighted = true;
  int64_t at[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double cx = ix - (k & 1), cy = iy - (k >> 1);
    const bool inside = cx >= 0. && cy >= 0. && cx < d.nx && cy < d.ny;
    at[k] = inside ? static_cast<int64_t>(cy) * d.nx + static_cast<int64_t>(cx) : -1;
    wt[k] = inside ? Cells::Weight(d, at[k]) : 0.f;
    all_weighted = all_weighted && wt[k] != 0.f;
  }
  const double dx = static_cast<double>(__fsub_rn(x2, x1)), dy = static_cast<double>(__fsub_rn(y2, y1));
  const double nx = (x - static_cast<double>(x1)) / dx, ny = (y - static_cast<double>(y1)) / dy;
  const double inv_dx = 1. / dx, inv_dy = 1. / dy;
  // k = 0: q11, 1: q12 (-1, 0), 2: q21 (0, -1), 3: q22 (-1, -1).
  Bilinear(nx, ny, inv_dx, inv_dy, wt[0], wt[1], wt[2], wt[3], w, &dw[0], &dw[1]);
  if (!all_weighted) {
    *c = d.max_cost;
    dc[0] = dc[1] = 0.;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = Cells::Tsd(d, at[k]);
  Bilinear(nx, ny, inv_dx, inv_dy, q[0], q[1], q[2], q[3], c, &dc[0], &dc[1]);
}

// Point i at pose x: b = N s c w (before the division by W), w, and with kJac
// their gradients by the pose.
template <class Cells, bool kJac>
__device__ __forceinline__ void Point(const RefineDesc& d, const float* pts, double ns,
                                      const double* x, double s, double c, int i, double* b,
                                      double* db, double* w, double* dw) {
  const double px = static_cast<double>(pts[3 * i]), py = static_cast<double>(pts[3 * i + 1]);
  const double wx = c * px + (-s * py + x[0] * 1.);
  const double wy = s * px + (c * py + x[1] * 1.);
  double cc, dcc[2], ww, dww[2];
  Interpolate<Cells>(d, wx, wy, &cc, dcc, &ww, dww);
  *b = ns * cc * ww;
  *w = ww;
  if (kJac) {
    const double dwx_dt = -s * px - c * py, dwy_dt = c * px - s * py;
    const double dc[3] = {dcc[0], dcc[1], dcc[0] * dwx_dt + dcc[1] * dwy_dt};
    dw[0] = dww[0];
    dw[1] = dww[1];
    dw[2] = dww[0] * dwx_dt + dww[1] * dwy_dt;
    for (int a = 0; a < 3; ++a) db[a] = ns * (dc[a] * ww + cc * dw[a]);
  }
}

// W = sum w_i and (kJac) dW/dpose over the cloud; false when W == 0.
template <class Cells, bool kJac>
__device__ bool SummedWeight(const RefineDesc& d, const float* pts, double ns, const double* x,
                             double s, double c, double* W, double (*red)[4]) {
  double acc[4] = {0., 0., 0., 0.};
  for (int i = threadIdx.x; i < d.n; i += kRefineThreads) {
    double b, db[3], w, dw[3];
    Point<Cells, kJac>(d, pts, ns, x, s, c, i, &b, db, &w, dw);
    acc[0] += w;
    if (kJac)
      for (int a = 0; a < 3; ++a) acc[1 + a] += dw[a];
  }
  BlockSum<4>(acc, red);
  for (int k = 0; k < 4; ++k) W[k] = acc[k];
  return acc[0] != 0.;
}

// Row i of the cost block given W: r = b / W, J = db / W - b dW / W^2.
template <class Cells, bool kJac>
__device__ __forceinline__ void Row(const RefineDesc& d, const float* pts, double ns,
                                    const double* x, double s, double c, const double* W, int i,
                                    double* r, double* J) {
  double b, db[3], w, dw[3];
  Point<Cells, kJac>(d, pts, ns, x, s, c, i, &b, db, &w, dw);
  *r = b / W[0];
  if (kJac)
    for (int a = 0; a < 3; ++a) J[a] = (db[a] - *r * W[1 + a]) / W[0];
}

// ceres2d.hip's Pass with the TSDF cost block; false when the block fails to
// evaluate (out is then untouched).
template <class Cells, bool kJac>
__device__ bool Pass(const RefineDesc& d, const float* pts, double ns, const RefineOpts& o,
                     const double* x, double* out, double (*red)[10], double (*red4)[4]) {
  const double s = sin(x[2]), c = cos(x[2]);
  double W[4];
  if (!SummedWeight<Cells, kJac>(d, pts, ns, x, s, c, W, red4)) return false;
  double acc[10] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  for (int i = threadIdx.x; i < d.n + 3; i += kRefineThreads) {
    double r, J[3] = {0., 0., 0.};
    if (i < d.n) {
      Row<Cells, kJac>(d, pts, ns, x, s, c, W, i, &r, J);
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
  return true;
}

// ceres2d_refine's loop (Ceres' TrustRegionMinimizer::Minimize) with the two
// failure rules of the header comment. Every thread runs the scalar step logic
// on the same block-reduced sums.
template <class Cells>
__global__ void __launch_bounds__(kRefineThreads)
ceres2d_tsdf_refine(const RefineDesc* __restrict__ items, const int32_t* __restrict__ order,
                    const float* __restrict__ points, RefineOpts o, double* __restrict__ out_pose,
                    int32_t* __restrict__ out_iters) {
  __shared__ double red[kRefineThreads / 64][10];
  __shared__ double red4[kRefineThreads / 64][4];
  const int item = order ? order[blockIdx.x] : static_cast<int>(blockIdx.x);
  const RefineDesc d = items[item];
  const float* pts = points + 3 * d.point_offset;
  // T(point_cloud_.size()) * residual_scaling_factor_ (:57).
  const double ns = static_cast<double>(d.n) * (o.occupied / sqrt(static_cast<double>(d.n)));
  double x[3] = {d.initial[0], d.initial[1], d.initial[2]};
  double best[3] = {x[0], x[1], x[2]};
  int iter = 0;
  double S[10];
  if (Pass<Cells, true>(d, pts, ns, o, x, S, red, red4)) {
    double cost = 0.5 * S[0];
    // Jacobi scaling from the initial Jacobian.
    const double js[3] = {1. / (1. + sqrt(S[1])), 1. / (1. + sqrt(S[4])), 1. / (1. + sqrt(S[6]))};
    StepEvaluator ev(cost, o.nonmonotonic != 0);
    double best_cost = cost;
    LmRadius lm;
    int invalid = 0;
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
        // A candidate that fails to evaluate costs DBL_MAX.
        const double new_cost = Pass<Cells, false>(d, pts, ns, o, xn, T, red, red4) ? 0.5 * T[0] : DBL_MAX;
        if (sqrt(step_norm) <= (sqrt(x_norm) + 1e-8) * 1e-8) break;  // parameter tolerance
        if (fabs(cost - new_cost) <= 1e-6 * cost) break;             // function tolerance
        const double quality = ev.Quality(new_cost, model);
        if (quality > 1e-3) {
          for (int a = 0; a < 3; ++a) x[a] = xn[a];
          // The candidate evaluated, so the same point with its Jacobian does.
          Pass<Cells, true>(d, pts, ns, o, x, S, red, red4);
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
  }
  if (threadIdx.x == 0) {
    out_pose[3 * item + 0] = best[0];
    out_pose[3 * item + 1] = best[1];
    out_pose[3 * item + 2] = best[2];
    if (out_iters) out_iters[item] = iter;
  }
}

// The cost block alone at pose x (csm_ceres2d_tsdf_evaluate): n residuals and
// their n x 3 Jacobian through the device functions the solver uses; nothing
// is written when the evaluation fails.
__global__ void __launch_bounds__(kRefineThreads)
ceres2d_tsdf_evaluate(RefineDesc d, const float* __restrict__ pts, double scaling_factor,
                      double x0, double x1, double x2, double* __restrict__ residuals,
                      double* __restrict__ jacobian, int32_t* __restrict__ valid) {
  __shared__ double red4[kRefineThreads / 64][4];
  const double x[3] = {x0, x1, x2};
  const double ns = static_cast<double>(d.n) * scaling_factor;
  const double s = sin(x[2]), c = cos(x[2]);
  double W[4];
  const bool ok = SummedWeight<PlaneCells, true>(d, pts, ns, x, s, c, W, red4);
  if (threadIdx.x == 0) *valid = ok ? 1 : 0;
  if (!ok) return;
  for (int i = threadIdx.x; i < d.n; i += kRefineThreads)
    Row<PlaneCells, true>(d, pts, ns, x, s, c, W, i, &residuals[i], &jacobian[3 * i]);
}

}  // namespace

hipError_t LaunchCeres2dTsdfRefine(const RefineDesc* items, const int32_t* order, int count,
                                   bool u16, const float* points, const RefineOpts& o,
                                   double* out_pose, int32_t* out_iters, hipStream_t st) {
  if (u16)
    hipLaunchKernelGGL(ceres2d_tsdf_refine<U16Cells>, dim3(static_cast<unsigned>(count)),
                       dim3(kRefineThreads), 0, st, items, order, points, o, out_pose, out_iters);
  else
    hipLaunchKernelGGL(ceres2d_tsdf_refine<PlaneCells>, dim3(static_cast<unsigned>(count)),
                       dim3(kRefineThreads), 0, st, items, order, points, o, out_pose, out_iters);
  return hipGetLastError();
}

}  // namespace csm

extern "C" {

int csm_ceres2d_tsdf_evaluate(csm_context* ctx, const csm_fast2d* m, const float* points_xyz,
                              int32_t n, double scaling_factor, const double pose[3],
                              double* residuals, double* jacobian, int32_t* valid) {
  using namespace csm;
  if (!ctx || !m || !points_xyz || n < 1 || !pose || !residuals || !jacobian || !valid)
    return CSM_EINVAL;
  if (m->ctx != ctx || !m->tsdf || !m->cost.ptr || !m->weight.ptr) return CSM_EINVAL;
  for (int64_t i = 0; i < 3 * static_cast<int64_t>(n); ++i)
    if (!std::isfinite(points_xyz[i])) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  int rc;
  const size_t out_bytes = sizeof(double) * 4 * n + sizeof(int32_t);
  if ((rc = ctx->cr_points.Reserve(sizeof(float) * 3 * n)) || (rc = ctx->cr_out.Reserve(out_bytes)))
    return rc;
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(ctx->cr_points.ptr, points_xyz, sizeof(float) * 3 * n,
                         hipMemcpyHostToDevice, st));
  CSM_HIP(hipMemsetAsync(ctx->cr_out.ptr, 0, out_bytes, st));
  RefineDesc d{};
  d.cost = m->cost.as<float>();
  d.weight = m->weight.as<float>();
  d.max_x = m->limits.max_x;
  d.max_y = m->limits.max_y;
  d.resolution = m->limits.resolution;
  d.nx = m->limits.num_x_cells;
  d.ny = m->limits.num_y_cells;
  d.max_cost = static_cast<double>(m->max_cc);
  d.n = n;
  double* dres = ctx->cr_out.as<double>();
  double* djac = dres + n;
  int32_t* dvalid = reinterpret_cast<int32_t*>(djac + 3 * static_cast<size_t>(n));
  hipLaunchKernelGGL(ceres2d_tsdf_evaluate, dim3(1), dim3(kRefineThreads), 0, st, d,
                     ctx->cr_points.as<float>(), scaling_factor, pose[0], pose[1], pose[2], dres,
                     djac, dvalid);
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(residuals, dres, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipMemcpyAsync(jacobian, djac, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipMemcpyAsync(valid, dvalid, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

}  // extern "C"
