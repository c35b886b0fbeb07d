// CeresScanMatcher3D::Match (mapping/internal/3d/scan_matching/
// ceres_scan_matcher_3d.cc:84-160), batched on gfx950: the refinement
// ConstraintBuilder3D::ComputeConstraint runs on every accepted match
// (constraint_builder_3d.cc:264-275).
//
// One workgroup per match. Residuals: OccupiedSpaceCostFunction3D for the
// high-resolution cloud in the high-resolution HybridGrid and the
// low-resolution cloud in the low-resolution grid (InterpolatedGrid's
// smooth-step tricubic interpolation, interpolated_grid.h:50-150), the
// translation delta to the match and the rotation delta vec(target^-1 q).
// The pose is (t, q) with ceres::QuaternionParameterization: Jacobians are
// taken in the 6-dimensional tangent space and a step updates
// q <- (cos|d|, sin|d|/|d| d) * q. Each iteration the workgroup reduces
// J^T J (6 x 6) and J^T r in double and one lane takes a Levenberg-Marquardt
// trust-region step with Ceres' defaults, as oracle/ceres3d.cc restates
// (parity with Ceres unpinned).
//
// With an intensity grid (LocalTrajectoryBuilder3D::ScanMatch,
// local_trajectory_builder_3d.cc:488-501; ceres_scan_matcher_3d.cc:126-142)
// the high-resolution cloud also feeds IntensityCostFunction3D
// (intensity_cost_function_3d.h:67-85) under ceres::HuberLoss: in the same pass
// over the points its sum of squares, J^T J and J^T r go into a second set of
// sums, and after the block reduction 0.5 rho(S) joins the cost and rho' J^T J,
// rho' J^T r the normal equations. That is Ceres' Corrector for a loss with
// rho'' <= 0, which Huber's is in both regimes: residuals and Jacobian scaled
// by sqrt(rho'). The Huber and Corrector rules are written from memory of
// Ceres 1.13 and are unpinned like the LM loop. The second set is compiled out
// of the kernel for items without an intensity grid (kIntens), whose
// arithmetic is unchanged.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ceres_lm.h"
#include "csm_internal.h"

namespace csm {
namespace {

constexpr int kR3Threads = 256;
constexpr int kSums = 1 + 21 + 6;  // cost, upper J^T J, J^T r

struct GridView3 {
  const float* prob;
  Brick3 b;
  float res;
};

struct Refine3Desc {
  GridView3 grid[2];
  int64_t offset[2];  // into the points buffer (points)
  int32_t n[2];
  double t[3], q[4], target[3];
};

struct Refine3Opts {
  double w0, w1, wt, wr;
  int max_iterations;
  int nonmonotonic;  // ceres_solver_options.use_nonmonotonic_steps
};

// IntensityHybridGrid on the device (csm_intensity_grid).
struct IntensView3 {
  const float* sum;
  const int32_t* count;
  Brick3 b;
  float res;
};

// The intensity block of one item: IntensityCostFunction3D's arguments and the
// Huber scale.
struct IntensBlock3 {
  IntensView3 g;
  int64_t offset;  // of the high-resolution cloud's intensities in the values buffer
  double scale;    // weight / sqrt(N)
  double huber;
  float threshold;
};

// InterpolatedGrid::GetValue for the intensity grid: GetIntensity
// (hybrid_grid.h:563-570), 0 for a cell that no return fell into.
__device__ __forceinline__ double Prob(const IntensView3& g, int x, int y, int z) {
  const int lx = x - g.b.ox, ly = y - g.b.oy, lz = z - g.b.oz;
  if (static_cast<unsigned>(lx) >= static_cast<unsigned>(g.b.nx) ||
      static_cast<unsigned>(ly) >= static_cast<unsigned>(g.b.ny) ||
      static_cast<unsigned>(lz) >= static_cast<unsigned>(g.b.nz))
    return 0.;
  const int64_t i = (static_cast<int64_t>(lz) * g.b.ny + ly) * g.b.nx + lx;
  const int32_t c = g.count[i];
  return c == 0 ? 0. : static_cast<double>(__fdiv_rn(g.sum[i], static_cast<float>(c)));
}

__device__ __forceinline__ double Prob(const GridView3& g, int x, int y, int z) {
  const int lx = x - g.b.ox, ly = y - g.b.oy, lz = z - g.b.oz;
  if (static_cast<unsigned>(lx) >= static_cast<unsigned>(g.b.nx) ||
      static_cast<unsigned>(ly) >= static_cast<unsigned>(g.b.ny) ||
      static_cast<unsigned>(lz) >= static_cast<unsigned>(g.b.nz))
    return static_cast<double>(0.1f);  // unknown: kMinProbability
  return static_cast<double>(g.prob[(static_cast<int64_t>(lz) * g.b.ny + ly) * g.b.nx + lx]);
}

// HybridGridBase::GetCellIndex: lround(p / res) in float.
__device__ __forceinline__ int CellF(float v, float res) {
  return static_cast<int>(roundf(__fdiv_rn(v, res)));
}

struct StepF {
  double t, tt, ttt;
  __device__ double f(double a, double b) const { return (a - b) * ttt * 2. + (b - a) * tt * 3. + a; }
  __device__ double dt(double a, double b) const { return (a - b) * 6. * tt + (b - a) * 6. * t; }
  __device__ double da() const { return 2. * ttt - 3. * tt + 1.; }
  __device__ double db() const { return -2. * ttt + 3. * tt; }
};

// InterpolatedGrid::GetInterpolatedValue and its gradient; View is the grid
// (GridView3: probabilities, IntensView3: mean intensities).
template <typename View>
__device__ double Interpolate(const View& g, double x, double y, double z, double* grad) {
  const float res = g.res;
  const float fx = static_cast<float>(x), fy = static_cast<float>(y), fz = static_cast<float>(z);
  float cx = __fmul_rn(static_cast<float>(CellF(fx, res)), res);
  float cy = __fmul_rn(static_cast<float>(CellF(fy, res)), res);
  float cz = __fmul_rn(static_cast<float>(CellF(fz, res)), res);
  if (cx > x) cx = __fsub_rn(cx, res);
  if (cy > y) cy = __fsub_rn(cy, res);
  if (cz > z) cz = __fsub_rn(cz, res);
  const double x1 = cx, y1 = cy, z1 = cz;
  const double x2 = __fadd_rn(cx, res), y2 = __fadd_rn(cy, res), z2 = __fadd_rn(cz, res);
  const int ix = CellF(cx, res), iy = CellF(cy, res), iz = CellF(cz, res);
  const double q111 = Prob(g, ix, iy, iz), q112 = Prob(g, ix, iy, iz + 1);
  const double q121 = Prob(g, ix, iy + 1, iz), q122 = Prob(g, ix, iy + 1, iz + 1);
  const double q211 = Prob(g, ix + 1, iy, iz), q212 = Prob(g, ix + 1, iy, iz + 1);
  const double q221 = Prob(g, ix + 1, iy + 1, iz), q222 = Prob(g, ix + 1, iy + 1, iz + 1);
  const double nx = (x - x1) / (x2 - x1), ny = (y - y1) / (y2 - y1), nz = (z - z1) / (z2 - z1);
  const StepF sx{nx, nx * nx, nx * (nx * nx)}, sy{ny, ny * ny, ny * (ny * ny)},
      sz{nz, nz * nz, nz * (nz * nz)};
  const double q11 = sz.f(q111, q112), q12 = sz.f(q121, q122);
  const double q21 = sz.f(q211, q212), q22 = sz.f(q221, q222);
  const double q1 = sy.f(q11, q12), q2 = sy.f(q21, q22);
  if (grad) {
    grad[0] = sx.dt(q1, q2) / (x2 - x1);
    grad[1] = (sx.da() * sy.dt(q11, q12) + sx.db() * sy.dt(q21, q22)) / (y2 - y1);
    grad[2] = (sx.da() * (sy.da() * sz.dt(q111, q112) + sy.db() * sz.dt(q121, q122)) +
               sx.db() * (sy.da() * sz.dt(q211, q212) + sy.db() * sz.dt(q221, q222))) /
              (z2 - z1);
  }
  return sx.f(q1, q2);
}

// Eigen _transformVector and its derivative in (w, x, y, z) (3 x 4).
__device__ void Rotate(const double* q, const double v[3], double out[3], double* J) {
  const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
  const double ax = qy * v[2] - qz * v[1], ay = qz * v[0] - qx * v[2], az = qx * v[1] - qy * v[0];
  const double ux = 2. * ax, uy = 2. * ay, uz = 2. * az;
  out[0] = v[0] + w * ux + (qy * uz - qz * uy);
  out[1] = v[1] + w * uy + (qz * ux - qx * uz);
  out[2] = v[2] + w * uz + (qx * uy - qy * ux);
  if (!J) return;
  const double V[9] = {0., -v[2], v[1], v[2], 0., -v[0], -v[1], v[0], 0.};
  const double A[9] = {0., -az, ay, az, 0., -ax, -ay, ax, 0.};
  const double Q[9] = {0., -qz, qy, qz, 0., -qx, -qy, qx, 0.};
  const double u[3] = {ux, uy, uz};
  for (int r = 0; r < 3; ++r) {
    J[4 * r] = u[r];
    for (int c = 0; c < 3; ++c) {
      double qv_v = 0.;
      for (int k = 0; k < 3; ++k) qv_v += Q[3 * r + k] * V[3 * k + c];
      J[4 * r + 1 + c] = -2. * w * V[3 * r + c] - 2. * A[3 * r + c] - 2. * qv_v;
    }
  }
}

__device__ void QuatProduct(const double* a, const double* b, double* z) {
  z[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  z[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  z[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  z[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

__device__ __forceinline__ double WaveSumD(double v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ void BlockSum(double* v, double (*red)[kSums]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = 0; k < kSums; ++k) {
    const double t = WaveSumD(v[k]);
    if (lane == 0) red[w][k] = t;
  }
  __syncthreads();
  for (int k = 0; k < kSums; ++k) {
    double t = 0.;
    for (int q = 0; q < kR3Threads / 64; ++q) t += red[q][k];
    v[k] = t;
  }
  __syncthreads();
}

// Adds residual r with tangent Jacobian row j[6] to the sums.
__device__ __forceinline__ void Accumulate(double* acc, double r, const double* j, bool jac) {
  acc[0] += r * r;
  if (!jac) return;
  int k = 1;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) acc[k++] += j[a] * j[b];
  for (int a = 0; a < 6; ++a) acc[22 + a] += j[a] * r;
}

// IntensityCostFunction3D's residual i and its tangent Jacobian row (zero
// above the threshold) at the transformed point w; Jq is Rotate's derivative
// and L the parameterization's Jacobian.
template <bool kJac>
__device__ void IntensityRow(const IntensBlock3& b, float intensity, const double* w,
                             const double* Jq, const double* L, double* r, double* j) {
  *r = 0.;
  if (intensity > b.threshold) return;
  double grad[3];
  const double val = Interpolate(b.g, w[0], w[1], w[2], kJac ? grad : nullptr);
  *r = b.scale * (val - static_cast<double>(intensity));
  if (kJac) {
    double dq[4] = {0., 0., 0., 0.};
    for (int c = 0; c < 4; ++c)
      for (int a = 0; a < 3; ++a) dq[c] += b.scale * grad[a] * Jq[4 * a + c];
    for (int a = 0; a < 3; ++a) j[a] = b.scale * grad[a];
    for (int c = 0; c < 3; ++c) {
      double s = 0.;
      for (int m = 0; m < 4; ++m) s += dq[m] * L[3 * m + c];
      j[3 + c] = s;
    }
  }
}

// ceres::HuberLoss(a) at s: rho and rho' (loss_function.cc); rho'' <= 0.
__device__ __forceinline__ void Huber(double a, double s, double* rho, double* rho1) {
  if (s > a * a) {
    const double r = sqrt(s);
    *rho = 2. * a * r - a * a;
    *rho1 = fmax(2.2250738585072014e-308, a / r);  // std::numeric_limits<double>::min()
  } else {
    *rho = s;
    *rho1 = 1.;
  }
}

// kRows (csm_ceres3d_evaluate only): also writes residual i to rows_r[i] and
// its tangent Jacobian row to rows_j[6 * i], n[0] + n[1] + 6 rows.
template <bool kJac, bool kIntens, bool kRows = false>
__device__ void Pass3(const Refine3Desc& d, const float* pts, const double* scale,
                      const Refine3Opts& o, const double* t, const double* q,
                      const double* target_inv, double* out, double (*red)[kSums],
                      const IntensBlock3* ib, const float* values, double* rows_r = nullptr,
                      double* rows_j = nullptr) {
  double acc[kSums], acc2[kIntens ? kSums : 1];
  for (int k = 0; k < kSums; ++k) acc[k] = 0.;
  if (kIntens)
    for (int k = 0; k < kSums; ++k) acc2[k] = 0.;
  // QuaternionParameterization::ComputeJacobian (4 x 3).
  const double L[12] = {-q[1], -q[2], -q[3], q[0], q[3], -q[2], -q[3], q[0], q[1], q[2], -q[1], q[0]};
  const int n0 = d.n[0], total = d.n[0] + d.n[1] + 6;
  for (int i = threadIdx.x; i < total; i += kR3Threads) {
    double r, j[6] = {0., 0., 0., 0., 0., 0.};
    if (i < n0 + d.n[1]) {
      const int k = i < n0 ? 0 : 1;
      const float* p = pts + 3 * (d.offset[k] + (i < n0 ? i : i - n0));
      const double v[3] = {static_cast<double>(p[0]), static_cast<double>(p[1]),
                           static_cast<double>(p[2])};
      double w[3], Jq[12], grad[3];
      Rotate(q, v, w, kJac ? Jq : nullptr);
      for (int a = 0; a < 3; ++a) w[a] += t[a];
      if (kIntens && k == 0) {
        double r2, j2[6] = {0., 0., 0., 0., 0., 0.};
        IntensityRow<kJac>(*ib, values[ib->offset + i], w, Jq, L, &r2, j2);
        Accumulate(acc2, r2, j2, kJac);
      }
      const double val = Interpolate(d.grid[k], w[0], w[1], w[2], kJac ? grad : nullptr);
      r = scale[k] * (1. - val);
      if (kJac) {
        double dq[4] = {0., 0., 0., 0.};
        for (int c = 0; c < 4; ++c)
          for (int a = 0; a < 3; ++a) dq[c] += -scale[k] * grad[a] * Jq[4 * a + c];
        for (int a = 0; a < 3; ++a) j[a] = -scale[k] * grad[a];
        for (int c = 0; c < 3; ++c) {
          double s = 0.;
          for (int m = 0; m < 4; ++m) s += dq[m] * L[3 * m + c];
          j[3 + c] = s;
        }
      }
    } else if (i < n0 + d.n[1] + 3) {
      const int a = i - n0 - d.n[1];
      r = o.wt * (t[a] - d.target[a]);
      j[a] = o.wt;
    } else {
      const int a = i - n0 - d.n[1] - 3;
      double delta[4];
      QuatProduct(target_inv, q, delta);
      r = o.wr * delta[a + 1];
      const double* ti = target_inv;
      const double M[3][4] = {{ti[1], ti[0], -ti[3], ti[2]},
                              {ti[2], ti[3], ti[0], -ti[1]},
                              {ti[3], -ti[2], ti[1], ti[0]}};
      for (int c = 0; c < 3; ++c) {
        double s = 0.;
        for (int m = 0; m < 4; ++m) s += o.wr * M[a][m] * L[3 * m + c];
        j[3 + c] = s;
      }
    }
    if (kRows) {
      rows_r[i] = r;
      for (int a = 0; a < 6; ++a) rows_j[6 * i + a] = j[a];
    }
    Accumulate(acc, r, j, kJac);
  }
  BlockSum(acc, red);
  for (int k = 0; k < kSums; ++k) out[k] = acc[k];
  if (kIntens) {
    BlockSum(acc2, red);
    double rho, rho1;
    Huber(ib->huber, acc2[0], &rho, &rho1);
    out[0] += rho;
    for (int k = 1; k < kSums; ++k) out[k] += rho1 * acc2[k];
  }
}

__device__ bool Solve6(double* M, double* b, double* out) {
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    for (int i = c + 1; i < 6; ++i)
      if (fabs(M[i * 6 + c]) > fabs(M[piv * 6 + c])) piv = i;
    if (M[piv * 6 + c] == 0.) return false;
    for (int j = 0; j < 6; ++j) {
      const double s = M[c * 6 + j];
      M[c * 6 + j] = M[piv * 6 + j];
      M[piv * 6 + j] = s;
    }
    const double sb = b[c];
    b[c] = b[piv];
    b[piv] = sb;
    for (int i = c + 1; i < 6; ++i) {
      const double f = M[i * 6 + c] / M[c * 6 + c];
      for (int j = c; j < 6; ++j) M[i * 6 + j] -= f * M[c * 6 + j];
      b[i] -= f * b[c];
    }
  }
  for (int i = 5; i >= 0; --i) {
    double v = b[i];
    for (int j = i + 1; j < 6; ++j) v -= M[i * 6 + j] * out[j];
    out[i] = v / M[i * 6 + i];
  }
  return true;
}

__device__ void Unpack(const double* S, double* Au, double* gu) {
  int k = 1;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      Au[6 * a + b] = S[k];
      Au[6 * b + a] = S[k];
      ++k;
    }
  for (int a = 0; a < 6; ++a) gu[a] = S[22 + a];
}

// Ceres 1.13 TrustRegionMinimizer::Minimize as in ceres2d.hip: every thread
// runs the 6-dimensional step logic on the same block-reduced sums.
template <bool kIntens>
__global__ void __launch_bounds__(kR3Threads)
ceres3d_refine(const Refine3Desc* __restrict__ items, const float* __restrict__ points,
               Refine3Opts o, double* __restrict__ out, int32_t* __restrict__ out_iters,
               const IntensBlock3* __restrict__ blocks, const float* __restrict__ values) {
  __shared__ double red[kR3Threads / 64][kSums];
  const Refine3Desc d = items[blockIdx.x];
  IntensBlock3 block;
  if (kIntens) block = blocks[blockIdx.x];
  const IntensBlock3* ib = kIntens ? &block : nullptr;
  const double scale[2] = {o.w0 / sqrt(static_cast<double>(d.n[0])),
                           o.w1 / sqrt(static_cast<double>(d.n[1]))};
  const double target_inv[4] = {d.q[0], -d.q[1], -d.q[2], -d.q[3]};
  double t[3] = {d.t[0], d.t[1], d.t[2]}, q[4] = {d.q[0], d.q[1], d.q[2], d.q[3]};
  double S[kSums], T[kSums];
  Pass3<true, kIntens>(d, points, scale, o, t, q, target_inv, S, red, ib, values);
  double cost = 0.5 * S[0];
  double Au[36], gu[6], js[6];
  Unpack(S, Au, gu);
  for (int a = 0; a < 6; ++a) js[a] = 1. / (1. + sqrt(Au[7 * a]));
  StepEvaluator ev(cost, o.nonmonotonic != 0);
  LmRadius lm;
  double best_t[3] = {t[0], t[1], t[2]}, best_q[4] = {q[0], q[1], q[2], q[3]}, best_cost = cost;
  int iter = 0, invalid = 0;
  auto gradient_small = [&]() {
    double gmax = 0.;
    for (int a = 0; a < 6; ++a) gmax = fmax(gmax, fabs(gu[a]));
    return gmax <= 1e-10;
  };
  bool go = o.max_iterations > 0 && !gradient_small();
  while (go) {
    ++iter;
    double A[36], g[6], M[36], rhs[6], ds[6] = {0., 0., 0., 0., 0., 0.};
    for (int a = 0; a < 6; ++a) {
      g[a] = gu[a] * js[a];
      for (int b = 0; b < 6; ++b) A[6 * a + b] = Au[6 * a + b] * js[a] * js[b];
    }
    for (int a = 0; a < 6; ++a) {
      for (int b = 0; b < 6; ++b) M[6 * a + b] = A[6 * a + b];
      M[7 * a] += fmin(fmax(A[7 * a], 1e-6), 1e32) / lm.radius;
      rhs[a] = -g[a];
    }
    const bool solved = Solve6(M, rhs, ds);
    double gd = 0., dad = 0.;
    for (int a = 0; a < 6; ++a) {
      gd += g[a] * ds[a];
      for (int b = 0; b < 6; ++b) dad += ds[a] * A[6 * a + b] * ds[b];
    }
    const double model = -(gd + 0.5 * dad);
    if (!solved || !(model > 0.)) {
      if (++invalid > 5) break;  // HandleInvalidStep: LM rejects the step
      lm.Rejected();
    } else {
      invalid = 0;
      double step[6], step_norm = 0., x_norm = 0.;
      for (int a = 0; a < 6; ++a) {
        step[a] = ds[a] * js[a];
        step_norm += step[a] * step[a];
      }
      for (int a = 0; a < 3; ++a) x_norm += t[a] * t[a];
      for (int a = 0; a < 4; ++a) x_norm += q[a] * q[a];
      // Plus: t + dt; QuaternionParameterization::Plus on the rotation.
      double tn[3] = {t[0] + step[0], t[1] + step[1], t[2] + step[2]}, qn[4];
      const double nrm = sqrt(step[3] * step[3] + step[4] * step[4] + step[5] * step[5]);
      if (nrm > 0.) {
        const double sn = sin(nrm) / nrm;
        const double qd[4] = {cos(nrm), sn * step[3], sn * step[4], sn * step[5]};
        QuatProduct(qd, q, qn);
      } else {
        for (int a = 0; a < 4; ++a) qn[a] = q[a];
      }
      Pass3<false, kIntens>(d, points, scale, o, tn, qn, target_inv, T, red, ib, values);
      const double new_cost = 0.5 * T[0];
      if (sqrt(step_norm) <= (sqrt(x_norm) + 1e-8) * 1e-8) break;  // parameter tolerance
      if (fabs(cost - new_cost) <= 1e-6 * cost) break;             // function tolerance
      const double quality = ev.Quality(new_cost, model);
      if (quality > 1e-3) {
        for (int a = 0; a < 3; ++a) t[a] = tn[a];
        for (int a = 0; a < 4; ++a) q[a] = qn[a];
        Pass3<true, kIntens>(d, points, scale, o, t, q, target_inv, S, red, ib, values);
        cost = 0.5 * S[0];
        Unpack(S, Au, gu);
        lm.Accepted(quality);
        ev.Accepted(new_cost, model);
        if (cost < best_cost) {
          best_cost = cost;
          for (int a = 0; a < 3; ++a) best_t[a] = t[a];
          for (int a = 0; a < 4; ++a) best_q[a] = q[a];
        }
      } else {
        lm.Rejected();
      }
    }
    go = iter < o.max_iterations && lm.radius >= 1e-32 && !gradient_small();
  }
  if (threadIdx.x == 0) {
    for (int a = 0; a < 3; ++a) out[7 * blockIdx.x + a] = best_t[a];
    for (int a = 0; a < 4; ++a) out[7 * blockIdx.x + 3 + a] = best_q[a];
    if (out_iters) out_iters[blockIdx.x] = iter;
  }
}

// csm_ceres3d_evaluate: one Pass3<true, false> at the pose (d.t, d.q), the
// plain solver's own, which also writes its rows; sums receives the kSums
// block-reduced sums as the solver reads them. The rotation delta is taken to
// target_q, which the solver sets to its initial rotation.
struct Quat3 {
  double v[4];
};
__global__ void __launch_bounds__(kR3Threads)
ceres3d_evaluate(Refine3Desc d, const float* __restrict__ points, Refine3Opts o, Quat3 target_q,
                 double* __restrict__ residuals, double* __restrict__ jacobian,
                 double* __restrict__ sums) {
  __shared__ double red[kR3Threads / 64][kSums];
  const double scale[2] = {o.w0 / sqrt(static_cast<double>(d.n[0])),
                           o.w1 / sqrt(static_cast<double>(d.n[1]))};
  const double target_inv[4] = {target_q.v[0], -target_q.v[1], -target_q.v[2], -target_q.v[3]};
  double S[kSums];
  Pass3<true, false, true>(d, points, scale, o, d.t, d.q, target_inv, S, red, nullptr, nullptr,
                           residuals, jacobian);
  if (threadIdx.x == 0)
    for (int k = 0; k < kSums; ++k) sums[k] = S[k];
}

// Test-visible lookups on a device grid (csm_hybrid_grid_get_probability /
// _interpolate): the same Prob / Interpolate the refinement kernel uses.
__global__ void grid_probability(GridView3 g, const int32_t* __restrict__ ijk, int64_t n,
                                 float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = static_cast<float>(Prob(g, ijk[3 * i], ijk[3 * i + 1], ijk[3 * i + 2]));
}
__global__ void grid_interpolate(GridView3 g, const double* __restrict__ xyz, int64_t n,
                                 double* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = Interpolate(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], nullptr);
}

template <typename In, typename Out, typename K>
int GridLookup(const csm_hybrid_grid* g, const In* in, int64_t n, Out* out, K kernel) {
  if (!g || n < 0 || (n > 0 && (!in || !out))) return CSM_EINVAL;
  if (n == 0) return CSM_OK;
  csm_context* ctx = g->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  DevBuf din, dout;
  int rc;
  if ((rc = din.Reserve(sizeof(In) * 3 * n)) || (rc = dout.Reserve(sizeof(Out) * n))) return rc;
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(din.ptr, in, sizeof(In) * 3 * n, hipMemcpyHostToDevice, st));
  const GridView3 view{g->prob.as<float>(), g->brick, g->resolution};
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, view,
                     din.as<In>(), n, dout.as<Out>());
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(out, dout.ptr, sizeof(Out) * n, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

// csm_ceres3d_intensity_evaluate: IntensityCostFunction3D alone, one thread
// per point, through IntensityRow.
__global__ void ceres3d_intensity_eval(IntensBlock3 block, const float* __restrict__ points,
                                       const float* __restrict__ values, int32_t n,
                                       const double* __restrict__ pose,
                                       double* __restrict__ residuals,
                                       double* __restrict__ jacobian) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* t = pose;
  const double* q = pose + 3;
  const double L[12] = {-q[1], -q[2], -q[3], q[0], q[3], -q[2], -q[3], q[0], q[1], q[2], -q[1], q[0]};
  const double v[3] = {static_cast<double>(points[3 * i]), static_cast<double>(points[3 * i + 1]),
                       static_cast<double>(points[3 * i + 2])};
  double w[3], Jq[12], r, j[6] = {0., 0., 0., 0., 0., 0.};
  Rotate(q, v, w, Jq);
  for (int a = 0; a < 3; ++a) w[a] += t[a];
  IntensityRow<true>(block, values[i], w, Jq, L, &r, j);
  residuals[i] = r;
  for (int a = 0; a < 6; ++a) jacobian[6 * i + a] = j[a];
}

// The intensity half of csm_ceres3d_refine_intensity_batch; null for
// csm_ceres3d_refine_batch.
struct Intens3Args {
  const csm_intensity_grid* const* grids;
  int32_t num_grids;
  const float* const* node_intensities;  // per node, of its high-resolution cloud
  const int32_t* grid_of_item;           // -1: none
  const csm_ceres3d_intensity_options* options;
};

int Refine3Batch(csm_context* ctx, const csm_hybrid_grid* const* grids, int32_t num_grids,
                 const csm_node3d* nodes, int32_t num_nodes, const csm_refine3d* items, int64_t n,
                 const csm_ceres3d_options* options, csm_pose3d* out, int32_t* iterations,
                 const Intens3Args* ia) {
  if (!ctx || !options || (n > 0 && (!items || !out || !grids || !nodes))) return CSM_EINVAL;
  if (n == 0) return CSM_OK;
  if (!(options->occupied_space_weight_0 > 0.) || !(options->occupied_space_weight_1 > 0.) ||
      !(options->translation_weight > 0.) || !(options->rotation_weight > 0.) ||
      options->max_num_iterations < 0)
    return CSM_EINVAL;  // CHECK_GTs of ceres_scan_matcher_3d.cc:106-156
  if (n > 0x7fffffff) return CSM_ERANGE;
  // Items with an intensity grid run the kernel with the intensity block, after
  // the others: item i is descriptor slot[i].
  std::vector<int64_t> slot(static_cast<size_t>(n));
  int64_t num_plain = n;
  if (ia && ia->grid_of_item) {
    num_plain = 0;
    for (int64_t i = 0; i < n; ++i) num_plain += ia->grid_of_item[i] < 0;
  }
  const int64_t num_intens = n - num_plain;
  if (num_intens > 0) {
    const csm_ceres3d_intensity_options* io = ia->options;
    // CHECK_GTs of ceres_scan_matcher_3d.cc:127-130.
    if (!io || !(io->weight > 0.) || !(io->huber_scale > 0.) || !(io->intensity_threshold > 0.))
      return CSM_EINVAL;
  }
  for (int64_t i = 0, p = 0, q = num_plain; i < n; ++i)
    slot[i] = num_intens > 0 && ia->grid_of_item[i] >= 0 ? q++ : p++;
  // Node clouds once each, high then low resolution; the high-resolution
  // cloud's intensities once each.
  std::vector<int64_t> off(2 * static_cast<size_t>(num_nodes), -1);
  std::vector<int64_t> voff(static_cast<size_t>(num_nodes), -1);
  std::vector<float> pts, vals;
  std::vector<Refine3Desc> desc(static_cast<size_t>(n));
  std::vector<IntensBlock3> blocks(static_cast<size_t>(num_intens));
  for (int64_t i = 0; i < n; ++i) {
    const csm_refine3d& it = items[i];
    if (it.high_grid < 0 || it.high_grid >= num_grids || it.low_grid < 0 ||
        it.low_grid >= num_grids || !grids[it.high_grid] || !grids[it.low_grid] || it.node < 0 ||
        it.node >= num_nodes)
      return CSM_EINVAL;
    const csm_node3d& nd = nodes[it.node];
    if (nd.num_high_resolution <= 0 || nd.num_low_resolution <= 0 || !nd.high_resolution_xyz ||
        !nd.low_resolution_xyz)
      return CSM_EINVAL;
    if (off[2 * it.node] < 0) {
      off[2 * it.node] = static_cast<int64_t>(pts.size() / 3);
      pts.insert(pts.end(), nd.high_resolution_xyz, nd.high_resolution_xyz + 3 * nd.num_high_resolution);
      off[2 * it.node + 1] = static_cast<int64_t>(pts.size() / 3);
      pts.insert(pts.end(), nd.low_resolution_xyz, nd.low_resolution_xyz + 3 * nd.num_low_resolution);
    }
    Refine3Desc& d = desc[slot[i]];
    const csm_hybrid_grid* g[2] = {grids[it.high_grid], grids[it.low_grid]};
    for (int k = 0; k < 2; ++k) {
      // Grids from any context on ctx's device (e.g. one whose stream built
      // them while ctx searched); their builds are waited for below.
      if (!g[k]->ctx || g[k]->ctx->device != ctx->device) return CSM_EINVAL;
      d.grid[k] = GridView3{g[k]->prob.as<float>(), g[k]->brick, g[k]->resolution};
      d.offset[k] = off[2 * it.node + k];
    }
    d.n[0] = nd.num_high_resolution;
    d.n[1] = nd.num_low_resolution;
    for (int a = 0; a < 3; ++a) {
      d.t[a] = it.initial.t[a];
      d.target[a] = it.target[a];
    }
    for (int a = 0; a < 4; ++a) d.q[a] = it.initial.q[a];
    if (slot[i] < num_plain) continue;
    // The intensity block on the high-resolution cloud (cloud 0) only.
    const int32_t ig = ia->grid_of_item[i];
    if (ig >= ia->num_grids || !ia->grids[ig] || !ia->node_intensities ||
        !ia->node_intensities[it.node])
      return CSM_EINVAL;
    const csm_intensity_grid* igrid = ia->grids[ig];
    if (!igrid->ctx || igrid->ctx->device != ctx->device) return CSM_EINVAL;
    if (voff[it.node] < 0) {
      const float* v = ia->node_intensities[it.node];
      for (int32_t k = 0; k < nd.num_high_resolution; ++k)
        if (!std::isfinite(v[k])) return CSM_EINVAL;
      voff[it.node] = static_cast<int64_t>(vals.size());
      vals.insert(vals.end(), v, v + nd.num_high_resolution);
    }
    blocks[slot[i] - num_plain] = IntensBlock3{
        IntensView3{igrid->sum.as<float>(), igrid->count.as<int32_t>(), igrid->brick,
                    igrid->resolution},
        voff[it.node], ia->options->weight / std::sqrt(static_cast<double>(nd.num_high_resolution)),
        ia->options->huber_scale, static_cast<float>(ia->options->intensity_threshold)};
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  int rc;
  const size_t desc_bytes = (sizeof(Refine3Desc) * n + 15) & ~size_t{15};
  if ((rc = ctx->cr3_items.Reserve(desc_bytes + sizeof(IntensBlock3) * num_intens))) return rc;
  if ((rc = ctx->cr3_points.Reserve(sizeof(float) * std::max<size_t>(pts.size() + vals.size(), 3))))
    return rc;
  if ((rc = ctx->cr3_out.Reserve(sizeof(double) * 7 * n + sizeof(int32_t) * n))) return rc;
  hipStream_t st = ctx->stream;
  for (int32_t k = 0; k < num_grids; ++k)  // grids another context's stream built
    if (grids[k] && (rc = WaitBuilt(grids[k]->ready, grids[k]->ctx->stream, st))) return rc;
  for (int32_t k = 0; num_intens > 0 && k < ia->num_grids; ++k)
    if (ia->grids[k] && (rc = WaitBuilt(ia->grids[k]->ready, ia->grids[k]->ctx->stream, st)))
      return rc;
  CSM_HIP(hipMemcpyAsync(ctx->cr3_items.ptr, desc.data(), sizeof(Refine3Desc) * n,
                         hipMemcpyHostToDevice, st));
  CSM_HIP(hipMemcpyAsync(ctx->cr3_points.ptr, pts.data(), sizeof(float) * pts.size(),
                         hipMemcpyHostToDevice, st));
  const Refine3Opts o{options->occupied_space_weight_0, options->occupied_space_weight_1,
                      options->translation_weight, options->rotation_weight,
                      options->max_num_iterations, options->use_nonmonotonic_steps ? 1 : 0};
  double* dout = ctx->cr3_out.as<double>();
  int32_t* diters = reinterpret_cast<int32_t*>(dout + 7 * n);
  const Refine3Desc* ditems = ctx->cr3_items.as<Refine3Desc>();
  const float* dpts = ctx->cr3_points.as<float>();
  if (num_plain > 0) {
    hipLaunchKernelGGL(ceres3d_refine<false>, dim3(static_cast<unsigned>(num_plain)),
                       dim3(kR3Threads), 0, st, ditems, dpts, o, dout, diters, nullptr, nullptr);
    CSM_HIP(hipGetLastError());
  }
  if (num_intens > 0) {
    IntensBlock3* dblocks = reinterpret_cast<IntensBlock3*>(ctx->cr3_items.as<char>() + desc_bytes);
    float* dvals = ctx->cr3_points.as<float>() + pts.size();
    CSM_HIP(hipMemcpyAsync(dblocks, blocks.data(), sizeof(IntensBlock3) * num_intens,
                           hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemcpyAsync(dvals, vals.data(), sizeof(float) * vals.size(), hipMemcpyHostToDevice,
                           st));
    hipLaunchKernelGGL(ceres3d_refine<true>, dim3(static_cast<unsigned>(num_intens)),
                       dim3(kR3Threads), 0, st, ditems + num_plain, dpts, o, dout + 7 * num_plain,
                       diters + num_plain, dblocks, dvals);
    CSM_HIP(hipGetLastError());
  }
  std::vector<double> host(7 * static_cast<size_t>(n));
  std::vector<int32_t> host_iters(static_cast<size_t>(n));
  CSM_HIP(hipMemcpyAsync(host.data(), dout, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, st));
  if (iterations)
    CSM_HIP(hipMemcpyAsync(host_iters.data(), diters, sizeof(int32_t) * n, hipMemcpyDeviceToHost,
                           st));
  CSM_HIP(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; ++i) {
    for (int a = 0; a < 3; ++a) out[i].t[a] = host[7 * slot[i] + a];
    for (int a = 0; a < 4; ++a) out[i].q[a] = host[7 * slot[i] + 3 + a];
    if (iterations) iterations[i] = host_iters[slot[i]];
  }
  return CSM_OK;
}

}  // namespace
}  // namespace csm

extern "C" {

int csm_ceres3d_refine_batch(csm_context* ctx, const csm_hybrid_grid* const* grids,
                             int32_t num_grids, const csm_node3d* nodes, int32_t num_nodes,
                             const csm_refine3d* items, int64_t n,
                             const csm_ceres3d_options* options, csm_pose3d* out,
                             int32_t* iterations) {
  return csm::Refine3Batch(ctx, grids, num_grids, nodes, num_nodes, items, n, options, out,
                           iterations, nullptr);
}

int csm_ceres3d_refine_intensity_batch(
    csm_context* ctx, const csm_hybrid_grid* const* grids, int32_t num_grids,
    const csm_intensity_grid* const* intensity_grids, int32_t num_intensity_grids,
    const csm_node3d* nodes, const float* const* node_intensities, int32_t num_nodes,
    const csm_refine3d* items, const int32_t* intensity_grid_of_item, int64_t n,
    const csm_ceres3d_options* options, const csm_ceres3d_intensity_options* intensity_options,
    csm_pose3d* out, int32_t* iterations) {
  if (num_intensity_grids < 0 || (num_intensity_grids > 0 && !intensity_grids))
    return CSM_EINVAL;
  const csm::Intens3Args ia{intensity_grids, num_intensity_grids, node_intensities,
                            intensity_grid_of_item, intensity_options};
  return csm::Refine3Batch(ctx, grids, num_grids, nodes, num_nodes, items, n, options, out,
                           iterations, &ia);
}

int csm_ceres3d_intensity_evaluate(const csm_intensity_grid* grid, const float* points_xyz,
                                   const float* intensities, int32_t n, const double pose[7],
                                   double scaling_factor, float intensity_threshold,
                                   double* residuals, double* jacobian) {
  using namespace csm;
  if (!grid || n < 0 || !pose || (n > 0 && (!points_xyz || !intensities || !residuals || !jacobian)))
    return CSM_EINVAL;
  if (!std::isfinite(scaling_factor) || std::isnan(intensity_threshold)) return CSM_EINVAL;
  for (int a = 0; a < 7; ++a)
    if (!std::isfinite(pose[a])) return CSM_EINVAL;
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(intensities[i]) || !std::isfinite(points_xyz[3 * i]) ||
        !std::isfinite(points_xyz[3 * i + 1]) || !std::isfinite(points_xyz[3 * i + 2]))
      return CSM_EINVAL;
  if (n == 0) return CSM_OK;
  csm_context* ctx = grid->ctx;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  DevBuf din, dout;
  int rc;
  const size_t in_bytes = sizeof(double) * 7 + sizeof(float) * 4 * n;
  if ((rc = din.Reserve(in_bytes)) || (rc = dout.Reserve(sizeof(double) * 7 * n))) return rc;
  std::vector<char> host(in_bytes);
  std::memcpy(host.data(), pose, sizeof(double) * 7);
  std::memcpy(host.data() + sizeof(double) * 7, points_xyz, sizeof(float) * 3 * n);
  std::memcpy(host.data() + sizeof(double) * 7 + sizeof(float) * 3 * n, intensities,
              sizeof(float) * n);
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(din.ptr, host.data(), in_bytes, hipMemcpyHostToDevice, st));
  const double* dpose = din.as<double>();
  const float* dpts = reinterpret_cast<const float*>(dpose + 7);
  const IntensBlock3 block{IntensView3{grid->sum.as<float>(), grid->count.as<int32_t>(),
                                       grid->brick, grid->resolution},
                           0, scaling_factor, 0., intensity_threshold};
  hipLaunchKernelGGL(ceres3d_intensity_eval, dim3(static_cast<unsigned>((n + 255) / 256)),
                     dim3(256), 0, st, block, dpts, dpts + 3 * static_cast<size_t>(n), n, dpose,
                     dout.as<double>(), dout.as<double>() + n);
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(residuals, dout.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipMemcpyAsync(jacobian, dout.as<double>() + n, sizeof(double) * 6 * n,
                         hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

int csm_ceres3d_evaluate(csm_context* ctx, const csm_hybrid_grid* high, const csm_hybrid_grid* low,
                         const csm_node3d* node, const csm_ceres3d_options* options,
                         const double target_translation[3], const double target_rotation[4],
                         const csm_pose3d* pose, double* residuals, double* jacobian,
                         double* sums) {
  using namespace csm;
  if (!ctx || !high || !low || !node || !options || !target_translation || !target_rotation ||
      !pose || !residuals || !jacobian || !sums)
    return CSM_EINVAL;
  if (!(options->occupied_space_weight_0 > 0.) || !(options->occupied_space_weight_1 > 0.) ||
      !(options->translation_weight > 0.) || !(options->rotation_weight > 0.))
    return CSM_EINVAL;
  const int32_t n0 = node->num_high_resolution, n1 = node->num_low_resolution;
  if (n0 <= 0 || n1 <= 0 || !node->high_resolution_xyz || !node->low_resolution_xyz)
    return CSM_EINVAL;
  const csm_hybrid_grid* g[2] = {high, low};
  Refine3Desc d{};
  for (int k = 0; k < 2; ++k) {
    if (!g[k]->ctx || g[k]->ctx->device != ctx->device || !g[k]->prob.ptr) return CSM_EINVAL;
    d.grid[k] = GridView3{g[k]->prob.as<float>(), g[k]->brick, g[k]->resolution};
  }
  d.offset[0] = 0;
  d.offset[1] = n0;
  d.n[0] = n0;
  d.n[1] = n1;
  Quat3 tq;
  for (int a = 0; a < 3; ++a) {
    d.t[a] = pose->t[a];
    d.target[a] = target_translation[a];
    if (!std::isfinite(d.t[a]) || !std::isfinite(d.target[a])) return CSM_EINVAL;
  }
  for (int a = 0; a < 4; ++a) {
    d.q[a] = pose->q[a];
    tq.v[a] = target_rotation[a];
    if (!std::isfinite(d.q[a]) || !std::isfinite(tq.v[a])) return CSM_EINVAL;
  }
  const size_t total = static_cast<size_t>(n0) + static_cast<size_t>(n1);
  std::vector<float> pts(3 * total);
  std::memcpy(pts.data(), node->high_resolution_xyz, sizeof(float) * 3 * n0);
  std::memcpy(pts.data() + 3 * static_cast<size_t>(n0), node->low_resolution_xyz,
              sizeof(float) * 3 * n1);
  for (float v : pts)
    if (!std::isfinite(v)) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  int rc;
  const size_t rows = total + 6;
  if ((rc = ctx->cr3_points.Reserve(sizeof(float) * pts.size())) ||
      (rc = ctx->cr3_out.Reserve(sizeof(double) * (7 * rows + kSums))))
    return rc;
  hipStream_t st = ctx->stream;
  for (int k = 0; k < 2; ++k)
    if ((rc = WaitBuilt(g[k]->ready, g[k]->ctx->stream, st))) return rc;
  CSM_HIP(hipMemcpyAsync(ctx->cr3_points.ptr, pts.data(), sizeof(float) * pts.size(),
                         hipMemcpyHostToDevice, st));
  const Refine3Opts o{options->occupied_space_weight_0, options->occupied_space_weight_1,
                      options->translation_weight, options->rotation_weight,
                      options->max_num_iterations, options->use_nonmonotonic_steps ? 1 : 0};
  double* dres = ctx->cr3_out.as<double>();
  double* djac = dres + rows;
  double* dsums = djac + 6 * rows;
  hipLaunchKernelGGL(ceres3d_evaluate, dim3(1), dim3(kR3Threads), 0, st, d,
                     ctx->cr3_points.as<float>(), o, tq, dres, djac, dsums);
  CSM_HIP(hipGetLastError());
  CSM_HIP(hipMemcpyAsync(residuals, dres, sizeof(double) * rows, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipMemcpyAsync(jacobian, djac, sizeof(double) * 6 * rows, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipMemcpyAsync(sums, dsums, sizeof(double) * kSums, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

int csm_hybrid_grid_get_probability(const csm_hybrid_grid* g, const int32_t* xyz_indices, int64_t n,
                                    float* out) {
  return csm::GridLookup(g, xyz_indices, n, out, csm::grid_probability);
}

int csm_hybrid_grid_interpolate(const csm_hybrid_grid* g, const double* xyz, int64_t n,
                                double* out) {
  return csm::GridLookup(g, xyz, n, out, csm::grid_interpolate);
}

}  // extern "C"
