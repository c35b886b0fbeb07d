// OptimizationProblem2D's solve on the device (csm_pose_graph2d_evaluate,
// csm_pose_graph2d_solve): Ceres 1.13's TrustRegionMinimizer with the
// LevenbergMarquardtStrategy over the SPA cost of every edge, everything in
// double.
//
// The host drives the Levenberg-Marquardt loop (trust_region_minimizer.cc's
// order of checks, StepEvaluator and LmRadius of ceres_lm.h) and reads a few
// doubles per iteration. The device linearises (one thread per edge), forms
// the gradient and the 3x3 diagonal blocks of J'J (one wave per vertex row
// over a vertex -> incident-edge list in edge order), and solves
//   (S J'J S + D^2) y = -S g,  step = S y
// with S the Jacobi column scaling 1 / (1 + |col|) of the first linearisation
// and D^2 = clamp(diag(S J'J S), 1e-6, 1e32) / radius, by conjugate gradients
// preconditioned with the inverse 3x3 vertex blocks. J'J is never formed: a
// product walks the row's edges and rebuilds both Jacobian blocks from the
// six numbers EdgeLin keeps per edge (cos, sin, the two angle derivatives and
// the two weights times sqrt(rho')); keeping both 3x3 blocks instead measured
// a quarter slower.
//
// The Huber corrector has rho'' <= 0, so (corrector.cc) residual and Jacobian
// are scaled by sqrt(rho') and nothing else.
//
// Determinism: no floating-point atomics. A sum over edges or vertices is cut
// into at most kMaxParts contiguous chunks, one workgroup each; a thread adds
// its strided share in index order, a wave adds its lanes by a fixed shuffle
// tree, a workgroup its waves in wave order, and every consumer adds the
// chunks' partial sums the same way. Grid sizes depend on V and E only.
//
// Hang safety: no cooperative launch, no grid-wide barrier, no wait on device
// memory; every device loop is bounded by its row, its chunk or a constant.
// Conjugate-gradient iterations are enqueued kCgBatch at a time, three
// launches each; each launch returns at once when the `done` word of its
// iteration is set, and the host reads that word after every batch. A solve
// therefore makes at most
//   6 + max_num_iterations * (3 * (max_cg_iterations + kCgBatch) + 9)
// launches.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "ceres_lm.h"
#include "csm_internal.h"

namespace csm {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxParts = 1024;
constexpr int kCgBatch = 16;

// Conjugate-gradient outcomes (CgInfo::status).
constexpr int kCgRunning = 0, kCgConverged = 1, kCgBreakdown = 2, kCgFailed = 3;

// One edge at the linearisation point. With c, s of the start angle and
// (dx, dy) = end - start: a = s dx - c dy and b = c dx + s dy are the
// derivatives of the two translation residuals by the start angle. wt, wr
// carry sqrt(rho'), and so does the residual r. The Jacobian blocks are
//   start: wt [c s a; -s c b], wr [0 0 1]    end: wt [-c -s 0; s -c 0], wr [0 0 -1].
struct EdgeLin {
  double c, s, a, b, wt, wr, r0, r1, r2;
};

struct CgInfo {
  int32_t done[2];  // done[k & 1] is read by iteration k, done[(k + 1) & 1] written by it
  int32_t status, iterations;
};

__device__ inline double WaveSum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0
}

__device__ inline double WaveMax(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// The workgroup's sum, on every thread. lds: kWaves doubles.
__device__ inline double BlockSum(double v, double* lds) {
  v = WaveSum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = lds[0];
  for (int i = 1; i < kWaves; ++i) t += lds[i];
  return t;
}

__device__ inline double BlockMax(double v, double* lds) {
  v = WaveMax(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = lds[0];
  for (int i = 1; i < kWaves; ++i) t = fmax(t, lds[i]);
  return t;
}

// The sum of n <= kMaxParts partial sums, the same bits on every thread of
// every workgroup that asks.
__device__ inline double SumParts(const double* parts, int n, double* lds) {
  double v = 0.;
  for (int i = threadIdx.x; i < n; i += kBlock) v += parts[i];
  return BlockSum(v, lds);
}

// This workgroup's chunk [begin, end) of n items cut into gridDim.x chunks.
__device__ inline void Chunk(int64_t n, int64_t* begin, int64_t* end) {
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  *begin = min(n, per * blockIdx.x);
  *end = min(n, *begin + per);
}

// This wave's rows [begin, end) of n rows cut over every wave of the grid.
__device__ inline void WaveRows(int n, int* begin, int* end) {
  const int64_t waves = int64_t{gridDim.x} * kWaves;
  const int64_t per = (n + waves - 1) / waves;
  const int64_t gw = int64_t{blockIdx.x} * kWaves + (threadIdx.x >> 6);
  *begin = static_cast<int>(min(int64_t{n}, per * gw));
  *end = static_cast<int>(min(int64_t{n}, *begin + per));
}

// common::NormalizeAngleDifference (common/math.h): its two loops, bounded; an
// angle further out than the bound allows is first brought back by remainder().
__device__ inline double NormalizeAngleDifference(double d) {
  const double kPi = M_PI;
  if (fabs(d) > 128. * kPi) d = remainder(d, 2. * kPi);
  for (int k = 0; k < 66 && d > kPi; ++k) d -= 2. * kPi;
  for (int k = 0; k < 66 && d < -kPi; ++k) d += 2. * kPi;
  return d;
}

// ComputeUnscaledError and ScaleError (cost_helpers_impl.h:28-56), then
// ceres::HuberLoss and the corrector. Returns rho(|r|^2).
__device__ inline double Linearize(const csm_pose_graph2d_edge& e, const double* poses,
                                   double huber_a, EdgeLin* out, double* raw) {
  const double* ps = poses + 3 * int64_t{e.start};
  const double* pt = poses + 3 * int64_t{e.end};
  const double c = cos(ps[2]), s = sin(ps[2]);
  const double dx = pt[0] - ps[0], dy = pt[1] - ps[1];
  const double h0 = c * dx + s * dy, h1 = -s * dx + c * dy, h2 = pt[2] - ps[2];
  const double u0 = (e.zbar[0] - h0) * e.translation_weight;
  const double u1 = (e.zbar[1] - h1) * e.translation_weight;
  const double u2 = NormalizeAngleDifference(e.zbar[2] - h2) * e.rotation_weight;
  if (raw) {
    raw[0] = u0;
    raw[1] = u1;
    raw[2] = u2;
  }
  const double sq = u0 * u0 + u1 * u1 + u2 * u2;
  double rho = sq, root = 1.;
  if (e.loss == CSM_POSE_GRAPH2D_LOSS_HUBER && sq > huber_a * huber_a) {
    const double r = sqrt(sq);
    rho = 2. * huber_a * r - huber_a * huber_a;
    root = sqrt(fmax(DBL_MIN, huber_a / r));
  }
  if (out) {
    const double wt = e.translation_weight * root, wr = e.rotation_weight * root;
    *out = EdgeLin{c, s, -h1, h0, wt, wr, u0 * root, u1 * root, u2 * root};
  }
  return rho;
}

// One thread per edge: the linearisation (lin and raw may be null) and the
// chunk's share of the cost 1/2 sum rho.
__global__ __launch_bounds__(kBlock) void pg2_linearize(
    const double* __restrict__ poses, const csm_pose_graph2d_edge* __restrict__ edges, int64_t E,
    double huber_a, EdgeLin* __restrict__ lin, double* __restrict__ raw,
    double* __restrict__ cost_parts) {
  __shared__ double lds[kWaves];
  int64_t begin, end;
  Chunk(E, &begin, &end);
  double cost = 0.;
  for (int64_t i = begin + threadIdx.x; i < end; i += kBlock) {
    const csm_pose_graph2d_edge e = edges[i];
    cost += 0.5 * Linearize(e, poses, huber_a, lin ? lin + i : nullptr, raw ? raw + 3 * i : nullptr);
  }
  cost = BlockSum(cost, lds);
  if (threadIdx.x == 0) cost_parts[blockIdx.x] = cost;
}

// J' applied to a 3-vector j of one edge, for the row's end of the edge.
__device__ inline void JtApply(const EdgeLin& L, bool is_end, double j0, double j1, double j2,
                               double* o0, double* o1, double* o2) {
  const double tx = L.wt * (L.c * j0 - L.s * j1), ty = L.wt * (L.s * j0 + L.c * j1);
  if (is_end) {
    *o0 = -tx;
    *o1 = -ty;
    *o2 = -(L.wr * j2);
  } else {
    *o0 = tx;
    *o1 = ty;
    *o2 = L.wt * (L.a * j0 + L.b * j1) + L.wr * j2;
  }
}
// J applied to (qs, qt), the two vertices' 3-vectors.
__device__ inline void JApply(const EdgeLin& L, const double* qs, const double* qt, double* j) {
  const double q0 = qs[0] - qt[0], q1 = qs[1] - qt[1];
  j[0] = L.wt * (L.c * q0 + L.s * q1 + L.a * qs[2]);
  j[1] = L.wt * (-L.s * q0 + L.c * q1 + L.b * qs[2]);
  j[2] = L.wr * (qs[2] - qt[2]);
}
// The edge's share of its vertex's diagonal block of J'J.
__device__ inline void JtJDiagonal(const EdgeLin& L, bool is_end, double* hxx, double* hxt,
                                   double* hyt, double* htt) {
  const double w2 = L.wt * L.wt;
  *hxx += w2;
  if (is_end) {
    *htt += L.wr * L.wr;
  } else {
    *hxt += w2 * (L.c * L.a - L.s * L.b);
    *hyt += w2 * (L.s * L.a + L.c * L.b);
    *htt += w2 * (L.a * L.a + L.b * L.b) + L.wr * L.wr;
  }
}

// One wave per vertex row: g = J' r and the row's diagonal block of J'J, which
// is [hxx 0 hxt; 0 hxx hyt; hxt hyt htt] (H: four doubles per vertex). A
// constant vertex gets zeros. gmax_parts: max |g| per workgroup.
__global__ __launch_bounds__(kBlock) void pg2_gradient(
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ adj,
    const EdgeLin* __restrict__ lin, const uint8_t* __restrict__ constant, int V,
    double* __restrict__ g, double* __restrict__ H, double* __restrict__ gmax_parts) {
  __shared__ double lds[kWaves];
  const int lane = threadIdx.x & 63;
  int begin, end;
  WaveRows(V, &begin, &end);
  double gmax = 0., bad = 0.;
  for (int v = begin; v < end; ++v) {
    double a0 = 0., a1 = 0., a2 = 0., hxx = 0., hxt = 0., hyt = 0., htt = 0.;
    if (!(constant && constant[v])) {
      const int row_end = offsets[v + 1];
      for (int k = offsets[v] + lane; k < row_end; k += 64) {
        const int32_t code = adj[k];
        const EdgeLin L = lin[code >> 1];
        const bool is_end = code & 1;
        double o0, o1, o2;
        JtApply(L, is_end, L.r0, L.r1, L.r2, &o0, &o1, &o2);
        a0 += o0;
        a1 += o1;
        a2 += o2;
        JtJDiagonal(L, is_end, &hxx, &hxt, &hyt, &htt);
      }
    }
    a0 = WaveSum(a0);
    a1 = WaveSum(a1);
    a2 = WaveSum(a2);
    hxx = WaveSum(hxx);
    hxt = WaveSum(hxt);
    hyt = WaveSum(hyt);
    htt = WaveSum(htt);
    if (lane == 0) {
      g[3 * int64_t{v}] = a0;
      g[3 * int64_t{v} + 1] = a1;
      g[3 * int64_t{v} + 2] = a2;
      H[4 * int64_t{v}] = hxx;
      H[4 * int64_t{v} + 1] = hxt;
      H[4 * int64_t{v} + 2] = hyt;
      H[4 * int64_t{v} + 3] = htt;
      gmax = fmax(gmax, fmax(fabs(a0), fmax(fabs(a1), fabs(a2))));
      // fmax drops a NaN: carry it in a sum, so that a non-finite gradient is seen.
      const double sum = a0 + a1 + a2;
      if (sum != sum) bad = sum;
    }
  }
  gmax = BlockMax(gmax, lds);
  bad = BlockSum(bad, lds);
  if (threadIdx.x == 0) gmax_parts[blockIdx.x] = (bad != bad) ? bad : gmax;
}

// Jacobi scaling of trust_region_minimizer.cc: 1 / (1 + sqrt(|col|^2)).
__global__ __launch_bounds__(kBlock) void pg2_jacobi_scale(const double* __restrict__ H, int V,
                                                          double* __restrict__ scale) {
  const int v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= V) return;
  const double sx = 1. / (1. + sqrt(H[4 * int64_t{v}]));
  scale[3 * int64_t{v}] = sx;
  scale[3 * int64_t{v} + 1] = sx;
  scale[3 * int64_t{v} + 2] = 1. / (1. + sqrt(H[4 * int64_t{v} + 3]));
}

// Start of one linear solve, one thread per vertex: the Levenberg-Marquardt
// diagonal dd (levenberg_marquardt_strategy.cc), the inverse of the vertex's
// block of S J'J S + D^2 (six doubles, symmetric; zeros for a constant
// vertex), and y = 0, r = b = -S g, z = M^-1 r, p = z with the chunk's shares
// of r.z and r.r.
__global__ __launch_bounds__(kBlock) void pg2_cg_init(
    const double* __restrict__ g, const double* __restrict__ H, const double* __restrict__ scale,
    const uint8_t* __restrict__ constant, int V, double radius, double* __restrict__ dd,
    double* __restrict__ Minv, double* __restrict__ y, double* __restrict__ r,
    double* __restrict__ z, double* __restrict__ p, double* __restrict__ rz_parts,
    double* __restrict__ rr0_parts, CgInfo* __restrict__ info) {
  __shared__ double lds[kWaves];
  int64_t begin, end;
  Chunk(V, &begin, &end);
  double rz = 0., rr = 0.;
  for (int64_t v = begin + threadIdx.x; v < end; v += kBlock) {
    double mi[6] = {0., 0., 0., 0., 0., 0.}, d[3] = {0., 0., 0.}, b[3] = {0., 0., 0.};
    if (!constant[v]) {
      const double s0 = scale[3 * v], s2 = scale[3 * v + 2];
      const double hxx = s0 * s0 * H[4 * v], htt = s2 * s2 * H[4 * v + 3];
      d[0] = d[1] = fmin(fmax(hxx, 1e-6), 1e32) / radius;
      d[2] = fmin(fmax(htt, 1e-6), 1e32) / radius;
      const double m = hxx + d[0], t = htt + d[2];
      const double u = s0 * s2 * H[4 * v + 1], w = s0 * s2 * H[4 * v + 2];
      const double det = m * (m * t - u * u - w * w);
      if (det > 0. && det <= DBL_MAX) {
        // Cofactors of [m 0 u; 0 m w; u w t]: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).
        mi[0] = (m * t - w * w) / det;
        mi[1] = (u * w) / det;
        mi[2] = -(m * u) / det;
        mi[3] = (m * t - u * u) / det;
        mi[4] = -(m * w) / det;
        mi[5] = (m * m) / det;
      } else {
        mi[0] = mi[3] = 1. / m;
        mi[5] = 1. / t;
      }
      for (int i = 0; i < 3; ++i) b[i] = -(scale[3 * v + i] * g[3 * v + i]);
    }
    const double z0 = mi[0] * b[0] + mi[1] * b[1] + mi[2] * b[2];
    const double z1 = mi[1] * b[0] + mi[3] * b[1] + mi[4] * b[2];
    const double z2 = mi[2] * b[0] + mi[4] * b[1] + mi[5] * b[2];
    for (int i = 0; i < 6; ++i) Minv[6 * v + i] = mi[i];
    for (int i = 0; i < 3; ++i) {
      dd[3 * v + i] = d[i];
      y[3 * v + i] = 0.;
      r[3 * v + i] = b[i];
    }
    z[3 * v] = p[3 * v] = z0;
    z[3 * v + 1] = p[3 * v + 1] = z1;
    z[3 * v + 2] = p[3 * v + 2] = z2;
    rz += b[0] * z0 + b[1] * z1 + b[2] * z2;
    rr += b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  }
  rz = BlockSum(rz, lds);
  rr = BlockSum(rr, lds);
  if (threadIdx.x == 0) {
    rz_parts[blockIdx.x] = rz;
    rr0_parts[blockIdx.x] = rr;
    if (blockIdx.x == 0) *info = CgInfo{{0, 0}, kCgRunning, 0};
  }
}

// Ap = (S J'J S + D^2) p, one wave per vertex row, and the workgroup's share
// of p.Ap. Iteration k of the solve.
__global__ __launch_bounds__(kBlock) void pg2_cg_product(
    int k, const CgInfo* __restrict__ info, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ adj, const csm_pose_graph2d_edge* __restrict__ edges,
    const EdgeLin* __restrict__ lin, const double* __restrict__ scale,
    const double* __restrict__ dd, const uint8_t* __restrict__ constant,
    const double* __restrict__ p, int V, double* __restrict__ Ap, double* __restrict__ pap_parts) {
  __shared__ double lds[kWaves];
  if (info->done[k & 1]) return;
  const int lane = threadIdx.x & 63;
  int begin, end;
  WaveRows(V, &begin, &end);
  double pap = 0.;
  for (int v = begin; v < end; ++v) {
    double a0 = 0., a1 = 0., a2 = 0.;
    const bool fixed = constant[v];
    if (!fixed) {
      const int row_end = offsets[v + 1];
      for (int k2 = offsets[v] + lane; k2 < row_end; k2 += 64) {
        const int32_t code = adj[k2];
        const int32_t e = code >> 1;
        const EdgeLin L = lin[e];
        const int64_t vs = edges[e].start, vt = edges[e].end;
        double qs[3], qt[3], j[3];
        for (int i = 0; i < 3; ++i) {
          qs[i] = scale[3 * vs + i] * p[3 * vs + i];
          qt[i] = scale[3 * vt + i] * p[3 * vt + i];
        }
        JApply(L, qs, qt, j);
        double o0, o1, o2;
        JtApply(L, code & 1, j[0], j[1], j[2], &o0, &o1, &o2);
        a0 += o0;
        a1 += o1;
        a2 += o2;
      }
    }
    a0 = WaveSum(a0);
    a1 = WaveSum(a1);
    a2 = WaveSum(a2);
    if (lane == 0) {
      const int64_t i = 3 * int64_t{v};
      double r0 = 0., r1 = 0., r2 = 0.;
      if (!fixed) {
        r0 = scale[i] * a0 + dd[i] * p[i];
        r1 = scale[i + 1] * a1 + dd[i + 1] * p[i + 1];
        r2 = scale[i + 2] * a2 + dd[i + 2] * p[i + 2];
      }
      Ap[i] = r0;
      Ap[i + 1] = r1;
      Ap[i + 2] = r2;
      pap += p[i] * r0 + p[i + 1] * r1 + p[i + 2] * r2;
    }
  }
  pap = BlockSum(pap, lds);
  if (threadIdx.x == 0) pap_parts[blockIdx.x] = pap;
}

__device__ inline bool BadCurvature(double pap) { return !(pap > 0.) || !(pap <= DBL_MAX); }

// y += alpha p, r -= alpha Ap, z = M^-1 r, with the chunk's shares of r.z and
// r.r. Nothing moves when p.Ap is not a positive finite number.
__global__ __launch_bounds__(kBlock) void pg2_cg_update(
    int k, const CgInfo* __restrict__ info, int V, int row_parts, const double* __restrict__ p,
    const double* __restrict__ Ap, const double* __restrict__ Minv,
    const double* __restrict__ pap_parts, double* __restrict__ rz_parts /* 2 x kMaxParts */,
    double* __restrict__ rr_parts, double* __restrict__ y, double* __restrict__ r,
    double* __restrict__ z) {
  __shared__ double lds[kWaves];
  if (info->done[k & 1]) return;
  const double rz_old = SumParts(rz_parts + (k & 1) * kMaxParts, gridDim.x, lds);
  const double pap = SumParts(pap_parts, row_parts, lds);
  if (BadCurvature(pap)) return;
  const double alpha = rz_old / pap;
  int64_t begin, end;
  Chunk(V, &begin, &end);
  double rz = 0., rr = 0.;
  for (int64_t v = begin + threadIdx.x; v < end; v += kBlock) {
    double rn[3];
    for (int i = 0; i < 3; ++i) {
      y[3 * v + i] += alpha * p[3 * v + i];
      rn[i] = r[3 * v + i] - alpha * Ap[3 * v + i];
      r[3 * v + i] = rn[i];
    }
    const double* mi = Minv + 6 * v;
    const double z0 = mi[0] * rn[0] + mi[1] * rn[1] + mi[2] * rn[2];
    const double z1 = mi[1] * rn[0] + mi[3] * rn[1] + mi[4] * rn[2];
    const double z2 = mi[2] * rn[0] + mi[4] * rn[1] + mi[5] * rn[2];
    z[3 * v] = z0;
    z[3 * v + 1] = z1;
    z[3 * v + 2] = z2;
    rz += rn[0] * z0 + rn[1] * z1 + rn[2] * z2;
    rr += rn[0] * rn[0] + rn[1] * rn[1] + rn[2] * rn[2];
  }
  rz = BlockSum(rz, lds);
  rr = BlockSum(rr, lds);
  if (threadIdx.x == 0) {
    rz_parts[((k + 1) & 1) * kMaxParts + blockIdx.x] = rz;
    rr_parts[blockIdx.x] = rr;
  }
}

// The end of iteration k: stop (and say why) or p = z + beta p. Every
// workgroup reaches the same decision from the same partial sums; workgroup 0
// records it.
__global__ __launch_bounds__(kBlock) void pg2_cg_direction(
    int k, CgInfo* __restrict__ info, int V, int row_parts, double tolerance,
    const double* __restrict__ pap_parts, const double* __restrict__ rz_parts,
    const double* __restrict__ rr_parts, const double* __restrict__ rr0_parts,
    const double* __restrict__ z, double* __restrict__ p) {
  __shared__ double lds[kWaves];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (info->done[k & 1]) {
    if (writer) info->done[(k + 1) & 1] = 1;
    return;
  }
  const double pap = SumParts(pap_parts, row_parts, lds);
  int status = kCgRunning, iterations = k + 1;
  double beta = 0.;
  if (BadCurvature(pap)) {
    status = k == 0 ? kCgFailed : kCgBreakdown;
    iterations = k;
  } else {
    const double rz_old = SumParts(rz_parts + (k & 1) * kMaxParts, gridDim.x, lds);
    const double rz_new = SumParts(rz_parts + ((k + 1) & 1) * kMaxParts, gridDim.x, lds);
    const double rr = SumParts(rr_parts, gridDim.x, lds);
    const double rr0 = SumParts(rr0_parts, gridDim.x, lds);
    if (!(rr <= DBL_MAX)) {
      status = kCgFailed;  // the iterate is no longer finite
    } else if (sqrt(rr) <= tolerance * sqrt(rr0)) {
      status = kCgConverged;
    } else {
      beta = rz_new / rz_old;
    }
  }
  if (writer) {
    info->done[(k + 1) & 1] = status != kCgRunning;
    info->status = status;
    info->iterations = iterations;
  }
  if (status != kCgRunning) return;
  int64_t begin, end;
  Chunk(V, &begin, &end);
  for (int64_t i = 3 * begin + threadIdx.x; i < 3 * end; i += kBlock) p[i] = z[i] + beta * p[i];
}

// delta = S y and the candidate x + delta, with the chunk's shares of
// |delta|^2 and |x|^2 over the variable vertices.
__global__ __launch_bounds__(kBlock) void pg2_candidate(
    const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ scale,
    const uint8_t* __restrict__ constant, int V, double* __restrict__ delta,
    double* __restrict__ candidate, double* __restrict__ step_parts,
    double* __restrict__ x_parts) {
  __shared__ double lds[kWaves];
  int64_t begin, end;
  Chunk(V, &begin, &end);
  double step = 0., xx = 0.;
  for (int64_t v = begin + threadIdx.x; v < end; v += kBlock) {
    const bool fixed = constant[v];
    for (int i = 0; i < 3; ++i) {
      const double xi = x[3 * v + i];
      const double d = fixed ? 0. : scale[3 * v + i] * y[3 * v + i];
      delta[3 * v + i] = d;
      candidate[3 * v + i] = fixed ? xi : xi + d;
      step += d * d;
      if (!fixed) xx += xi * xi;
    }
  }
  step = BlockSum(step, lds);
  xx = BlockSum(xx, lds);
  if (threadIdx.x == 0) {
    step_parts[blockIdx.x] = step;
    x_parts[blockIdx.x] = xx;
  }
}

// The model's cost change -(J delta)'(r + J delta / 2), one thread per edge.
__global__ __launch_bounds__(kBlock) void pg2_model_change(
    const csm_pose_graph2d_edge* __restrict__ edges, const EdgeLin* __restrict__ lin,
    const double* __restrict__ delta, int64_t E, double* __restrict__ parts) {
  __shared__ double lds[kWaves];
  int64_t begin, end;
  Chunk(E, &begin, &end);
  double sum = 0.;
  for (int64_t i = begin + threadIdx.x; i < end; i += kBlock) {
    const EdgeLin L = lin[i];
    const double* ds = delta + 3 * int64_t{edges[i].start};
    const double* dt = delta + 3 * int64_t{edges[i].end};
    double m[3];
    JApply(L, ds, dt, m);
    sum -= m[0] * (L.r0 + m[0] / 2.) + m[1] * (L.r1 + m[1] / 2.) + m[2] * (L.r2 + m[2] / 2.);
  }
  sum = BlockSum(sum, lds);
  if (threadIdx.x == 0) parts[blockIdx.x] = sum;
}

// One workgroup: out[i] = the sum (or, is_max, the maximum; a NaN part wins)
// of parts[i][0 .. n[i]).
struct Reduce4 {
  const double* parts[4];
  int n[4];
  int is_max[4];
  int count;
};
__global__ __launch_bounds__(kBlock) void pg2_reduce(Reduce4 a, double* __restrict__ out) {
  __shared__ double lds[kWaves];
  for (int i = 0; i < a.count; ++i) {
    double v;
    if (a.is_max[i]) {
      double m = 0., bad = 0.;
      for (int j = threadIdx.x; j < a.n[i]; j += kBlock) {
        const double x = a.parts[i][j];
        if (x != x) bad = x;
        m = fmax(m, x);
      }
      m = BlockMax(m, lds);
      bad = BlockSum(bad, lds);
      v = bad != bad ? bad : m;
    } else {
      v = SumParts(a.parts[i], a.n[i], lds);
    }
    if (threadIdx.x == 0) out[i] = v;
  }
}

int PartsFor(int64_t n) {
  return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(kMaxParts, (n + kBlock - 1) / kBlock)));
}
int RowPartsFor(int V) {
  return std::max(1, std::min(kMaxParts, (V + kWaves - 1) / kWaves));
}

bool Finite(double v) { return std::isfinite(v); }

// The checks that come before anything is enqueued.
int Validate(const csm_pose_graph2d_options* o, const double* poses, int32_t V,
             const csm_pose_graph2d_edge* edges, int64_t E) {
  if (!o || V < 0 || E < 0 || (V > 0 && !poses) || (E > 0 && !edges)) return CSM_EINVAL;
  if (V > CSM_POSE_GRAPH2D_MAX_VERTICES || E > CSM_POSE_GRAPH2D_MAX_EDGES) return CSM_ERANGE;
  if (!(o->huber_scale > 0.) || !Finite(o->huber_scale)) return CSM_EINVAL;
  if (o->max_num_iterations < 0 || o->max_cg_iterations < 1) return CSM_EINVAL;
  if (o->max_num_iterations > CSM_POSE_GRAPH2D_MAX_LM_ITERATIONS ||
      o->max_cg_iterations > CSM_POSE_GRAPH2D_MAX_CG_ITERATIONS)
    return CSM_ERANGE;
  if (!(o->cg_relative_tolerance > 0.) || !Finite(o->cg_relative_tolerance)) return CSM_EINVAL;
  for (int64_t i = 0; i < 3 * int64_t{V}; ++i)
    if (!Finite(poses[i])) return CSM_EINVAL;
  for (int64_t i = 0; i < E; ++i) {
    const csm_pose_graph2d_edge& e = edges[i];
    if (e.start < 0 || e.start >= V || e.end < 0 || e.end >= V || e.start == e.end)
      return CSM_EINVAL;
    if (!Finite(e.zbar[0]) || !Finite(e.zbar[1]) || !Finite(e.zbar[2]) ||
        !Finite(e.translation_weight) || !Finite(e.rotation_weight))
      return CSM_EINVAL;
    if (e.loss != CSM_POSE_GRAPH2D_LOSS_NONE && e.loss != CSM_POSE_GRAPH2D_LOSS_HUBER)
      return CSM_EINVAL;
  }
  return CSM_OK;
}

// The device arena of one call, carved from ctx->pg2_dev.
struct Arena {
  char* base = nullptr;
  size_t used = 0;
  template <typename T>
  T* Take(size_t count) {
    used = (used + 255) & ~size_t{255};
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += count * sizeof(T);
    return p;
  }
};

struct Buffers {
  double *x, *cand, *best, *g, *H, *scale, *dd, *Minv, *y, *r, *z, *p, *Ap, *delta, *raw;
  uint8_t* constant;
  csm_pose_graph2d_edge *edges, *fixed_edges;
  EdgeLin* lin;
  int32_t *offsets, *adj;
  double *cost_parts, *gmax_parts, *rz_parts, *rr_parts, *rr0_parts, *pap_parts, *step_parts,
      *x_parts, *model_parts, *out;
  CgInfo* info;
};

void Carve(Arena* a, int64_t V, int64_t E, int64_t F, bool solve, bool raw, Buffers* b) {
  const size_t v3 = 3 * static_cast<size_t>(V), e = static_cast<size_t>(E);
  b->x = a->Take<double>(v3);
  b->g = a->Take<double>(v3);
  b->H = a->Take<double>(4 * static_cast<size_t>(V));
  b->edges = a->Take<csm_pose_graph2d_edge>(e);
  b->lin = a->Take<EdgeLin>(e);
  b->offsets = a->Take<int32_t>(static_cast<size_t>(V) + 1);
  b->adj = a->Take<int32_t>(2 * e);
  b->cost_parts = a->Take<double>(kMaxParts);
  b->gmax_parts = a->Take<double>(kMaxParts);
  b->out = a->Take<double>(8);
  b->raw = raw ? a->Take<double>(3 * e) : nullptr;
  if (!solve) return;
  b->cand = a->Take<double>(v3);
  b->best = a->Take<double>(v3);
  b->scale = a->Take<double>(v3);
  b->dd = a->Take<double>(v3);
  b->Minv = a->Take<double>(6 * static_cast<size_t>(V));
  b->y = a->Take<double>(v3);
  b->r = a->Take<double>(v3);
  b->z = a->Take<double>(v3);
  b->p = a->Take<double>(v3);
  b->Ap = a->Take<double>(v3);
  b->delta = a->Take<double>(v3);
  b->constant = a->Take<uint8_t>(static_cast<size_t>(V));
  b->rz_parts = a->Take<double>(2 * kMaxParts);
  b->rr_parts = a->Take<double>(kMaxParts);
  b->rr0_parts = a->Take<double>(kMaxParts);
  b->pap_parts = a->Take<double>(kMaxParts);
  b->step_parts = a->Take<double>(kMaxParts);
  b->x_parts = a->Take<double>(kMaxParts);
  b->model_parts = a->Take<double>(kMaxParts);
  b->info = a->Take<CgInfo>(1);
  b->fixed_edges = a->Take<csm_pose_graph2d_edge>(static_cast<size_t>(F));
}

int Reserve(csm_context* ctx, int64_t V, int64_t E, int64_t F, bool solve, bool raw, Buffers* b) {
  Arena size;
  Carve(&size, V, E, F, solve, raw, b);
  int rc;
  if ((rc = ctx->pg2_dev.Reserve(size.used + 256))) return rc;
  if ((rc = ctx->pg2_host.Reserve(256))) return rc;
  Arena a;
  a.base = ctx->pg2_dev.as<char>();
  Carve(&a, V, E, F, solve, raw, b);
  return CSM_OK;
}

// The vertex -> incident-edge list in edge order: entry 2 e + (1 for e's end).
void BuildAdjacency(int32_t V, const csm_pose_graph2d_edge* edges, int64_t E,
                    std::vector<int32_t>* offsets, std::vector<int32_t>* adj) {
  offsets->assign(static_cast<size_t>(V) + 1, 0);
  for (int64_t i = 0; i < E; ++i) {
    ++(*offsets)[edges[i].start + 1];
    ++(*offsets)[edges[i].end + 1];
  }
  for (int32_t v = 0; v < V; ++v) (*offsets)[v + 1] += (*offsets)[v];
  adj->resize(2 * static_cast<size_t>(E));
  std::vector<int32_t> at(offsets->begin(), offsets->end() - 1);
  for (int64_t i = 0; i < E; ++i) {
    (*adj)[at[edges[i].start]++] = static_cast<int32_t>(2 * i);
    (*adj)[at[edges[i].end]++] = static_cast<int32_t>(2 * i + 1);
  }
}

int Upload(csm_context* ctx, const Buffers& b, const double* poses, int32_t V,
           const csm_pose_graph2d_edge* edges, int64_t E) {
  std::vector<int32_t> offsets, adj;
  BuildAdjacency(V, edges, E, &offsets, &adj);
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(b.x, poses, 24 * static_cast<size_t>(V), hipMemcpyHostToDevice, st));
  if (E > 0) {
    CSM_HIP(hipMemcpyAsync(b.edges, edges, sizeof(csm_pose_graph2d_edge) * static_cast<size_t>(E),
                           hipMemcpyHostToDevice, st));
    CSM_HIP(hipMemcpyAsync(b.adj, adj.data(), 4 * adj.size(), hipMemcpyHostToDevice, st));
  }
  CSM_HIP(hipMemcpyAsync(b.offsets, offsets.data(), 4 * offsets.size(), hipMemcpyHostToDevice, st));
  // The vectors go out of scope on return.
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

// Linearises at `x` and leaves (cost, max |g|) in out[0..2) on the host.
int LinearizeAt(csm_context* ctx, const Buffers& b, const double* x, const uint8_t* constant,
                int32_t V, int64_t E, double huber, double* raw, double* out2) {
  hipStream_t st = ctx->stream;
  const int ep = PartsFor(E), rp = RowPartsFor(V);
  hipLaunchKernelGGL(pg2_linearize, dim3(ep), dim3(kBlock), 0, st, x, b.edges, E, huber, b.lin,
                     raw, b.cost_parts);
  hipLaunchKernelGGL(pg2_gradient, dim3(rp), dim3(kBlock), 0, st, b.offsets, b.adj, b.lin,
                     constant, V, b.g, b.H, b.gmax_parts);
  Reduce4 red{};
  red.parts[0] = b.cost_parts;
  red.n[0] = ep;
  red.parts[1] = b.gmax_parts;
  red.n[1] = rp;
  red.is_max[1] = 1;
  red.count = 2;
  hipLaunchKernelGGL(pg2_reduce, dim3(1), dim3(kBlock), 0, st, red, b.out);
  CSM_HIP(hipGetLastError());
  double* host = ctx->pg2_host.as<double>();
  CSM_HIP(hipMemcpyAsync(host, b.out, 16, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  out2[0] = host[0];
  out2[1] = host[1];
  return CSM_OK;
}

// One linear solve at the current linearisation. status: CgInfo's.
int SolveStep(csm_context* ctx, const Buffers& b, int32_t V, double radius,
              const csm_pose_graph2d_options& o, int* status, int* iterations) {
  hipStream_t st = ctx->stream;
  const int vp = PartsFor(V), rp = RowPartsFor(V);
  hipLaunchKernelGGL(pg2_cg_init, dim3(vp), dim3(kBlock), 0, st, b.g, b.H, b.scale, b.constant, V,
                     radius, b.dd, b.Minv, b.y, b.r, b.z, b.p, b.rz_parts, b.rr0_parts, b.info);
  CgInfo* host = reinterpret_cast<CgInfo*>(ctx->pg2_host.as<char>() + 64);
  *status = kCgRunning;
  *iterations = 0;
  for (int k = 0; k < o.max_cg_iterations;) {
    const int batch_end = std::min(o.max_cg_iterations, k + kCgBatch);
    for (; k < batch_end; ++k) {
      hipLaunchKernelGGL(pg2_cg_product, dim3(rp), dim3(kBlock), 0, st, k, b.info, b.offsets,
                         b.adj, b.edges, b.lin, b.scale, b.dd, b.constant, b.p, V, b.Ap,
                         b.pap_parts);
      hipLaunchKernelGGL(pg2_cg_update, dim3(vp), dim3(kBlock), 0, st, k, b.info, V, rp, b.p, b.Ap,
                         b.Minv, b.pap_parts, b.rz_parts, b.rr_parts, b.y, b.r, b.z);
      hipLaunchKernelGGL(pg2_cg_direction, dim3(vp), dim3(kBlock), 0, st, k, b.info, V, rp,
                         o.cg_relative_tolerance, b.pap_parts, b.rz_parts, b.rr_parts,
                         b.rr0_parts, b.z, b.p);
    }
    CSM_HIP(hipGetLastError());
    CSM_HIP(hipMemcpyAsync(host, b.info, sizeof(CgInfo), hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    *status = host->status;
    *iterations = host->iterations;
    if (host->done[k & 1]) break;
  }
  return CSM_OK;
}

double Seconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace
}  // namespace csm

extern "C" {

void csm_pose_graph2d_default_options(csm_pose_graph2d_options* out) {
  if (!out) return;
  *out = csm_pose_graph2d_options{10., 50, 0, 500, 0, 1e-8};
}

int csm_pose_graph2d_evaluate(csm_context* ctx, const csm_pose_graph2d_options* options,
                              const double* poses, int32_t num_vertices,
                              const csm_pose_graph2d_edge* edges, int64_t num_edges, double* cost,
                              double* residuals, double* gradient) {
  using namespace csm;
  if (!ctx || !cost) return CSM_EINVAL;
  const int32_t V = num_vertices;
  const int64_t E = num_edges;
  int rc;
  if ((rc = Validate(options, poses, V, edges, E))) return rc;
  if (E == 0) {
    *cost = 0.;
    if (gradient) std::memset(gradient, 0, 24 * static_cast<size_t>(V));
    return CSM_OK;
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  Buffers b{};
  if ((rc = Reserve(ctx, V, E, 0, false, residuals != nullptr, &b))) return rc;
  if ((rc = Upload(ctx, b, poses, V, edges, E))) return rc;
  double out2[2];
  if ((rc = LinearizeAt(ctx, b, b.x, nullptr, V, E, options->huber_scale, b.raw, out2))) return rc;
  *cost = out2[0];
  hipStream_t st = ctx->stream;
  if (residuals)
    CSM_HIP(hipMemcpyAsync(residuals, b.raw, 24 * static_cast<size_t>(E), hipMemcpyDeviceToHost, st));
  if (gradient)
    CSM_HIP(hipMemcpyAsync(gradient, b.g, 24 * static_cast<size_t>(V), hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

int csm_pose_graph2d_solve(csm_context* ctx, const csm_pose_graph2d_options* options,
                           double* poses_inout, const uint8_t* constant, int32_t num_vertices,
                           const csm_pose_graph2d_edge* edges, int64_t num_edges,
                           csm_pose_graph2d_summary* summary) {
  using namespace csm;
  if (!ctx || !summary) return CSM_EINVAL;
  const int32_t V = num_vertices;
  int rc;
  if ((rc = Validate(options, poses_inout, V, edges, num_edges))) return rc;
  const csm_pose_graph2d_options o = *options;
  *summary = csm_pose_graph2d_summary{};
  summary->termination = CSM_POSE_GRAPH2D_CONVERGENCE_GRADIENT;
  bool any_variable = false;
  for (int32_t v = 0; v < V && !any_variable; ++v) any_variable = !(constant && constant[v]);
  if (num_edges == 0 || !any_variable) return CSM_OK;

  // A residual block whose two vertices are constant is no part of the
  // minimised problem (Ceres removes it and reports its cost as fixed_cost):
  // it is evaluated once and added to both reported costs.
  std::vector<csm_pose_graph2d_edge> active, fixed;
  if (constant) {
    int64_t num_fixed = 0;
    for (int64_t i = 0; i < num_edges; ++i)
      num_fixed += constant[edges[i].start] && constant[edges[i].end];
    if (num_fixed > 0) {
      active.reserve(static_cast<size_t>(num_edges - num_fixed));
      fixed.reserve(static_cast<size_t>(num_fixed));
      for (int64_t i = 0; i < num_edges; ++i)
        (constant[edges[i].start] && constant[edges[i].end] ? fixed : active).push_back(edges[i]);
      edges = active.data();
    }
  }
  const int64_t E = num_edges - static_cast<int64_t>(fixed.size());
  const int64_t F = static_cast<int64_t>(fixed.size());

  std::lock_guard<std::mutex> lock(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return CSM_EHIP;
  double* phase = ctx->pg2_phase_seconds;
  phase[0] = phase[1] = phase[2] = phase[3] = 0.;
  double t0 = Seconds();
  Buffers b{};
  if ((rc = Reserve(ctx, V, E, F, true, false, &b))) return rc;
  if ((rc = Upload(ctx, b, poses_inout, V, edges, E))) return rc;
  hipStream_t st = ctx->stream;
  double* host = ctx->pg2_host.as<double>();
  if (constant) {
    CSM_HIP(hipMemcpyAsync(b.constant, constant, static_cast<size_t>(V), hipMemcpyHostToDevice, st));
    CSM_HIP(hipStreamSynchronize(st));
  } else {
    CSM_HIP(hipMemsetAsync(b.constant, 0, static_cast<size_t>(V), st));
  }
  double fixed_cost = 0.;
  if (F > 0) {
    CSM_HIP(hipMemcpyAsync(b.fixed_edges, fixed.data(), sizeof(csm_pose_graph2d_edge) * fixed.size(),
                           hipMemcpyHostToDevice, st));
    const int fp = PartsFor(F);
    hipLaunchKernelGGL(pg2_linearize, dim3(fp), dim3(kBlock), 0, st, b.x, b.fixed_edges, F,
                       o.huber_scale, static_cast<EdgeLin*>(nullptr), static_cast<double*>(nullptr),
                       b.cost_parts);
    Reduce4 red{};
    red.parts[0] = b.cost_parts;
    red.n[0] = fp;
    red.count = 1;
    hipLaunchKernelGGL(pg2_reduce, dim3(1), dim3(kBlock), 0, st, red, b.out);
    CSM_HIP(hipGetLastError());
    CSM_HIP(hipMemcpyAsync(host, b.out, 8, hipMemcpyDeviceToHost, st));
    CSM_HIP(hipStreamSynchronize(st));
    fixed_cost = host[0];
  }
  phase[0] = Seconds() - t0;
  if (E == 0) {
    // Variable vertices, but no residual reaches them.
    summary->initial_cost = summary->final_cost = fixed_cost;
    return CSM_OK;
  }

  // trust_region_minimizer.cc: Init, then IterationZero.
  t0 = Seconds();
  double* x = b.x;
  double* candidate = b.cand;
  double lin[2];
  if ((rc = LinearizeAt(ctx, b, x, b.constant, V, E, o.huber_scale, nullptr, lin))) return rc;
  hipLaunchKernelGGL(pg2_jacobi_scale, dim3((V + kBlock - 1) / kBlock), dim3(kBlock), 0, st, b.H, V,
                     b.scale);
  CSM_HIP(hipGetLastError());
  phase[1] += Seconds() - t0;
  double cost = lin[0], gradient_max = lin[1];
  summary->initial_cost = summary->final_cost = cost + fixed_cost;
  if (!std::isfinite(cost) || !std::isfinite(gradient_max)) {
    summary->termination = CSM_POSE_GRAPH2D_FAILURE;
    return CSM_OK;
  }

  const double kFunctionTolerance = 1e-6, kGradientTolerance = 1e-10, kParameterTolerance = 1e-8;
  const double kMinRelativeDecrease = 1e-3, kMinRadius = 1e-32;
  const int kMaxInvalidSteps = 5;
  StepEvaluator evaluator(cost, o.use_nonmonotonic_steps != 0);
  LmRadius lm;
  // With non-monotonic steps an accepted step may raise the cost: the answer
  // is the cheapest point visited, kept in b.best (null: the current point).
  const double* best = nullptr;
  double minimum_cost = cost;
  int invalid_steps = 0, termination = -1, iteration = 0;
  const int ep = PartsFor(E), vp = PartsFor(V);
  // FinalizeIterationAndCheckIfMinimizerCanContinue, then one iteration.
  while (termination < 0) {
    // IterationZero tests the gradient before anything else; later iterations
    // test the iteration limit first.
    if (iteration > 0 && iteration >= o.max_num_iterations) {
      termination = CSM_POSE_GRAPH2D_NO_CONVERGENCE;
      break;
    }
    if (gradient_max <= kGradientTolerance) {
      termination = CSM_POSE_GRAPH2D_CONVERGENCE_GRADIENT;
      break;
    }
    if (iteration >= o.max_num_iterations) {
      termination = CSM_POSE_GRAPH2D_NO_CONVERGENCE;
      break;
    }
    if (lm.radius < kMinRadius) {
      // "Minimum trust region radius reached", a convergence: no step fits.
      termination = CSM_POSE_GRAPH2D_CONVERGENCE_PARAMETER;
      break;
    }
    ++iteration;
    t0 = Seconds();
    int cg_status, cg_iterations;
    if ((rc = SolveStep(ctx, b, V, lm.radius, o, &cg_status, &cg_iterations))) return rc;
    phase[2] += Seconds() - t0;
    summary->num_cg_iterations += cg_iterations;
    if (cg_status == kCgRunning) ++summary->num_cg_capped_steps;

    t0 = Seconds();
    bool valid = cg_status != kCgFailed;
    double model_change = 0., candidate_cost = 0., step_norm = 0., x_norm = 0.;
    if (valid) {
      hipLaunchKernelGGL(pg2_candidate, dim3(vp), dim3(kBlock), 0, st, x, b.y, b.scale,
                         b.constant, V, b.delta, candidate, b.step_parts, b.x_parts);
      hipLaunchKernelGGL(pg2_model_change, dim3(ep), dim3(kBlock), 0, st, b.edges, b.lin, b.delta,
                         E, b.model_parts);
      hipLaunchKernelGGL(pg2_linearize, dim3(ep), dim3(kBlock), 0, st, candidate, b.edges, E,
                         o.huber_scale, static_cast<EdgeLin*>(nullptr),
                         static_cast<double*>(nullptr), b.cost_parts);
      Reduce4 red{};
      const double* parts[4] = {b.model_parts, b.cost_parts, b.step_parts, b.x_parts};
      const int counts[4] = {ep, ep, vp, vp};
      for (int i = 0; i < 4; ++i) {
        red.parts[i] = parts[i];
        red.n[i] = counts[i];
      }
      red.count = 4;
      hipLaunchKernelGGL(pg2_reduce, dim3(1), dim3(kBlock), 0, st, red, b.out);
      CSM_HIP(hipGetLastError());
      CSM_HIP(hipMemcpyAsync(host, b.out, 32, hipMemcpyDeviceToHost, st));
      CSM_HIP(hipStreamSynchronize(st));
      model_change = host[0];
      candidate_cost = host[1];
      step_norm = std::sqrt(host[2]);
      x_norm = std::sqrt(host[3]);
      valid = std::isfinite(step_norm) && std::isfinite(model_change) && model_change > 0.;
    }
    phase[3] += Seconds() - t0;
    if (!valid) {
      // HandleInvalidStep.
      if (++invalid_steps >= kMaxInvalidSteps) {
        termination = CSM_POSE_GRAPH2D_FAILURE;
        break;
      }
      lm.Rejected();
      continue;
    }
    invalid_steps = 0;
    // A candidate whose cost cannot be evaluated counts as infinitely bad.
    if (!std::isfinite(candidate_cost)) candidate_cost = DBL_MAX;
    if (step_norm <= kParameterTolerance * (x_norm + kParameterTolerance)) {
      termination = CSM_POSE_GRAPH2D_CONVERGENCE_PARAMETER;
      break;
    }
    if (std::fabs(cost - candidate_cost) <= kFunctionTolerance * cost) {
      termination = CSM_POSE_GRAPH2D_CONVERGENCE_FUNCTION;
      break;
    }
    const double quality = evaluator.Quality(candidate_cost, model_change);
    if (quality > kMinRelativeDecrease) {
      // HandleSuccessfulStep.
      std::swap(x, candidate);
      t0 = Seconds();
      if ((rc = LinearizeAt(ctx, b, x, b.constant, V, E, o.huber_scale, nullptr, lin))) return rc;
      phase[1] += Seconds() - t0;
      cost = lin[0];
      gradient_max = lin[1];
      ++summary->num_successful_steps;
      lm.Accepted(quality);
      evaluator.Accepted(cost, model_change);
      if (cost < minimum_cost) {
        minimum_cost = cost;
        best = nullptr;
      } else if (!best) {
        // The cheapest point is the one x just left: after the swap above it
        // sits in `candidate`, which the next step overwrites.
        CSM_HIP(hipMemcpyAsync(b.best, candidate, 24 * static_cast<size_t>(V),
                               hipMemcpyDeviceToDevice, st));
        best = b.best;
      }
      if (!std::isfinite(gradient_max)) {
        termination = CSM_POSE_GRAPH2D_FAILURE;
        break;
      }
    } else {
      lm.Rejected();
    }
  }
  summary->num_iterations = iteration;
  summary->final_cost = minimum_cost + fixed_cost;
  summary->termination = termination;
  // Constant vertices were never written on the device: x holds their input bits.
  CSM_HIP(hipMemcpyAsync(poses_inout, best ? best : x, 24 * static_cast<size_t>(V),
                         hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  return CSM_OK;
}

void csm_pose_graph2d_last_phase_seconds(csm_context* ctx, double out[4]) {
  if (!ctx || !out) return;
  std::lock_guard<std::mutex> lock(ctx->mu);
  for (int i = 0; i < 4; ++i) out[i] = ctx->pg2_phase_seconds[i];
}

}  // extern "C"
