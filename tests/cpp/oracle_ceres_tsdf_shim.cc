// Test infrastructure: the CPU restatement of CeresScanMatcher2D::Match on a
// TSDF2D (ceres_scan_matcher_2d.cc:64-105, GridType::TSDF), on the oracle's
// TSDF2D. InterpolatedTSDF2D (interpolated_tsdf_2d.h:41-121) and
// TSDFMatchCostFunction2D (tsdf_match_cost_function_2d.cc:39-66) are restated
// with the Jacobian AutoDiff gives; the Levenberg-Marquardt loop is
// oracle/ceres2d.cc:164-268 with oracle/ceres_minimizer.h, plus the two rules
// for a cost that fails to evaluate: at the initial pose the solve ends with
// the parameters untouched and 0 iterations; at a candidate the step has cost
// DBL_MAX (Ceres 1.13 TrustRegionMinimizer, restated from memory: unpinned).
// Ceres is absent, so the restatement is pinned by the reference's own unit
// tests (tests/test_ceres_tsdf_host.py). Built by the tests against
// oracle/_build/liboracle.so with -ffp-contract=off.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ceres_minimizer.h"
#include "oracle_tsdf.h"

using namespace oracle;

namespace {

MapLimits Limits(double res, double max_x, double max_y, int nx, int ny) {
  MapLimits l;
  l.resolution = res;
  l.max_x = max_x;
  l.max_y = max_y;
  l.cells = CellLimits{nx, ny};
  return l;
}

// InterpolatedTSDF2D with T = (value, d/dx, d/dy).
class Interpolated {
 public:
  explicit Interpolated(const TSDF2D& t)
      : tsdf_(t),
        cost_table_(MakeConversionTable(t.GetMaxCorrespondenceCost(), t.converter().min_tsd(),
                                        t.converter().max_tsd())) {}

  // GetCorrespondenceCost (:41-66) and GetWeight (:69-82) at (x, y).
  void Get(double x, double y, double* c, double* dc, double* w, double* dw) const {
    const MapLimits& L = tsdf_.limits();
    // CenterOfLowerPixel (:109-121).
    const Idx2 cell = L.GetCellIndex(static_cast<float>(x), static_cast<float>(y));
    float x1 = static_cast<float>(L.max_x - L.resolution * (cell.y + 0.5));
    float y1 = static_cast<float>(L.max_y - L.resolution * (cell.x + 0.5));
    if (x1 > x) x1 = static_cast<float>(x1 - L.resolution);
    if (y1 > y) y1 = static_cast<float>(y1 - L.resolution);
    const float x2 = x1 + static_cast<float>(L.resolution);
    const float y2 = y1 + static_cast<float>(L.resolution);
    const Idx2 i1 = L.GetCellIndex(x1, y1);
    const Idx2 idx[4] = {i1, Idx2{i1.x - 1, i1.y}, Idx2{i1.x, i1.y - 1}, Idx2{i1.x - 1, i1.y - 1}};
    float wt[4];
    bool all_weighted = true;
    for (int k = 0; k < 4; ++k) {
      wt[k] = tsdf_.GetWeight(idx[k]);
      all_weighted = all_weighted && wt[k] != 0.f;
    }
    const double dx = static_cast<double>(x2 - x1), dy = static_cast<double>(y2 - y1);
    const double nx = (x - static_cast<double>(x1)) / dx, ny = (y - static_cast<double>(y1)) / dy;
    Bilinear(nx, ny, 1. / dx, 1. / dy, wt, w, dw);
    if (!all_weighted) {
      *c = static_cast<double>(tsdf_.GetMaxCorrespondenceCost());
      dc[0] = dc[1] = 0.;
      return;
    }
    float q[4];
    for (int k = 0; k < 4; ++k) q[k] = Cost(idx[k]);
    Bilinear(nx, ny, 1. / dx, 1. / dy, q, c, dc);
  }

 private:
  // Grid2D::GetCorrespondenceCost (grid_2d.h:53-57).
  float Cost(const Idx2& i) const {
    const MapLimits& L = tsdf_.limits();
    if (!L.Contains(i)) return tsdf_.GetMaxCorrespondenceCost();
    return cost_table_[tsdf_.tsd_cells()[static_cast<size_t>(i.y) * L.cells.num_x_cells + i.x] &
                       0x7fff];
  }
  // InterpolateBilinear (:95-104); q = q11, q12, q21, q22.
  static void Bilinear(double nx, double ny, double inv_dx, double inv_dy, const float* q,
                       double* f, double* df) {
    const double d1 = static_cast<double>(q[1] - q[0]), d2 = static_cast<double>(q[3] - q[2]);
    const double q1 = d1 * ny + static_cast<double>(q[0]);
    const double q2 = d2 * ny + static_cast<double>(q[2]);
    *f = (q2 - q1) * nx + q1;
    df[0] = (q2 - q1) * inv_dx;
    const double dq1 = d1 * inv_dy, dq2 = d2 * inv_dy;
    df[1] = (dq2 - dq1) * nx + dq1;
  }

  const TSDF2D& tsdf_;
  std::vector<float> cost_table_;
};

struct Problem {
  const Interpolated* grid;
  const float* xyz;
  int n;
  double scaling;  // residual_scaling_factor
  double wt, wr, tx, ty, t0;
};

// TSDFMatchCostFunction2D::operator() and its AutoDiff Jacobian: r (n) and J
// (n x 3, may be null). False when the summed weight is 0.
bool CostBlock(const Problem& p, const double* x, double* r, double* J) {
  const double s = std::sin(x[2]), c = std::cos(x[2]);
  const double ns = static_cast<double>(p.n) * p.scaling;
  std::vector<double> b(p.n), db(3 * static_cast<size_t>(p.n));
  double W = 0., dW[3] = {0., 0., 0.};
  for (int i = 0; i < p.n; ++i) {
    const double px = static_cast<double>(p.xyz[3 * i]), py = static_cast<double>(p.xyz[3 * i + 1]);
    const double wx = c * px + (-s * py + x[0] * 1.);
    const double wy = s * px + (c * py + x[1] * 1.);
    double cc, dcc[2], ww, dww[2];
    p.grid->Get(wx, wy, &cc, dcc, &ww, dww);
    b[i] = ns * cc * ww;
    W += ww;
    const double dwx_dt = -s * px - c * py, dwy_dt = c * px - s * py;
    const double dc[3] = {dcc[0], dcc[1], dcc[0] * dwx_dt + dcc[1] * dwy_dt};
    const double dw[3] = {dww[0], dww[1], dww[0] * dwx_dt + dww[1] * dwy_dt};
    for (int a = 0; a < 3; ++a) {
      db[3 * i + a] = ns * (dc[a] * ww + cc * dw[a]);
      dW[a] += dw[a];
    }
  }
  if (W == 0.) return false;
  for (int i = 0; i < p.n; ++i) {
    r[i] = b[i] / W;
    if (J)
      for (int a = 0; a < 3; ++a) J[3 * i + a] = (db[3 * i + a] - r[i] * dW[a]) / W;
  }
  return true;
}

// All n + 3 residuals (and the Jacobian) as oracle/ceres2d.cc's Evaluate;
// false when the cost block fails.
bool Evaluate(const Problem& p, const double* x, std::vector<double>* r, std::vector<double>* J,
              double* cost) {
  const size_t n = static_cast<size_t>(p.n);
  r->resize(n + 3);
  if (J) J->resize(3 * (n + 3));
  if (!CostBlock(p, x, r->data(), J ? J->data() : nullptr)) return false;
  (*r)[n] = p.wt * (x[0] - p.tx);
  (*r)[n + 1] = p.wt * (x[1] - p.ty);
  (*r)[n + 2] = p.wr * (x[2] - p.t0);
  double sum = 0.;
  for (size_t i = 0; i < n + 3; ++i) sum += (*r)[i] * (*r)[i];
  if (J) {
    for (int k = 0; k < 9; ++k) (*J)[3 * n + k] = 0.;
    (*J)[3 * n + 0] = p.wt;
    (*J)[3 * (n + 1) + 1] = p.wt;
    (*J)[3 * (n + 2) + 2] = p.wr;
  }
  *cost = 0.5 * sum;
  return true;
}

bool Solve3(double A[3][3], const double b[3], double out[3]) {
  double M[3][4];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) M[i][j] = A[i][j];
    M[i][3] = b[i];
  }
  for (int c = 0; c < 3; ++c) {
    int piv = c;
    for (int i = c + 1; i < 3; ++i)
      if (std::fabs(M[i][c]) > std::fabs(M[piv][c])) piv = i;
    if (M[piv][c] == 0.) return false;
    for (int j = 0; j < 4; ++j) std::swap(M[c][j], M[piv][j]);
    for (int i = c + 1; i < 3; ++i) {
      const double f = M[i][c] / M[c][c];
      for (int j = c; j < 4; ++j) M[i][j] -= f * M[c][j];
    }
  }
  for (int i = 2; i >= 0; --i) {
    double v = M[i][3];
    for (int j = i + 1; j < 3; ++j) v -= M[i][j] * out[j];
    out[i] = v / M[i][i];
  }
  return true;
}

// oracle/ceres2d.cc's CeresMatch2D loop over Evaluate above.
int Match(const Problem& p, int max_num_iterations, bool nonmonotonic, const double initial[3],
          double pose[3], int* failed_candidates) {
  double x[3] = {initial[0], initial[1], initial[2]};
  pose[0] = x[0];
  pose[1] = x[1];
  pose[2] = x[2];
  *failed_candidates = 0;
  std::vector<double> r, J, r_new;
  double cost;
  if (!Evaluate(p, x, &r, &J, &cost)) return 0;  // FAILURE: parameters untouched
  const size_t m = r.size();
  double scale[3];
  for (int j = 0; j < 3; ++j) {
    double s = 0.;
    for (size_t i = 0; i < m; ++i) s += J[3 * i + j] * J[3 * i + j];
    scale[j] = 1. / (1. + std::sqrt(s));
  }
  StepEvaluator ev(cost, nonmonotonic ? 5 : 0);
  double best[3] = {x[0], x[1], x[2]}, best_cost = cost;
  double radius = 1e4, decrease_factor = 2.;
  int iter = 0, invalid = 0;
  double Au[3][3], gu[3];
  auto normal_equations = [&]() {
    for (int a = 0; a < 3; ++a) {
      gu[a] = 0.;
      for (int b = 0; b < 3; ++b) Au[a][b] = 0.;
    }
    for (size_t i = 0; i < m; ++i)
      for (int a = 0; a < 3; ++a) {
        gu[a] += J[3 * i + a] * r[i];
        for (int b = 0; b < 3; ++b) Au[a][b] += J[3 * i + a] * J[3 * i + b];
      }
  };
  normal_equations();
  auto gradient_small = [&]() {
    return std::max({std::fabs(gu[0]), std::fabs(gu[1]), std::fabs(gu[2])}) <= 1e-10;
  };
  bool go = max_num_iterations > 0 && !gradient_small();
  while (go) {
    ++iter;
    double A[3][3], g[3];
    for (int a = 0; a < 3; ++a) {
      g[a] = gu[a] * scale[a];
      for (int b = 0; b < 3; ++b) A[a][b] = Au[a][b] * scale[a] * scale[b];
    }
    double M[3][3], rhs[3], ds[3] = {0., 0., 0.};
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) M[a][b] = A[a][b];
      M[a][a] += std::min(std::max(A[a][a], 1e-6), 1e32) / radius;
      rhs[a] = -g[a];
    }
    const bool solved = Solve3(M, rhs, ds);
    double gd = 0., dad = 0.;
    for (int a = 0; a < 3; ++a) {
      gd += g[a] * ds[a];
      for (int b = 0; b < 3; ++b) dad += ds[a] * A[a][b] * ds[b];
    }
    const double model = -(gd + 0.5 * dad);
    if (!solved || !(model > 0.)) {
      if (++invalid > 5) break;
      radius /= decrease_factor;
      decrease_factor *= 2.;
    } else {
      invalid = 0;
      double step[3], step_norm = 0., x_norm = 0.;
      for (int a = 0; a < 3; ++a) {
        step[a] = ds[a] * scale[a];
        step_norm += step[a] * step[a];
        x_norm += x[a] * x[a];
      }
      const double xn[3] = {x[0] + step[0], x[1] + step[1], x[2] + step[2]};
      double new_cost;
      if (!Evaluate(p, xn, &r_new, nullptr, &new_cost)) {
        new_cost = DBL_MAX;  // a candidate that fails to evaluate
        ++*failed_candidates;
      }
      if (std::sqrt(step_norm) <= (std::sqrt(x_norm) + 1e-8) * 1e-8) break;  // parameter tol.
      if (std::fabs(cost - new_cost) <= 1e-6 * cost) break;                 // function tol.
      const double quality = ev.Quality(new_cost, model);
      if (quality > 1e-3) {
        for (int a = 0; a < 3; ++a) x[a] = xn[a];
        Evaluate(p, x, &r, &J, &cost);
        normal_equations();
        const double tf = 2. * quality - 1.;
        radius = std::min(1e16, radius / std::max(1. / 3., 1. - tf * tf * tf));
        decrease_factor = 2.;
        ev.Accepted(new_cost, model);
        if (cost < best_cost) {
          best_cost = cost;
          for (int a = 0; a < 3; ++a) best[a] = x[a];
        }
      } else {
        radius /= decrease_factor;
        decrease_factor *= 2.;
      }
    }
    go = iter < max_num_iterations && radius >= 1e-32 && !gradient_small();
  }
  pose[0] = best[0];
  pose[1] = best[1];
  pose[2] = best[2];
  return iter;
}

TSDF2D MakeGrid(double res, double max_x, double max_y, int32_t nx, int32_t ny, float truncation,
                float max_weight, const uint16_t* tsd, const uint16_t* weight) {
  const size_t n = static_cast<size_t>(nx) * ny;
  return TSDF2D(Limits(res, max_x, max_y, nx, ny), truncation, max_weight,
                std::vector<uint16_t>(tsd, tsd + n), std::vector<uint16_t>(weight, weight + n));
}

int Expect(bool ok, const char* what, double got, double want) {
  if (ok) return 0;
  std::fprintf(stderr, "interpolated_tsdf_2d_test: %s: got %.9g, want %.9g\n", what, got, want);
  return 1;
}

}  // namespace

extern "C" {

// The cost block at `pose` with scaling factor `scaling`: returns 1 and fills
// residuals[n], jacobian[3n] (row-major), or returns 0.
int32_t shim_ceres_tsdf_evaluate(double res, double max_x, double max_y, int32_t nx, int32_t ny,
                                 float truncation, float max_weight, const uint16_t* tsd,
                                 const uint16_t* weight, const float* xyz, int32_t n,
                                 double scaling, const double* pose, double* residuals,
                                 double* jacobian) {
  const TSDF2D t = MakeGrid(res, max_x, max_y, nx, ny, truncation, max_weight, tsd, weight);
  const Interpolated g(t);
  const Problem p{&g, xyz, n, scaling, 0., 0., 0., 0., 0.};
  return CostBlock(p, pose, residuals, jacobian) ? 1 : 0;
}

// CeresScanMatcher2D::Match. opts as oracle_ceres2d_match. Returns the
// iterations; *failed_candidates the candidate evaluations that failed.
int32_t shim_ceres_tsdf_match(double res, double max_x, double max_y, int32_t nx, int32_t ny,
                              float truncation, float max_weight, const uint16_t* tsd,
                              const uint16_t* weight, const double* opts, const double* target,
                              const double* initial, const float* xyz, int32_t n, double* out,
                              int32_t* failed_candidates) {
  const TSDF2D t = MakeGrid(res, max_x, max_y, nx, ny, truncation, max_weight, tsd, weight);
  const Interpolated g(t);
  const Problem p{&g,      xyz,     n,         opts[0] / std::sqrt(static_cast<double>(n)),
                  opts[1], opts[2], target[0], target[1],
                  initial[2]};
  int failed = 0;
  const int iters = Match(p, static_cast<int>(opts[3]), opts[4] != 0., initial, out, &failed);
  *failed_candidates = failed;
  return iters;
}

// interpolated_tsdf_2d_test.cc's two cases (:48-88, :90-120) against the
// restated interpolation, at their tolerances. Returns the failed expectations.
int32_t shim_interpolated_tsdf_ref_tests() {
  int bad = 0;
  {  // InterpolatesGridPoints
    TSDF2D t(Limits(1., 5.5, 5.5, 10, 10), 1.0f, 10.0f);
    const MapLimits& L = t.limits();
    const float inner[4][2] = {{1.f, 1.f}, {2.f, 1.f}, {1.f, 2.f}, {2.f, 2.f}};
    for (const auto& q : inner) t.SetCell(L.GetCellIndex(q[0], q[1]), 0.1f, 1.0f);
    for (int x = 0; x < 4; ++x) {
      t.SetCell(L.GetCellIndex(static_cast<float>(x), 0.f), 0.1f, 1.0f);
      t.SetCell(L.GetCellIndex(static_cast<float>(x), 3.f), 0.1f, 1.0f);
    }
    for (int y = 1; y < 3; ++y) {
      t.SetCell(L.GetCellIndex(0.f, static_cast<float>(y)), 0.1f, 1.0f);
      t.SetCell(L.GetCellIndex(3.f, static_cast<float>(y)), 0.1f, 1.0f);
    }
    const Interpolated g(t);
    const std::vector<float> table = MakeConversionTable(1.0f, -1.0f, 1.0f);
    auto raw_cost = [&](float x, float y) {
      const Idx2 i = L.GetCellIndex(x, y);
      return table[t.tsd_cells()[static_cast<size_t>(i.y) * 10 + i.x] & 0x7fff];
    };
    double c, dc[2], w, dw[2];
    for (const auto& q : inner) {
      g.Get(q[0], q[1], &c, dc, &w, dw);
      bad += Expect(std::fabs(raw_cost(q[0], q[1]) - c) <= 1e-4, "grid point cost", c,
                    raw_cost(q[0], q[1]));
      const float rw = t.GetWeight(L.GetCellIndex(q[0], q[1]));
      bad += Expect(std::fabs(rw - w) <= 1e-4, "grid point weight", w, rw);
    }
    g.Get(3.0, 2.0, &c, dc, &w, dw);
    bad += Expect(std::fabs(t.GetMaxCorrespondenceCost() - c) <= 1e-4, "unknown cell cost", c,
                  t.GetMaxCorrespondenceCost());
    const float rw = t.GetWeight(L.GetCellIndex(3.f, 2.f));
    bad += Expect(std::fabs(rw - w) <= 1e-4, "unknown cell weight", w, rw);
  }
  {  // InterpolatesWithinCell
    TSDF2D t(Limits(1., 5.5, 5.5, 10, 10), 1.0f, 10.0f);
    const MapLimits& L = t.limits();
    const float tsd_00 = 0.1f, tsd_01 = 0.2f, tsd_10 = 0.3f, tsd_11 = 0.4f;
    const float w_00 = 1.f, w_01 = 2.f, w_10 = 3.f, w_11 = 4.f;
    t.SetCell(L.GetCellIndex(0.f, 0.f), tsd_00, w_00);
    t.SetCell(L.GetCellIndex(0.f, 1.f), tsd_01, w_01);
    t.SetCell(L.GetCellIndex(1.f, 0.f), tsd_10, w_10);
    t.SetCell(L.GetCellIndex(1.f, 1.f), tsd_11, w_11);
    const Interpolated g(t);
    const double step = L.resolution / 100.;
    for (double x = 0. + step; x < 1.; x += L.resolution)
      for (double y = 0. + step; y < 1.; y += L.resolution) {
        double c, dc[2], w, dw[2];
        g.Get(x, y, &c, dc, &w, dw);
        const float tsd_expected =
            (x * tsd_10 + (1.f - x) * tsd_00) * (1.f - y) + (x * tsd_11 + (1.f - x) * tsd_01) * y;
        const float w_expected =
            (x * w_10 + (1.f - x) * w_00) * (1.f - y) + (x * w_11 + (1.f - x) * w_01) * y;
        bad += Expect(std::fabs(c - tsd_expected) <= 1e-3, "within-cell cost", c, tsd_expected);
        bad += Expect(std::fabs(w - w_expected) <= 1e-3, "within-cell weight", w, w_expected);
      }
  }
  return bad;
}

}  // extern "C"
