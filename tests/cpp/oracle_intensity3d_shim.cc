// Test infrastructure: the CPU restatement of IntensityHybridGrid
// (mapping/3d/hybrid_grid.h:547-571) over the oracle's HybridGridBase3
// (oracle/oracle3d.h), of InsertIntensitiesIntoGrid
// (mapping/3d/range_data_inserter_3d.cc:76-89), of InterpolatedIntensityGrid
// with its analytic gradient (interpolated_grid.h:48-160), of
// IntensityCostFunction3D (intensity_cost_function_3d.h:67-85), of
// ceres::HuberLoss with Ceres' Corrector, and of CeresScanMatcher3D::Match with
// the optional intensity block (ceres_scan_matcher_3d.cc:84-160): the loop of
// oracle/ceres3d.cc, copied, so that without an intensity grid it returns what
// oracle_ceres3d_match returns. Ceres is not in this image: the Huber and
// Corrector rules are written from Ceres 1.13 and unpinned, like that loop.
// Built by the tests against oracle/_build/liboracle.so
// (tests/intensity3d_support.py).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ceres_minimizer.h"
#include "oracle3d.h"

using namespace oracle;

namespace {

// hybrid_grid.h:547-550.
struct AverageIntensityData {
  float sum = 0.f;
  int count = 0;
};
bool operator==(const AverageIntensityData& a, const AverageIntensityData& b) {
  return a.sum == b.sum && a.count == b.count;
}

// hybrid_grid.h:552-571.
class IntensityHybridGrid : public HybridGridBase3<AverageIntensityData> {
 public:
  explicit IntensityHybridGrid(float resolution)
      : HybridGridBase3<AverageIntensityData>(resolution) {}
  void AddIntensity(const Idx3& index, float intensity) {
    AverageIntensityData* const cell = mutable_value(index);
    cell->count += 1;
    cell->sum += intensity;
  }
  float GetIntensity(const Idx3& index) const {
    const AverageIntensityData cell = value(index);
    if (cell.count == 0) return 0.f;
    return cell.sum / cell.count;
  }
};

IntensityHybridGrid* Grid(void* h) { return static_cast<IntensityHybridGrid*>(h); }

// f(t; A, B) = (A - B) 2t^3 + (B - A) 3t^2 + A and its derivatives
// (interpolated_grid.h:107-116), as oracle/ceres3d.cc.
struct Step {
  double t, tt, ttt;
  double f(double a, double b) const { return (a - b) * ttt * 2. + (b - a) * tt * 3. + a; }
  double dt(double a, double b) const { return (a - b) * 6. * tt + (b - a) * 6. * t; }
  double da() const { return 2. * ttt - 3. * tt + 1.; }
  double db() const { return -2. * ttt + 3. * tt; }
};

// InterpolatedGrid<IntensityHybridGrid>::GetInterpolatedValue and its gradient:
// oracle::Interpolate with GetValue = GetIntensity (interpolated_grid.h:154-157).
double InterpolateIntensity(const IntensityHybridGrid& g, double x, double y, double z,
                            double grad[3]) {
  const float res = g.resolution();
  const Idx3 c = g.GetCellIndex(Vec3f{static_cast<float>(x), static_cast<float>(y),
                                      static_cast<float>(z)});
  float cx = static_cast<float>(c.x) * res, cy = static_cast<float>(c.y) * res,
        cz = static_cast<float>(c.z) * res;
  if (cx > x) cx -= res;
  if (cy > y) cy -= res;
  if (cz > z) cz -= res;
  const double x1 = cx, y1 = cy, z1 = cz;
  const double x2 = static_cast<float>(cx + res), y2 = static_cast<float>(cy + res),
               z2 = static_cast<float>(cz + res);
  const Idx3 i1 = g.GetCellIndex(Vec3f{cx, cy, cz});
  auto q = [&](int dx, int dy, int dz) {
    return static_cast<double>(g.GetIntensity(Idx3{i1.x + dx, i1.y + dy, i1.z + dz}));
  };
  const double q111 = q(0, 0, 0), q112 = q(0, 0, 1), q121 = q(0, 1, 0), q122 = q(0, 1, 1);
  const double q211 = q(1, 0, 0), q212 = q(1, 0, 1), q221 = q(1, 1, 0), q222 = q(1, 1, 1);
  const double nx = (x - x1) / (x2 - x1), ny = (y - y1) / (y2 - y1), nz = (z - z1) / (z2 - z1);
  const Step sx{nx, nx * nx, nx * (nx * nx)}, sy{ny, ny * ny, ny * (ny * ny)},
      sz{nz, nz * nz, nz * (nz * nz)};
  const double q11 = sz.f(q111, q112), q12 = sz.f(q121, q122);
  const double q21 = sz.f(q211, q212), q22 = sz.f(q221, q222);
  const double q1 = sy.f(q11, q12), q2 = sy.f(q21, q22);
  const double v = sx.f(q1, q2);
  if (grad) {
    const double dnx = sx.dt(q1, q2);
    const double dny = sx.da() * sy.dt(q11, q12) + sx.db() * sy.dt(q21, q22);
    const double dnz = sx.da() * (sy.da() * sz.dt(q111, q112) + sy.db() * sz.dt(q121, q122)) +
                       sx.db() * (sy.da() * sz.dt(q211, q212) + sy.db() * sz.dt(q221, q222));
    grad[0] = dnx / (x2 - x1);
    grad[1] = dny / (y2 - y1);
    grad[2] = dnz / (z2 - z1);
  }
  return v;
}

// Eigen _transformVector and its derivative in (w, x, y, z), as oracle/ceres3d.cc.
void Rotate(const double q[4], const double v[3], double out[3], double J[12]) {
  const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
  const double ax = qy * v[2] - qz * v[1], ay = qz * v[0] - qx * v[2], az = qx * v[1] - qy * v[0];
  const double ux = 2. * ax, uy = 2. * ay, uz = 2. * az;
  out[0] = v[0] + w * ux + (qy * uz - qz * uy);
  out[1] = v[1] + w * uy + (qz * ux - qx * uz);
  out[2] = v[2] + w * uz + (qx * uy - qy * ux);
  if (!J) return;
  auto cross = [](const double a[3]) {
    return std::vector<double>{0., -a[2], a[1], a[2], 0., -a[0], -a[1], a[0], 0.};
  };
  const double a[3] = {ax, ay, az}, qv[3] = {qx, qy, qz};
  const std::vector<double> V = cross(v), A = cross(a), Q = cross(qv);
  for (int r = 0; r < 3; ++r) {
    J[4 * r] = (r == 0 ? ux : r == 1 ? uy : uz);
    for (int c = 0; c < 3; ++c) {
      double qv_v = 0.;
      for (int k = 0; k < 3; ++k) qv_v += Q[3 * r + k] * V[3 * k + c];
      J[4 * r + 1 + c] = -2. * w * V[3 * r + c] - 2. * A[3 * r + c] - 2. * qv_v;
    }
  }
}

void QuatProduct(const double a[4], const double b[4], double z[4]) {
  z[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  z[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  z[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  z[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// QuaternionParameterization::ComputeJacobian (4 x 3, row-major).
void PlusJacobian(const double q[4], double L[12]) {
  const double v[12] = {-q[1], -q[2], -q[3], q[0], q[3], -q[2],
                        -q[3], q[0],  q[1],  q[2], -q[1], q[0]};
  for (int a = 0; a < 12; ++a) L[a] = v[a];
}

// IntensityCostFunction3D::Evaluate (intensity_cost_function_3d.h:67-85):
// residuals and, with J, the n x 6 Jacobian in the tangent space.
void IntensityBlock(const IntensityHybridGrid& grid, const std::vector<Vec3f>& cloud,
                    const float* intensities, double scale, float threshold, const double t[3],
                    const double q[4], std::vector<double>* r, std::vector<double>* J) {
  double L[12];
  PlusJacobian(q, L);
  for (size_t i = 0; i < cloud.size(); ++i) {
    if (intensities[i] > threshold) {
      r->push_back(0.);
      if (J)
        for (int c = 0; c < 6; ++c) J->push_back(0.);
      continue;
    }
    const double v[3] = {cloud[i].x, cloud[i].y, cloud[i].z};
    double w[3], Jq[12], grad[3];
    Rotate(q, v, w, J ? Jq : nullptr);
    for (int a = 0; a < 3; ++a) w[a] += t[a];
    const double val = InterpolateIntensity(grid, w[0], w[1], w[2], J ? grad : nullptr);
    r->push_back(scale * (val - static_cast<double>(intensities[i])));
    if (J) {
      double dq[4] = {0., 0., 0., 0.};
      for (int c = 0; c < 4; ++c)
        for (int a = 0; a < 3; ++a) dq[c] += scale * grad[a] * Jq[4 * a + c];
      for (int a = 0; a < 3; ++a) J->push_back(scale * grad[a]);
      for (int c = 0; c < 3; ++c) {
        double s = 0.;
        for (int m = 0; m < 4; ++m) s += dq[m] * L[3 * m + c];
        J->push_back(s);
      }
    }
  }
}

// ceres::HuberLoss::Evaluate (loss_function.cc): rho, rho', rho''.
void Huber(double a, double s, double rho[3]) {
  const double b = a * a;
  if (s > b) {
    const double r = std::sqrt(s);
    rho[0] = 2. * a * r - b;
    rho[1] = std::max(DBL_MIN, a / r);
    rho[2] = -rho[1] / (2. * s);
  } else {
    rho[0] = s;
    rho[1] = 1.;
    rho[2] = 0.;
  }
}

struct Problem3 {
  const HybridGrid* grid[2];
  const std::vector<Vec3f>* cloud[2];
  double scale[2];
  double wt, wr, target[3], target_inv[4];
  // The intensity block on cloud 0 (null: none).
  const IntensityHybridGrid* igrid = nullptr;
  const float* intensities = nullptr;
  double iscale = 0., huber = 0.;
  float threshold = 0.f;
};

// oracle/ceres3d.cc's Evaluate3 with the intensity block after cloud 0's
// occupied-space block (the order Match adds them in). The block's rows come
// out as Ceres' Corrector leaves them for rho'' <= 0 (corrector.cc): residuals
// and Jacobian scaled by sqrt(rho'); its cost is 0.5 rho(S). *block_s, if
// given, is S.
double Evaluate3(const Problem3& p, const double t[3], const double q[4], std::vector<double>* r,
                 std::vector<double>* J, double* block_s) {
  r->clear();
  if (J) J->clear();
  double cost = 0.;
  double L[12];
  PlusJacobian(q, L);
  for (int k = 0; k < 2; ++k) {
    for (const Vec3f& pt : *p.cloud[k]) {
      const double v[3] = {pt.x, pt.y, pt.z};
      double w[3], Jq[12];
      Rotate(q, v, w, J ? Jq : nullptr);
      for (int a = 0; a < 3; ++a) w[a] += t[a];
      double grad[3];
      const double val = Interpolate(*p.grid[k], w[0], w[1], w[2], J ? grad : nullptr);
      const double res = p.scale[k] * (1. - val);
      r->push_back(res);
      cost += res * res;
      if (J) {
        double dq[4] = {0., 0., 0., 0.};
        for (int c = 0; c < 4; ++c)
          for (int a = 0; a < 3; ++a) dq[c] += -p.scale[k] * grad[a] * Jq[4 * a + c];
        for (int a = 0; a < 3; ++a) J->push_back(-p.scale[k] * grad[a]);
        for (int c = 0; c < 3; ++c) {
          double s = 0.;
          for (int m = 0; m < 4; ++m) s += dq[m] * L[3 * m + c];
          J->push_back(s);
        }
      }
    }
    if (k == 0 && p.igrid) {
      std::vector<double> br, bJ;
      IntensityBlock(*p.igrid, *p.cloud[0], p.intensities, p.iscale, p.threshold, t, q, &br,
                     J ? &bJ : nullptr);
      double s = 0.;
      for (double v : br) s += v * v;
      if (block_s) *block_s = s;
      double rho[3];
      Huber(p.huber, s, rho);
      cost += rho[0];
      const double root = std::sqrt(rho[1]);
      for (double v : br) r->push_back(root * v);
      if (J)
        for (double v : bJ) J->push_back(root * v);
    }
  }
  for (int a = 0; a < 3; ++a) {
    const double res = p.wt * (t[a] - p.target[a]);
    r->push_back(res);
    cost += res * res;
    if (J)
      for (int c = 0; c < 6; ++c) J->push_back(c == a ? p.wt : 0.);
  }
  double delta[4];
  QuatProduct(p.target_inv, q, delta);
  const double* ti = p.target_inv;
  const double M[3][4] = {{ti[1], ti[0], -ti[3], ti[2]},
                          {ti[2], ti[3], ti[0], -ti[1]},
                          {ti[3], -ti[2], ti[1], ti[0]}};
  for (int a = 0; a < 3; ++a) {
    const double res = p.wr * delta[a + 1];
    r->push_back(res);
    cost += res * res;
    if (J) {
      for (int c = 0; c < 3; ++c) J->push_back(0.);
      for (int c = 0; c < 3; ++c) {
        double s = 0.;
        for (int m = 0; m < 4; ++m) s += p.wr * M[a][m] * L[3 * m + c];
        J->push_back(s);
      }
    }
  }
  return 0.5 * cost;
}

bool SolveN(std::vector<double> M, std::vector<double> b, int n, double* out) {
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int i = c + 1; i < n; ++i)
      if (std::fabs(M[i * n + c]) > std::fabs(M[piv * n + c])) piv = i;
    if (M[piv * n + c] == 0.) return false;
    for (int j = 0; j < n; ++j) std::swap(M[c * n + j], M[piv * n + j]);
    std::swap(b[c], b[piv]);
    for (int i = c + 1; i < n; ++i) {
      const double f = M[i * n + c] / M[c * n + c];
      for (int j = c; j < n; ++j) M[i * n + j] -= f * M[c * n + j];
      b[i] -= f * b[c];
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = b[i];
    for (int j = i + 1; j < n; ++j) v -= M[i * n + j] * out[j];
    out[i] = v / M[i * n + i];
  }
  return true;
}

// oracle/ceres3d.cc's CeresMatch3D over Problem3 (Ceres 1.13
// TrustRegionMinimizer::Minimize). *initial_s: the intensity block's S at the
// initial pose.
int Match3(const Problem3& p, int max_num_iterations, bool nonmonotonic, const double initial_t[3],
           const double initial_q[4], double out_t[3], double out_q[4], double* initial_s) {
  double t[3] = {initial_t[0], initial_t[1], initial_t[2]};
  double q[4] = {initial_q[0], initial_q[1], initial_q[2], initial_q[3]};
  std::vector<double> r, J, rn;
  double cost = Evaluate3(p, t, q, &r, &J, initial_s);
  const size_t m = r.size();
  auto normal = [&](double* Au, double* gu) {
    for (int a = 0; a < 36; ++a) Au[a] = 0.;
    for (int a = 0; a < 6; ++a) gu[a] = 0.;
    for (size_t i = 0; i < m; ++i)
      for (int a = 0; a < 6; ++a) {
        gu[a] += J[6 * i + a] * r[i];
        for (int b = 0; b < 6; ++b) Au[6 * a + b] += J[6 * i + a] * J[6 * i + b];
      }
  };
  double Au[36], gu[6], scale[6];
  normal(Au, gu);
  for (int a = 0; a < 6; ++a) scale[a] = 1. / (1. + std::sqrt(Au[7 * a]));
  StepEvaluator ev(cost, nonmonotonic ? 5 : 0);
  double best_t[3] = {t[0], t[1], t[2]}, best_q[4] = {q[0], q[1], q[2], q[3]}, best_cost = cost;
  double radius = 1e4, decrease = 2.;
  int iter = 0, invalid = 0;
  auto gradient_small = [&]() {
    double gmax = 0.;
    for (int a = 0; a < 6; ++a) gmax = std::max(gmax, std::fabs(gu[a]));
    return gmax <= 1e-10;
  };
  bool go = max_num_iterations > 0 && !gradient_small();
  while (go) {
    ++iter;
    std::vector<double> A(36), g(6), M(36), rhs(6);
    for (int a = 0; a < 6; ++a) {
      g[a] = gu[a] * scale[a];
      for (int b = 0; b < 6; ++b) A[6 * a + b] = Au[6 * a + b] * scale[a] * scale[b];
    }
    for (int a = 0; a < 6; ++a) {
      for (int b = 0; b < 6; ++b) M[6 * a + b] = A[6 * a + b];
      M[7 * a] += std::min(std::max(A[7 * a], 1e-6), 1e32) / radius;
      rhs[a] = -g[a];
    }
    double ds[6] = {0., 0., 0., 0., 0., 0.};
    const bool solved = SolveN(M, rhs, 6, ds);
    double gd = 0., dad = 0.;
    for (int a = 0; a < 6; ++a) {
      gd += g[a] * ds[a];
      for (int b = 0; b < 6; ++b) dad += ds[a] * A[6 * a + b] * ds[b];
    }
    const double model = -(gd + 0.5 * dad);
    if (!solved || !(model > 0.)) {
      if (++invalid > 5) break;
      radius /= decrease;
      decrease *= 2.;
    } else {
      invalid = 0;
      double step[6], step_norm = 0., x_norm = 0.;
      for (int a = 0; a < 6; ++a) {
        step[a] = ds[a] * scale[a];
        step_norm += step[a] * step[a];
      }
      for (int a = 0; a < 3; ++a) x_norm += t[a] * t[a];
      for (int a = 0; a < 4; ++a) x_norm += q[a] * q[a];
      double tn[3] = {t[0] + step[0], t[1] + step[1], t[2] + step[2]}, qn[4];
      const double nrm = std::sqrt(step[3] * step[3] + step[4] * step[4] + step[5] * step[5]);
      if (nrm > 0.) {
        const double sn = std::sin(nrm) / nrm;
        const double qd[4] = {std::cos(nrm), sn * step[3], sn * step[4], sn * step[5]};
        QuatProduct(qd, q, qn);
      } else {
        for (int a = 0; a < 4; ++a) qn[a] = q[a];
      }
      const double new_cost = Evaluate3(p, tn, qn, &rn, nullptr, nullptr);
      if (std::sqrt(step_norm) <= (std::sqrt(x_norm) + 1e-8) * 1e-8) break;
      if (std::fabs(cost - new_cost) <= 1e-6 * cost) break;
      const double quality = ev.Quality(new_cost, model);
      if (quality > 1e-3) {
        for (int a = 0; a < 3; ++a) t[a] = tn[a];
        for (int a = 0; a < 4; ++a) q[a] = qn[a];
        cost = Evaluate3(p, t, q, &r, &J, nullptr);
        normal(Au, gu);
        const double tf = 2. * quality - 1.;
        radius = std::min(1e16, radius / std::max(1. / 3., 1. - tf * tf * tf));
        decrease = 2.;
        ev.Accepted(new_cost, model);
        if (cost < best_cost) {
          best_cost = cost;
          for (int a = 0; a < 3; ++a) best_t[a] = t[a];
          for (int a = 0; a < 4; ++a) best_q[a] = q[a];
        }
      } else {
        radius /= decrease;
        decrease *= 2.;
      }
    }
    go = iter < max_num_iterations && radius >= 1e-32 && !gradient_small();
  }
  for (int a = 0; a < 3; ++a) out_t[a] = best_t[a];
  for (int a = 0; a < 4; ++a) out_q[a] = best_q[a];
  return iter;
}

std::vector<Vec3f> Cloud(const float* xyz, int32_t n) {
  std::vector<Vec3f> c(static_cast<size_t>(n));
  for (int32_t i = 0; i < n; ++i) c[i] = Vec3f{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  return c;
}

}  // namespace

extern "C" {

void* shimi_create(float resolution) { return new IntensityHybridGrid(resolution); }
void shimi_destroy(void* h) { delete Grid(h); }
int32_t shimi_grid_size(void* h) { return Grid(h)->grid_size(); }

void shimi_add_intensity(void* h, int32_t x, int32_t y, int32_t z, float intensity) {
  Grid(h)->AddIntensity(Idx3{x, y, z}, intensity);
}

void shimi_get_intensity(void* h, const int32_t* ijk, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i)
    out[i] = Grid(h)->GetIntensity(Idx3{ijk[3 * i], ijk[3 * i + 1], ijk[3 * i + 2]});
}

// InsertIntensitiesIntoGrid (range_data_inserter_3d.cc:76-89); intensities
// null is a cloud whose intensities() is empty.
void shimi_insert(void* h, const float* xyz, const float* intensities, int64_t n,
                  float intensity_threshold) {
  if (!intensities) return;
  for (int64_t i = 0; i < n; ++i) {
    if (intensities[i] > intensity_threshold) continue;
    const Idx3 hit_cell = Grid(h)->GetCellIndex(Vec3f{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
    Grid(h)->AddIntensity(hit_cell, intensities[i]);
  }
}

// The cells that differ from the default, as the reference's iterator yields
// them. First call with null outputs for the number.
int64_t shimi_cells(void* h, int32_t* ijk, float* sums, int32_t* counts) {
  int64_t n = 0;
  Grid(h)->ForEach([&](const Idx3& c, const AverageIntensityData& v) {
    if (ijk) {
      ijk[3 * n] = c.x;
      ijk[3 * n + 1] = c.y;
      ijk[3 * n + 2] = c.z;
      sums[n] = v.sum;
      counts[n] = v.count;
    }
    ++n;
  });
  return n;
}

// IntensityCostFunction3D alone at pose (t, q as w, x, y, z): residuals[n] and
// the n x 6 Jacobian in the tangent space, without the loss.
void shimi_cost_block(void* h, const float* xyz, const float* intensities, int32_t n,
                      const double* pose7, double scale, float threshold, double* residuals,
                      double* jacobian) {
  std::vector<double> r, J;
  IntensityBlock(*Grid(h), Cloud(xyz, n), intensities, scale, threshold, pose7, pose7 + 3, &r, &J);
  for (int32_t i = 0; i < n; ++i) residuals[i] = r[i];
  for (int32_t i = 0; i < 6 * n; ++i) jacobian[i] = J[i];
}

void shimi_huber(double a, double s, double* rho3) { Huber(a, s, rho3); }

// opts: w0, w1, wt, wr, max_num_iterations, use_nonmonotonic_steps; iopts:
// weight, huber_scale, intensity_threshold. high / low: oracle HybridGrid
// handles; igrid: a shim grid or null (then oracle_ceres3d_match's result).
// out: t[3], q[4]; *initial_s: the intensity block's sum of squares at the
// initial pose. Returns the iterations.
int32_t shimi_ceres3d_match(void* high, void* low, const float* high_xyz, int32_t nh,
                            const float* low_xyz, int32_t nl, const double* opts,
                            const double* target, const double* initial, void* igrid,
                            const float* intensities, const double* iopts, double* out,
                            double* initial_s) {
  const std::vector<Vec3f> hc = Cloud(high_xyz, nh), lc = Cloud(low_xyz, nl);
  Problem3 p;
  p.grid[0] = static_cast<HybridGrid*>(high);
  p.grid[1] = static_cast<HybridGrid*>(low);
  p.cloud[0] = &hc;
  p.cloud[1] = &lc;
  p.scale[0] = opts[0] / std::sqrt(static_cast<double>(hc.size()));
  p.scale[1] = opts[1] / std::sqrt(static_cast<double>(lc.size()));
  p.wt = opts[2];
  p.wr = opts[3];
  for (int a = 0; a < 3; ++a) p.target[a] = target[a];
  p.target_inv[0] = initial[3];
  for (int a = 1; a < 4; ++a) p.target_inv[a] = -initial[3 + a];
  if (igrid) {
    p.igrid = Grid(igrid);
    p.intensities = intensities;
    p.iscale = iopts[0] / std::sqrt(static_cast<double>(hc.size()));
    p.huber = iopts[1];
    p.threshold = static_cast<float>(iopts[2]);
  }
  double s0 = 0.;
  const int it = Match3(p, static_cast<int>(opts[4]), opts[5] != 0., initial, initial + 3, out,
                        out + 3, &s0);
  if (initial_s) *initial_s = s0;
  return it;
}

}  // extern "C"
