// CPU checker of the pose-graph solve (tests/pose_graph2d_support.py builds
// it): the SPA cost of every edge with its full 3 x 6 Jacobian, Huber's
// corrector, and Ceres 1.13's trust-region loop with the Levenberg-Marquardt
// strategy, restated on the host with a dense normal matrix and a dense
// Cholesky factorisation as the linear solve. It shares no code with the
// library: a direct solve beside the library's iterative one.
//
// Layouts: poses V x 3 (x, y, angle); residuals E x 3; jacobians E x 18, the
// start block's 3 x 3 row-major, then the end block's; gradient V x 3.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

// csm_pose_graph2d_edge's layout.
struct Edge {
  int32_t start, end;
  double zbar[3];
  double translation_weight, rotation_weight;
  int32_t loss;  // 0 none, 1 Huber
  int32_t reserved;
};

namespace {

double WrapAngle(double d) {
  while (d > M_PI) d -= 2. * M_PI;
  while (d < -M_PI) d += 2. * M_PI;
  return d;
}

// The weighted residual and its Jacobian (3 x 6: columns start x, y, angle,
// end x, y, angle) before any loss.
void Spa(const Edge& e, const double* a, const double* b, double r[3], double J[3][6]) {
  const double ct = std::cos(a[2]), st = std::sin(a[2]);
  const double dx = b[0] - a[0], dy = b[1] - a[1];
  const double wt = e.translation_weight, wr = e.rotation_weight;
  r[0] = wt * (e.zbar[0] - (ct * dx + st * dy));
  r[1] = wt * (e.zbar[1] - (-st * dx + ct * dy));
  r[2] = wr * WrapAngle(e.zbar[2] - (b[2] - a[2]));
  const double full[3][6] = {
      {wt * ct, wt * st, wt * (st * dx - ct * dy), -wt * ct, -wt * st, 0.},
      {-wt * st, wt * ct, wt * (ct * dx + st * dy), wt * st, -wt * ct, 0.},
      {0., 0., wr, 0., 0., -wr}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 6; ++j) J[i][j] = full[i][j];
}

// rho(s) and sqrt(rho'(s)) of the edge's loss at s = |r|^2.
void Loss(const Edge& e, double huber, double s, double* rho, double* root) {
  *rho = s;
  *root = 1.;
  if (e.loss == 1 && s > huber * huber) {
    const double n = std::sqrt(s);
    *rho = 2. * huber * n - huber * huber;
    *root = std::sqrt(std::fmax(DBL_MIN, huber / n));
  }
}

struct Linearised {
  double cost = 0.;
  std::vector<double> r;  // corrected residuals, E x 3
  std::vector<double> J;  // corrected Jacobians, E x 18 as [row][column of 6]
};

double Evaluate(const double* poses, const Edge* edges, int64_t E, double huber, Linearised* out,
                double* raw_residuals, double* raw_jacobians) {
  double cost = 0.;
  if (out) {
    out->r.assign(3 * E, 0.);
    out->J.assign(18 * E, 0.);
  }
  for (int64_t k = 0; k < E; ++k) {
    const Edge& e = edges[k];
    double r[3], J[3][6];
    Spa(e, poses + 3 * e.start, poses + 3 * e.end, r, J);
    if (raw_residuals)
      for (int i = 0; i < 3; ++i) raw_residuals[3 * k + i] = r[i];
    if (raw_jacobians)
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          raw_jacobians[18 * k + 3 * i + j] = J[i][j];
          raw_jacobians[18 * k + 9 + 3 * i + j] = J[i][3 + j];
        }
    double rho, root;
    Loss(e, huber, r[0] * r[0] + r[1] * r[1] + r[2] * r[2], &rho, &root);
    cost += 0.5 * rho;
    if (out) {
      for (int i = 0; i < 3; ++i) {
        out->r[3 * k + i] = root * r[i];
        for (int j = 0; j < 6; ++j) out->J[18 * k + 6 * i + j] = root * J[i][j];
      }
    }
  }
  if (out) out->cost = cost;
  return cost;
}

// In-place lower Cholesky of the n x n row-major A; false if not positive
// definite or not finite.
bool Cholesky(std::vector<double>* A, int n) {
  double* a = A->data();
  for (int i = 0; i < n; ++i) {
    double* ri = a + static_cast<size_t>(i) * n;
    for (int j = 0; j <= i; ++j) {
      const double* rj = a + static_cast<size_t>(j) * n;
      double sum = ri[j];
      for (int k = 0; k < j; ++k) sum -= ri[k] * rj[k];
      if (i == j) {
        if (!(sum > 0.) || !std::isfinite(sum)) return false;
        ri[j] = std::sqrt(sum);
      } else {
        ri[j] = sum / rj[j];
      }
    }
  }
  return true;
}

void CholeskySolve(const std::vector<double>& L, int n, std::vector<double>* b) {
  double* x = b->data();
  for (int i = 0; i < n; ++i) {
    const double* ri = L.data() + static_cast<size_t>(i) * n;
    double sum = x[i];
    for (int k = 0; k < i; ++k) sum -= ri[k] * x[k];
    x[i] = sum / ri[i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double sum = x[i];
    for (int k = i + 1; k < n; ++k) sum -= L[static_cast<size_t>(k) * n + i] * x[k];
    x[i] = sum / L[static_cast<size_t>(i) * n + i];
  }
}

// Columns of the variable vertices: index[v] = first column or -1.
int IndexColumns(const uint8_t* constant, int V, std::vector<int>* index) {
  index->assign(V, -1);
  int n = 0;
  for (int v = 0; v < V; ++v)
    if (!(constant && constant[v])) {
      (*index)[v] = n;
      n += 3;
    }
  return n;
}

void Gradient(const Linearised& lin, const Edge* edges, int64_t E, const std::vector<int>& index,
              int n, std::vector<double>* g) {
  g->assign(n, 0.);
  for (int64_t k = 0; k < E; ++k) {
    const int cols[2] = {index[edges[k].start], index[edges[k].end]};
    for (int side = 0; side < 2; ++side) {
      if (cols[side] < 0) continue;
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i)
          (*g)[cols[side] + j] += lin.J[18 * k + 6 * i + 3 * side + j] * lin.r[3 * k + i];
    }
  }
}

double MaxAbs(const std::vector<double>& v) {
  double m = 0.;
  for (double x : v) m = std::fmax(m, std::fabs(x));
  return m;
}

}  // namespace

extern "C" {

int pg2ref_evaluate(const double* poses, int32_t V, const Edge* edges, int64_t E, double huber,
                    double* cost, double* residuals, double* gradient, double* jacobians) {
  Linearised lin;
  *cost = Evaluate(poses, edges, E, huber, &lin, residuals, jacobians);
  if (gradient) {
    std::vector<int> index;
    const int n = IndexColumns(nullptr, V, &index);
    std::vector<double> g;
    Gradient(lin, edges, E, index, n, &g);
    for (int i = 0; i < n; ++i) gradient[i] = g[i];
  }
  return 0;
}

// summary: initial cost, final cost, iterations, successful steps,
// termination (0 gradient, 1 parameter, 2 function tolerance, 3 no
// convergence, 4 failure), max |gradient| at the end.
int pg2ref_solve(double* poses, const uint8_t* constant, int32_t V, const Edge* edges, int64_t E,
                 double huber, int32_t max_num_iterations, double* summary) {
  std::vector<int> index;
  const int n = IndexColumns(constant, V, &index);
  std::vector<double> x(poses, poses + 3 * V), candidate(3 * V);
  Linearised lin;
  Evaluate(x.data(), edges, E, huber, &lin, nullptr, nullptr);
  std::vector<double> g;
  Gradient(lin, edges, E, index, n, &g);
  double cost = lin.cost;
  summary[0] = cost;
  int iterations = 0, successful = 0, termination = -1, invalid = 0;

  // Jacobi scaling from the first Jacobian.
  std::vector<double> scale(n, 0.);
  for (int64_t k = 0; k < E; ++k) {
    const int cols[2] = {index[edges[k].start], index[edges[k].end]};
    for (int side = 0; side < 2; ++side) {
      if (cols[side] < 0) continue;
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
          const double v = lin.J[18 * k + 6 * i + 3 * side + j];
          scale[cols[side] + j] += v * v;
        }
    }
  }
  for (int i = 0; i < n; ++i) scale[i] = 1. / (1. + std::sqrt(scale[i]));

  double radius = 1e4, decrease = 2.;
  // Monotonic steps only: the reference cost is the current cost.
  while (termination < 0) {
    if (iterations > 0 && iterations >= max_num_iterations) {
      termination = 3;
      break;
    }
    if (MaxAbs(g) <= 1e-10) {
      termination = 0;
      break;
    }
    if (iterations >= max_num_iterations) {
      termination = 3;
      break;
    }
    if (radius < 1e-32) {
      termination = 1;
      break;
    }
    ++iterations;
    // Normal matrix of the scaled Jacobian.
    std::vector<double> A(static_cast<size_t>(n) * n, 0.);
    for (int64_t k = 0; k < E; ++k) {
      const int cols[2] = {index[edges[k].start], index[edges[k].end]};
      for (int sa = 0; sa < 2; ++sa) {
        if (cols[sa] < 0) continue;
        for (int sb = 0; sb < 2; ++sb) {
          if (cols[sb] < 0) continue;
          for (int ja = 0; ja < 3; ++ja)
            for (int jb = 0; jb < 3; ++jb) {
              double sum = 0.;
              for (int i = 0; i < 3; ++i)
                sum += lin.J[18 * k + 6 * i + 3 * sa + ja] * lin.J[18 * k + 6 * i + 3 * sb + jb];
              const int ra = cols[sa] + ja, rb = cols[sb] + jb;
              A[static_cast<size_t>(ra) * n + rb] += scale[ra] * sum * scale[rb];
            }
        }
      }
    }
    for (int i = 0; i < n; ++i) {
      double& d = A[static_cast<size_t>(i) * n + i];
      d += std::fmin(std::fmax(d, 1e-6), 1e32) / radius;
    }
    std::vector<double> step(n);
    for (int i = 0; i < n; ++i) step[i] = -scale[i] * g[i];
    bool valid = Cholesky(&A, n);
    double model = 0.;
    if (valid) {
      CholeskySolve(A, n, &step);
      for (int i = 0; i < n; ++i) {
        step[i] *= scale[i];
        valid = valid && std::isfinite(step[i]);
      }
    }
    if (valid) {
      for (int64_t k = 0; k < E; ++k) {
        const int cols[2] = {index[edges[k].start], index[edges[k].end]};
        for (int i = 0; i < 3; ++i) {
          double m = 0.;
          for (int side = 0; side < 2; ++side)
            if (cols[side] >= 0)
              for (int j = 0; j < 3; ++j)
                m += lin.J[18 * k + 6 * i + 3 * side + j] * step[cols[side] + j];
          model -= m * (lin.r[3 * k + i] + m / 2.);
        }
      }
      valid = model > 0.;
    }
    if (!valid) {
      if (++invalid >= 5) {
        termination = 4;
        break;
      }
      radius /= decrease;
      decrease *= 2.;
      continue;
    }
    invalid = 0;
    double step_norm = 0., x_norm = 0.;
    candidate = x;
    for (int v = 0; v < V; ++v)
      if (index[v] >= 0)
        for (int j = 0; j < 3; ++j) {
          candidate[3 * v + j] += step[index[v] + j];
          step_norm += step[index[v] + j] * step[index[v] + j];
          x_norm += x[3 * v + j] * x[3 * v + j];
        }
    step_norm = std::sqrt(step_norm);
    x_norm = std::sqrt(x_norm);
    double candidate_cost = Evaluate(candidate.data(), edges, E, huber, nullptr, nullptr, nullptr);
    if (!std::isfinite(candidate_cost)) candidate_cost = DBL_MAX;
    if (step_norm <= 1e-8 * (x_norm + 1e-8)) {
      termination = 1;
      break;
    }
    if (std::fabs(cost - candidate_cost) <= 1e-6 * cost) {
      termination = 2;
      break;
    }
    const double quality = (cost - candidate_cost) / model;
    if (quality > 1e-3) {
      x = candidate;
      Evaluate(x.data(), edges, E, huber, &lin, nullptr, nullptr);
      Gradient(lin, edges, E, index, n, &g);
      cost = lin.cost;
      ++successful;
      const double t = 2. * quality - 1.;
      radius = std::fmin(1e16, radius / std::fmax(1. / 3., 1. - t * t * t));
      decrease = 2.;
    } else {
      radius /= decrease;
      decrease *= 2.;
    }
  }
  for (int i = 0; i < 3 * V; ++i) poses[i] = x[i];
  summary[1] = cost;
  summary[2] = iterations;
  summary[3] = successful;
  summary[4] = termination;
  summary[5] = MaxAbs(g);
  return 0;
}

}  // extern "C"
