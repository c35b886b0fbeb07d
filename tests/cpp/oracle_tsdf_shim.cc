// Test infrastructure: C entry points over oracle symbols its C API does not
// expose (oracle/oracle_tsdf.h): EstimateNormals, the TSDValueConverter round
// trips, the RangeDataSorter's comparator (restated here from
// tsdf_range_data_inserter_2d.cc:69-88) and TSDF2D::ComputeCroppedGrid
// (tsdf_2d.cc:118-135) restated from the oracle TSDF2D's public methods.
// Built by the tests against oracle/_build/liboracle.so.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "oracle_tsdf.h"

using namespace oracle;

namespace {

Vec2f Normalized(float x, float y) {  // Eigen Vector2f::normalized()
  const float sq = x * x + y * y;
  if (sq > 0.f) {
    const float n = std::sqrt(sq);
    return Vec2f{x / n, y / n};
  }
  return Vec2f{x, y};
}

// RangeDataSorter::operator() (:74-85).
bool Before(const float* origin, const float* l, const float* r) {
  const Vec2f dl = Normalized(l[0] - origin[0], l[1] - origin[1]);
  const Vec2f dr = Normalized(r[0] - origin[0], r[1] - origin[1]);
  if ((dl.y < 0.f) != (dr.y < 0.f)) return dl.y < 0.f;
  if (dl.y < 0.f) return dl.x < dr.x;
  return dl.x > dr.x;
}

MapLimits Limits(double res, double max_x, double max_y, int nx, int ny) {
  MapLimits l;
  l.resolution = res;
  l.max_x = max_x;
  l.max_y = max_y;
  l.cells = CellLimits{nx, ny};
  return l;
}

}  // namespace

extern "C" {

// Adjacent pairs (k, k + 1) of returns[order[.]] with the later one strictly
// before the earlier one under the comparator: 0 for a sorted sequence.
int32_t shim_tsdf_out_of_order(const float* origin, const float* returns, int32_t n,
                               const int32_t* order) {
  int32_t bad = 0;
  for (int32_t k = 0; k + 1 < n; ++k)
    if (Before(origin, returns + 3 * order[k + 1], returns + 3 * order[k])) ++bad;
  return bad;
}

// oracle::EstimateNormals of the returns as given (already in cast order).
void shim_tsdf_normals(const float* origin, const float* returns, int32_t n, int32_t num_samples,
                       float sample_radius, float* out) {
  RangeData rd;
  rd.origin = Vec3f{origin[0], origin[1], origin[2]};
  for (int32_t i = 0; i < n; ++i)
    rd.returns.push_back(Vec3f{returns[3 * i], returns[3 * i + 1], returns[3 * i + 2]});
  NormalEstimationOptions2D o;
  o.num_normal_samples = num_samples;
  o.sample_radius = sample_radius;
  const std::vector<float> normals = EstimateNormals(rd, o);
  for (int32_t i = 0; i < n; ++i) out[i] = normals[i];
}

// TSDToValue(ValueToTSD(v)) and WeightToValue(ValueToWeight(v)), v < 32768.
void shim_tsdf_round_trip(float truncation, float max_weight, uint16_t* tsd_out,
                          uint16_t* weight_out) {
  const TSDValueConverter conv(truncation, max_weight);
  for (int v = 0; v < 32768; ++v) {
    tsd_out[v] = conv.TSDToValue(conv.ValueToTSD(static_cast<uint16_t>(v)));
    weight_out[v] = conv.WeightToValue(conv.ValueToWeight(static_cast<uint16_t>(v)));
  }
}

// ComputeCroppedGrid of the TSDF2D given by its limits and planes. Writes the
// cropped limits (resolution, max_x, max_y), the cell counts, and the planes
// (capacity: cells per plane); returns the cropped cell count.
int64_t shim_tsdf_crop(double res, double max_x, double max_y, int32_t nx, int32_t ny,
                       float truncation, float max_weight, const uint16_t* tsd,
                       const uint16_t* weight, double* limits3, int32_t* cells2,
                       uint16_t* tsd_out, uint16_t* weight_out, int64_t capacity) {
  const size_t n = static_cast<size_t>(nx) * ny;
  const TSDF2D src(Limits(res, max_x, max_y, nx, ny), truncation, max_weight,
                   std::vector<uint16_t>(tsd, tsd + n), std::vector<uint16_t>(weight, weight + n));
  // Grid2D::ComputeCroppedLimits (grid_2d.cc:121-132): the known-cells box.
  bool empty = true;
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  for (int y = 0; y < ny; ++y)
    for (int x = 0; x < nx; ++x) {
      if (!src.IsKnown(Idx2{x, y})) continue;
      if (empty) {
        x0 = x1 = x;
        y0 = y1 = y;
        empty = false;
      } else {
        x0 = x < x0 ? x : x0;
        x1 = x > x1 ? x : x1;
        y0 = y < y0 ? y : y0;
        y1 = y > y1 ? y : y1;
      }
    }
  const Idx2 offset = empty ? Idx2{0, 0} : Idx2{x0, y0};
  const CellLimits cl = empty ? CellLimits{1, 1} : CellLimits{x1 - x0 + 1, y1 - y0 + 1};
  TSDF2D cropped(Limits(res, max_x - res * offset.y, max_y - res * offset.x, cl.num_x_cells,
                        cl.num_y_cells),
                 truncation, max_weight);
  for (int y = 0; y < cl.num_y_cells; ++y)
    for (int x = 0; x < cl.num_x_cells; ++x) {
      const Idx2 s{x + offset.x, y + offset.y};
      if (!src.IsKnown(s)) continue;
      cropped.SetCell(Idx2{x, y}, src.GetTSD(s), src.GetWeight(s));
    }
  cropped.FinishUpdate();
  limits3[0] = cropped.limits().resolution;
  limits3[1] = cropped.limits().max_x;
  limits3[2] = cropped.limits().max_y;
  cells2[0] = cl.num_x_cells;
  cells2[1] = cl.num_y_cells;
  const int64_t count = static_cast<int64_t>(cl.num_x_cells) * cl.num_y_cells;
  for (int64_t i = 0; i < count && i < capacity; ++i) {
    tsd_out[i] = cropped.tsd_cells()[i];
    weight_out[i] = cropped.weight_cells()[i];
  }
  return count;
}

}  // extern "C"
