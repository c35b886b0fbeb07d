// Test infrastructure: C entry points over three oracle symbols the oracle's
// own C API does not expose (oracle/csm_oracle.h): RayToPixelMask,
// LookupTableToApplyCorrespondenceCostOdds, and ProbabilityGridInserter2D::
// Insert with misses on a handle from oracle_grid_create. Built by the tests
// against oracle/_build/liboracle.so.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "csm_oracle.h"

using namespace oracle;

extern "C" {

// Cells (x, y) of one ray into out (capacity in cells); returns the count.
int64_t shim_ray_to_pixel_mask(int32_t bx, int32_t by, int32_t ex, int32_t ey, int32_t scale,
                               int32_t* out, int64_t capacity) {
  const std::vector<Idx2> mask = RayToPixelMask(Idx2{bx, by}, Idx2{ex, ey}, scale);
  const int64_t n = static_cast<int64_t>(mask.size());
  for (int64_t i = 0; i < n && i < capacity; ++i) {
    out[2 * i] = mask[i].x;
    out[2 * i + 1] = mask[i].y;
  }
  return static_cast<int64_t>(mask.size());
}

// ComputeLookupTableToApplyCorrespondenceCostOdds(Odds(probability)).
void shim_lookup_table(float probability, uint16_t* out32768) {
  const std::vector<uint16_t> t = LookupTableToApplyCorrespondenceCostOdds(Odds(probability));
  for (int i = 0; i < 32768; ++i) out32768[i] = t[i];
}

void shim_grid_insert(void* grid, float hit_p, float miss_p, int32_t insert_free_space,
                      const float* origin, const float* returns, int32_t num_returns,
                      const float* misses, int32_t num_misses) {
  RangeData rd;
  rd.origin = Vec3f{origin[0], origin[1], origin[2]};
  for (int32_t i = 0; i < num_returns; ++i)
    rd.returns.push_back(Vec3f{returns[3 * i], returns[3 * i + 1], returns[3 * i + 2]});
  for (int32_t i = 0; i < num_misses; ++i)
    rd.misses.push_back(Vec3f{misses[3 * i], misses[3 * i + 1], misses[3 * i + 2]});
  ProbabilityGridInserter2D(hit_p, miss_p, insert_free_space != 0)
      .Insert(rd, static_cast<ProbabilityGrid*>(grid));
}

}  // extern "C"
