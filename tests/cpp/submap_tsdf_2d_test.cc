// ActiveSubmaps2D of include/cartographer_amd/submap_2d.h with
// grid_type = TSDF. Driven by tests/test_submap_tsdf2d_gpu.py:
//   submap_tsdf_2d_test counts
//       submap_2d_test.cc:35-96 TheRightNumberOfRangeDataAreInserted restated
//       on TSDF submaps (num_range_data = 10, 200 empty scans).
//   submap_tsdf_2d_test insert <scans> <out> <num_range_data>
//       inserts the scans of the file (int32 count; per scan: origin 3 floats,
//       int32 n, n * 3 floats returns) and writes the first finished submap's
//       grid: 3 doubles (resolution, max x, max y), 2 int32 (nx, ny), the TSD
//       plane, the weight plane; then the real-time matcher's score and pose
//       (4 doubles) for the last scan's returns, taken relative to its
//       origin, on that submap's device TSDF from a pose 3 cm off.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "cartographer_amd/submap_2d.h"

using namespace cartographer_amd;

#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                    \
    }                                                              \
  } while (0)

static SubmapsOptions2D Options(int num_range_data) {
  SubmapsOptions2D o;
  o.num_range_data = num_range_data;
  o.resolution = 0.05f;
  o.grid_type = Grid2DView::GridType::TSDF;  // the inserter options keep their defaults
  return o;
}

static int Counts() {
  constexpr int kNumRangeData = 10;
  ActiveSubmaps2D submaps{Options(kNumRangeData)};
  std::set<std::shared_ptr<const Submap2D>> all_submaps;
  for (int i = 0; i != 200; ++i) {
    auto insertion_submaps = submaps.InsertRangeData(RangeData{});
    EXPECT(insertion_submaps.size() <= 2);
    for (const auto& submap : insertion_submaps) {
      EXPECT(submap->tsdf() != nullptr && submap->grid() == nullptr);
      all_submaps.insert(submap);
    }
    if (submaps.submaps().size() > 1)
      EXPECT(kNumRangeData <= submaps.submaps().front()->num_range_data());
  }
  EXPECT(submaps.submaps().size() == 2);
  size_t finished = 0;
  int unfinished = 0;
  for (const auto& submap : all_submaps) {
    if (submap->num_range_data() == kNumRangeData * 2) {
      ++finished;
      EXPECT(submap->insertion_finished());
      const csm_map_limits l = submap->tsdf()->limits();  // all unknown: cropped to 1 x 1
      EXPECT(l.num_x_cells == 1 && l.num_y_cells == 1);
    } else {
      EXPECT(kNumRangeData == submap->num_range_data());
      ++unfinished;
    }
  }
  EXPECT(finished == all_submaps.size() - 1);
  EXPECT(unfinished == 1);
  std::printf("OK %zu submaps\n", all_submaps.size());
  return 0;
}

static int Insert(const char* scans_path, const char* out_path, int num_range_data) {
  std::FILE* f = std::fopen(scans_path, "rb");
  EXPECT(f != nullptr);
  int32_t count = 0;
  EXPECT(std::fread(&count, sizeof(count), 1, f) == 1);
  ActiveSubmaps2D submaps{Options(num_range_data)};
  std::shared_ptr<const Submap2D> first;
  RangeData rd;
  for (int32_t i = 0; i < count; ++i) {
    EXPECT(std::fread(rd.origin, sizeof(float), 3, f) == 3);
    int32_t n = 0;
    EXPECT(std::fread(&n, sizeof(n), 1, f) == 1 && n >= 0);
    rd.returns.xyz.resize(3 * static_cast<size_t>(n));
    EXPECT(n == 0 ||
           std::fread(rd.returns.xyz.data(), sizeof(float), rd.returns.xyz.size(), f) ==
               rd.returns.xyz.size());
    const auto insertion_submaps = submaps.InsertRangeData(rd);
    EXPECT(insertion_submaps.size() <= 2);
    if (!first && insertion_submaps.front()->insertion_finished()) first = insertion_submaps.front();
  }
  std::fclose(f);
  EXPECT(first != nullptr && first->tsdf() != nullptr);
  EXPECT(first->num_range_data() == 2 * num_range_data);
  const csm_map_limits l = first->tsdf()->limits();
  std::vector<uint16_t> tsd, weight;
  first->tsdf()->cells(&tsd, &weight);

  PointCloud cloud;
  for (size_t i = 0; i < rd.returns.size(); ++i)
    cloud.push_back(rd.returns.xyz[3 * i] - rd.origin[0], rd.returns.xyz[3 * i + 1] - rd.origin[1],
                    0.f);
  const RealTimeCorrelativeScanMatcher2D matcher{RealTimeCorrelativeScanMatcherOptions{}};
  Rigid2d pose;
  const double score = matcher.Match(Rigid2d{rd.origin[0] + 0.03, rd.origin[1] - 0.02, 0.01}, cloud,
                                     *first->tsdf(), &pose);

  std::FILE* out = std::fopen(out_path, "wb");
  EXPECT(out != nullptr);
  const double limits[3] = {l.resolution, l.max_x, l.max_y};
  const int32_t cells[2] = {l.num_x_cells, l.num_y_cells};
  const double match[4] = {score, pose.x, pose.y, pose.theta};
  std::fwrite(limits, sizeof(double), 3, out);
  std::fwrite(cells, sizeof(int32_t), 2, out);
  std::fwrite(tsd.data(), sizeof(uint16_t), tsd.size(), out);
  std::fwrite(weight.data(), sizeof(uint16_t), weight.size(), out);
  std::fwrite(match, sizeof(double), 4, out);
  std::fclose(out);
  std::printf("OK %d x %d\n", l.num_x_cells, l.num_y_cells);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "counts") return Counts();
  if (mode == "insert" && argc == 5) return Insert(argv[2], argv[3], std::atoi(argv[4]));
  std::printf("usage: submap_tsdf_2d_test counts | insert <scans> <out> <num_range_data>\n");
  return 2;
}
