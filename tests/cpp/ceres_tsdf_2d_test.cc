// TSDF submaps through loop-closure search and refinement with the C++
// drop-ins. Driven by tests/test_ceres_tsdf_dropin_gpu.py:
//   ceres_tsdf_2d_test <scans> <num_range_data>
// inserts the scans of the file (format of submap_tsdf_2d_test) into
// ActiveSubmaps2D(TSDF) and takes the first finished submap. Then
//   * FastMatcherFor(TSDF2D) gives a TSDF handle; csm_fast2d_match_batch and
//     csm_ceres2d_refine_batch on it are the direct result;
//   * ConstraintBuilder2D with refine_with_ceres, fed the submap's planes as a
//     TSDF Grid2DView, must return exactly those poses as constraints;
//   * CeresScanMatcher2D::Match on the live (unfinished) active TSDF must equal
//     the same Match on that grid's planes read back as a Grid2DView.
// Prints "OK <constraints>" or the failed expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cartographer_amd/constraint_builder_2d.h"
#include "cartographer_amd/submap_2d.h"

using namespace cartographer_amd;

#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                    \
    }                                                              \
  } while (0)

struct Scan {
  float origin[3];
  PointCloud returns;
};

// The scan's returns in its sensor frame, every `stride`-th.
static PointCloud SensorCloud(const Scan& s, size_t stride) {
  PointCloud cloud;
  for (size_t i = 0; i < s.returns.size(); i += stride)
    cloud.push_back(s.returns.xyz[3 * i] - s.origin[0], s.returns.xyz[3 * i + 1] - s.origin[1], 0.f);
  return cloud;
}

static Grid2DView TsdfView(const csm_map_limits& l, const std::vector<uint16_t>& tsd,
                           const std::vector<uint16_t>& weight,
                           const TSDFRangeDataInserterOptions2D& o) {
  Grid2DView v;
  v.grid_type = Grid2DView::GridType::TSDF;
  v.resolution = l.resolution;
  v.max_x = l.max_x;
  v.max_y = l.max_y;
  v.num_x_cells = l.num_x_cells;
  v.num_y_cells = l.num_y_cells;
  v.cells = tsd.data();
  v.weight_cells = weight.data();
  v.min_correspondence_cost = -static_cast<float>(o.truncation_distance);
  v.max_correspondence_cost = static_cast<float>(o.truncation_distance);
  v.max_weight = static_cast<float>(o.maximum_weight);
  return v;
}

static bool Same(const Rigid2d& a, const csm_pose2d& b) {
  return a.x == b.x && a.y == b.y && a.theta == b.theta;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: ceres_tsdf_2d_test <scans> <num_range_data>\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  EXPECT(f != nullptr);
  int32_t count = 0;
  EXPECT(std::fread(&count, sizeof(count), 1, f) == 1 && count > 0);
  std::vector<Scan> scans(static_cast<size_t>(count));
  for (Scan& s : scans) {
    EXPECT(std::fread(s.origin, sizeof(float), 3, f) == 3);
    int32_t n = 0;
    EXPECT(std::fread(&n, sizeof(n), 1, f) == 1 && n > 0);
    s.returns.xyz.resize(3 * static_cast<size_t>(n));
    EXPECT(std::fread(s.returns.xyz.data(), sizeof(float), s.returns.xyz.size(), f) ==
           s.returns.xyz.size());
  }
  std::fclose(f);

  SubmapsOptions2D so;
  so.num_range_data = std::atoi(argv[2]);
  so.resolution = 0.05f;
  so.grid_type = Grid2DView::GridType::TSDF;
  ActiveSubmaps2D active{so};
  std::shared_ptr<const Submap2D> first, live;
  RangeData rd;
  for (const Scan& s : scans) {
    for (int k = 0; k < 3; ++k) rd.origin[k] = s.origin[k];
    rd.returns = s.returns;
    const auto insertion_submaps = active.InsertRangeData(rd);
    if (!first && insertion_submaps.front()->insertion_finished()) first = insertion_submaps.front();
    live = insertion_submaps.back();
  }
  EXPECT(first != nullptr && first->tsdf() != nullptr);
  EXPECT(live != nullptr && live->tsdf() != nullptr && !live->insertion_finished());

  // ---- the batch API called directly on FastMatcherFor's handle ----------------
  ConstraintBuilderOptions bo;
  bo.sampling_ratio = 1.;
  bo.min_score = 0.5f;
  bo.fast_correlative_scan_matcher_options = FastCorrelativeScanMatcherOptions2D{0.5, 0.2, 3};
  bo.log_matches = false;
  csm_context* ctx = first->tsdf()->context();
  csm_fast2d* handle = FastMatcherFor(*first->tsdf(), bo.fast_correlative_scan_matcher_options);
  EXPECT(handle != nullptr);

  const size_t num_nodes = 4;
  EXPECT(scans.size() >= num_nodes);
  std::vector<PointCloud> clouds;
  std::vector<Rigid2d> initial;  // map <- node; the submap's local pose is the identity
  std::vector<float> xyz;
  std::vector<int64_t> offsets{0};
  for (size_t i = 0; i < num_nodes; ++i) {
    clouds.push_back(SensorCloud(scans[i], 6));
    initial.push_back(Rigid2d{scans[i].origin[0] + 0.06, scans[i].origin[1] - 0.04, 0.02});
    xyz.insert(xyz.end(), clouds[i].xyz.begin(), clouds[i].xyz.end());
    offsets.push_back(offsets.back() + static_cast<int64_t>(clouds[i].size()));
  }
  csm_scan_set* set = nullptr;
  CheckOk(csm_scan_set_create(ctx, xyz.data(), offsets.data(), static_cast<int32_t>(num_nodes), &set),
          "csm_scan_set_create");
  std::vector<csm_pair2d> pairs(num_nodes);
  for (size_t i = 0; i < num_nodes; ++i) {
    pairs[i] = csm_pair2d{};
    pairs[i].scan = static_cast<int32_t>(i);
    pairs[i].min_score = bo.min_score;
    pairs[i].initial = csm_pose2d{initial[i].x, initial[i].y, initial[i].theta};
  }
  std::vector<csm_result2d> matched(num_nodes);
  CheckOk(csm_fast2d_match_batch(ctx, &handle, 1, set, pairs.data(), static_cast<int64_t>(num_nodes),
                                 matched.data()),
          "csm_fast2d_match_batch");
  std::vector<csm_refine2d> items;
  for (size_t i = 0; i < num_nodes; ++i) {
    EXPECT(matched[i].status == CSM_OK);
    items.push_back(csm_refine2d{0, static_cast<int32_t>(i), matched[i].pose, matched[i].pose.x,
                                 matched[i].pose.y});
  }
  std::vector<csm_pose2d> refined(num_nodes);
  std::vector<int32_t> iterations(num_nodes);
  CheckOk(csm_ceres2d_refine_batch(ctx, &handle, 1, set, items.data(),
                                   static_cast<int64_t>(num_nodes), &bo.ceres_scan_matcher_options,
                                   refined.data(), iterations.data()),
          "csm_ceres2d_refine_batch");
  int moved = 0;
  for (size_t i = 0; i < num_nodes; ++i) {
    EXPECT(iterations[i] >= 1);  // the TSDF cost evaluated and the solver ran
    if (refined[i].x != matched[i].pose.x || refined[i].theta != matched[i].pose.theta) ++moved;
  }
  EXPECT(moved > 0);
  csm_scan_set_destroy(set);
  csm_fast2d_destroy(handle);

  // ---- ConstraintBuilder2D over the same submap as a TSDF view -----------------
  std::vector<uint16_t> tsd, weight;
  first->tsdf()->cells(&tsd, &weight);
  Submap2DView view;
  view.grid = TsdfView(first->tsdf()->limits(), tsd, weight, so.tsdf_range_data_inserter_options);
  ConstraintBuilder2D builder(bo, ctx);
  for (size_t i = 0; i < num_nodes; ++i) {
    builder.MaybeAddConstraint(SubmapId{0, 0}, &view, NodeId{0, static_cast<int>(i)}, &clouds[i],
                               initial[i]);
    builder.NotifyEndOfNode();
  }
  ConstraintBuilder2D::Result result;
  builder.WhenDone([&](const ConstraintBuilder2D::Result& r) { result = r; });
  EXPECT(result.size() == num_nodes);
  for (size_t i = 0; i < num_nodes; ++i) {
    EXPECT(result[i].node_id.node_index == static_cast<int>(i));
    EXPECT(result[i].score == matched[i].score);
    // local_pose is the identity: Compose(Inverse(identity), pose) == pose up to -0.0.
    EXPECT(Same(result[i].relative_pose, refined[i]));
  }

  // ---- CeresScanMatcher2D::Match on the live active grid -----------------------
  const CeresScanMatcher2D ceres{CeresScanMatcherOptions2D{}};
  const Scan& last = scans.back();
  const PointCloud cloud = SensorCloud(last, 4);
  const Rigid2d start{last.origin[0] + 0.03, last.origin[1] - 0.02, 0.01};
  const double target[2] = {start.x, start.y};
  Rigid2d on_device, on_view;
  int it_device = 0, it_view = 0;
  ceres.Match(target, start, cloud, *live->tsdf(), &on_device, &it_device);
  std::vector<uint16_t> live_tsd, live_weight;
  live->tsdf()->cells(&live_tsd, &live_weight);
  const Grid2DView live_view = TsdfView(live->tsdf()->limits(), live_tsd, live_weight,
                                        so.tsdf_range_data_inserter_options);
  ceres.Match(target, start, cloud, live_view, &on_view, &it_view);
  EXPECT(it_device >= 1 && it_device == it_view);
  EXPECT(on_device.x == on_view.x && on_device.y == on_view.y && on_device.theta == on_view.theta);
  EXPECT(on_device.x != start.x || on_device.theta != start.theta);

  std::printf("OK %zu constraints, live match %d iterations\n", result.size(), it_device);
  return 0;
}
