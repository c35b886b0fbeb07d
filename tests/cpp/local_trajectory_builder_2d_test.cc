// The C++ drop-in of LocalTrajectoryBuilder2D
// (include/cartographer_amd/local_trajectory_builder_2d.h) run from a script
// file written by tests/test_local_trajectory_builder_2d_gpu.py: options, then
// per AddRangeData call its inputs and the extrapolator's answers in the order
// the builder asks for them. Prints one line per call ("N", or "R" with the
// time, the local pose, whether the scan was inserted, the sizes and a checksum
// of the range data in the local frame, and a checksum of the node's cloud) and
// one "G" line per active submap, which the test compares with the Python
// mirror's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "cartographer_amd/local_trajectory_builder_2d.h"

namespace ca = cartographer_amd;

namespace {

struct Reader {
  std::vector<char> data;
  size_t at = 0;
  template <typename T>
  T Get() {
    T v;
    if (at + sizeof(T) > data.size()) {
      std::fprintf(stderr, "script too short\n");
      std::exit(2);
    }
    std::memcpy(&v, data.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
};

// Replays the answers the script recorded, in order.
class ReplayExtrapolator : public ca::PoseExtrapolatorInterface {
 public:
  struct Answer {
    double time;
    ca::Rigid3d pose;
  };
  ReplayExtrapolator(double start_time, const ca::Quaterniond& gravity)
      : last_pose_time_(start_time), last_extrapolated_time_(start_time), gravity_(gravity) {}

  double GetLastPoseTime() const override { return last_pose_time_; }
  double GetLastExtrapolatedTime() const override { return last_extrapolated_time_; }
  ca::Rigid3d ExtrapolatePose(double time) override {
    if (answers.empty() || answers.front().time != time) {
      std::fprintf(stderr, "unexpected ExtrapolatePose(%.17g)\n", time);
      std::exit(3);
    }
    const ca::Rigid3d pose = answers.front().pose;
    answers.pop_front();
    last_extrapolated_time_ = time;
    return pose;
  }
  ca::Quaterniond EstimateGravityOrientation(double) override { return gravity_; }
  void AddPose(double time, const ca::Rigid3d&) override { last_pose_time_ = time; }

  std::deque<Answer> answers;

 private:
  double last_pose_time_, last_extrapolated_time_;
  ca::Quaterniond gravity_;
};

// sum((i + 1) * word_i) mod 2^64.
template <typename T>
void Checksum(const T* words, size_t count, uint64_t* index, uint64_t* sum) {
  for (size_t i = 0; i < count; ++i) *sum += ++*index * static_cast<uint64_t>(words[i]);
}
uint64_t ChecksumFloats(std::initializer_list<const std::vector<float>*> parts, const float* head) {
  uint64_t index = 0, sum = 0;
  uint32_t w[3];
  if (head) {
    std::memcpy(w, head, sizeof(w));
    Checksum(w, 3, &index, &sum);
  }
  for (const std::vector<float>* part : parts) {
    std::vector<uint32_t> words(part->size());
    if (!words.empty()) std::memcpy(words.data(), part->data(), 4 * words.size());
    Checksum(words.data(), words.size(), &index, &sum);
  }
  return sum;
}
uint64_t ChecksumCells(const std::vector<uint16_t>& cells) {
  uint64_t index = 0, sum = 0;
  Checksum(cells.data(), cells.size(), &index, &sum);
  return sum;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Reader r;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0)
      r.data.insert(r.data.end(), buf, buf + got);
    std::fclose(f);
  }
  ca::LocalTrajectoryBuilderOptions2D o;
  const bool tsdf = r.Get<int32_t>() != 0;
  o.submaps_options.num_range_data = r.Get<int32_t>();
  o.submaps_options.grid_type =
      tsdf ? ca::Grid2DView::GridType::TSDF : ca::Grid2DView::GridType::PROBABILITY_GRID;
  o.num_accumulated_range_data = r.Get<int32_t>();
  o.use_online_correlative_scan_matching = r.Get<int32_t>() != 0;
  o.min_range = r.Get<float>();
  o.max_range = r.Get<float>();
  o.missing_data_ray_length = r.Get<float>();
  o.min_z = r.Get<float>();
  o.max_z = r.Get<float>();
  o.voxel_filter_size = r.Get<float>();
  o.adaptive_voxel_filter_options.max_length = r.Get<float>();
  o.adaptive_voxel_filter_options.min_num_points = r.Get<float>();
  o.adaptive_voxel_filter_options.max_range = r.Get<float>();
  o.real_time_correlative_scan_matcher_options.linear_search_window = r.Get<double>();
  o.real_time_correlative_scan_matcher_options.angular_search_window = r.Get<double>();
  o.real_time_correlative_scan_matcher_options.translation_delta_cost_weight = r.Get<double>();
  o.real_time_correlative_scan_matcher_options.rotation_delta_cost_weight = r.Get<double>();
  o.ceres_scan_matcher_options.occupied_space_weight = r.Get<double>();
  o.ceres_scan_matcher_options.translation_weight = r.Get<double>();
  o.ceres_scan_matcher_options.rotation_weight = r.Get<double>();
  o.ceres_scan_matcher_options.max_num_iterations = r.Get<int32_t>();
  o.ceres_scan_matcher_options.use_nonmonotonic_steps = r.Get<int32_t>() != 0;
  o.motion_filter_options.max_time_seconds = r.Get<double>();
  o.motion_filter_options.max_distance_meters = r.Get<double>();
  o.motion_filter_options.max_angle_radians = r.Get<double>();
  const double start_time = r.Get<double>();
  ca::Quaterniond gravity;
  gravity.w = r.Get<double>();
  gravity.x = r.Get<double>();
  gravity.y = r.Get<double>();
  gravity.z = r.Get<double>();

  ReplayExtrapolator extrapolator(start_time, gravity);
  ca::LocalTrajectoryBuilder2D builder(o, &extrapolator);
  const int32_t num_calls = r.Get<int32_t>();
  for (int32_t c = 0; c < num_calls; ++c) {
    const double time = r.Get<double>();
    std::vector<float> origins(3 * static_cast<size_t>(r.Get<int32_t>()));
    for (float& v : origins) v = r.Get<float>();
    std::vector<ca::RangeMeasurement> ranges(static_cast<size_t>(r.Get<int32_t>()));
    for (ca::RangeMeasurement& m : ranges) {
      for (float& v : m.position) v = r.Get<float>();
      m.time = r.Get<float>();
    }
    for (ca::RangeMeasurement& m : ranges) m.origin_index = r.Get<int32_t>();
    const int32_t num_answers = r.Get<int32_t>();
    for (int32_t a = 0; a < num_answers; ++a) {
      ReplayExtrapolator::Answer answer;
      answer.time = r.Get<double>();
      for (double& v : answer.pose.t) v = r.Get<double>();
      answer.pose.rotation.w = r.Get<double>();
      answer.pose.rotation.x = r.Get<double>();
      answer.pose.rotation.y = r.Get<double>();
      answer.pose.rotation.z = r.Get<double>();
      extrapolator.answers.push_back(answer);
    }
    const auto result = builder.AddRangeData(time, origins, ranges);
    if (!extrapolator.answers.empty()) {
      std::fprintf(stderr, "call %d left %zu answers unasked\n", c, extrapolator.answers.size());
      return 3;
    }
    if (!result) {
      std::printf("N\n");
      continue;
    }
    const ca::RangeData& rd = result->range_data_in_local;
    const ca::Rigid3d& p = result->local_pose;
    std::printf("R %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %zu %zu %llu %llu\n",
                result->time, p.t[0], p.t[1], p.t[2], p.rotation.w, p.rotation.x, p.rotation.y,
                p.rotation.z, result->insertion_result ? 1 : 0, rd.returns.size(),
                rd.misses.size(),
                static_cast<unsigned long long>(
                    ChecksumFloats({&rd.returns.xyz, &rd.misses.xyz}, rd.origin)),
                static_cast<unsigned long long>(
                    result->insertion_result
                        ? ChecksumFloats({&result->insertion_result->constant_data
                                               ->filtered_gravity_aligned_point_cloud.xyz},
                                         nullptr)
                        : 0));
  }
  for (const auto& submap : builder.active_submaps().submaps()) {
    if (submap->grid()) {
      const csm_map_limits l = submap->grid()->limits();
      std::printf("G %d %d %d %d %llu\n", l.num_x_cells, l.num_y_cells, submap->num_range_data(),
                  submap->insertion_finished() ? 1 : 0,
                  static_cast<unsigned long long>(ChecksumCells(submap->grid()->cells())));
    } else {
      const csm_map_limits l = submap->tsdf()->limits();
      std::vector<uint16_t> tsd, weight;
      submap->tsdf()->cells(&tsd, &weight);
      std::printf("G %d %d %d %d %llu %llu\n", l.num_x_cells, l.num_y_cells,
                  submap->num_range_data(), submap->insertion_finished() ? 1 : 0,
                  static_cast<unsigned long long>(ChecksumCells(tsd)),
                  static_cast<unsigned long long>(ChecksumCells(weight)));
    }
  }
  return 0;
}
