// ConstraintBuilder2D drop-in over the batched C-ABI.
//
// Mirrors mapping/internal/constraints/constraint_builder_2d.{h,cc}: the
// public methods, the distance filter and per-submap FixedRatioSampler of
// MaybeAddConstraint (:77-112), MaybeAddGlobalConstraint (:114-137),
// NotifyEndOfNode (:139-151), WhenDone (:153-163) with results in submission
// order and failures dropped (:279-300), GetNumFinishedNodes (:302-305),
// DeleteScanMatcher (:307-316), the per-submap matcher cache
// (DispatchScanMatcherConstruction :165-186), the metrics (:46-53,
// RegisterMetrics :318-343: constraint counters, queue-length and matcher
// gauges, local and global score histograms), the score histogram and the
// log_matches lines (:239, :260-276, :289-293). Instead of one Task per pair on common::ThreadPool, pending pairs
// are searched as one GPU batch when a node ends (or when `flush_pairs` are
// pending). Accepted matches are then refined as one batch by the
// CeresScanMatcher2D restatement of ComputeConstraint (:245-249;
// csm_ceres2d_refine_batch, parity with Ceres unpinned) unless
// options.refine_with_ceres is off. The cost follows the submap's grid type as
// ceres_scan_matcher_2d.cc:74-91 does: a TSDF view with its weights makes a
// TSDF matcher, whose items are refined with TSDFMatchCostFunction2D; one
// flush may mix TSDF and probability-grid submaps.
//
// Lifetimes: the Submap2DView and PointCloud passed to MaybeAdd* must stay
// valid (and unchanged) until the flush that searches the pair — the next
// NotifyEndOfNode that flushes, or WhenDone — as the reference's tasks read
// them until they run. Matchers are built from the view when the pair is
// enqueued (kStatic) or searched (kClaim, or after the budgeted matcher cache
// dropped the submap's matcher: options.matcher_cache_bytes, MatcherCache).
// DeleteScanMatcher drops the submap's pending pairs.
//
// Multi-GPU (set_communicator): every rank makes the same calls; a rank
// searches only the pairs of the submaps it owns (ShardOwner, Sharding::kStatic)
// or the chunks of each flush it claims (Sharding::kClaim) on its own device,
// and WhenDone gathers the accepted constraints to rank 0 in submission order
// (constraint_gather.h). Rank 0's callback gets the whole
// result, the other ranks' callbacks an empty one; the metric counters are
// summed over the ranks and last_error reduced over them at every WhenDone.
//
// All of that but the 2D types, the device batch, the resident scan set and
// the log texts lives in ConstraintBuilderBase (constraint_builder_base.h).
#ifndef CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_2D_H_
#define CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_2D_H_

#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "constraint_builder_base.h"
#include "scan_matching.h"

namespace cartographer_amd {

// What the builder reads of a Submap2D: its grid and ComputeSubmapPose(),
// i.e. Project2D(submap.local_pose()) (constraint_builder_2d.cc:55-57).
struct Submap2DView {
  Grid2DView grid;
  Rigid2d local_pose;
};

// PoseGraphInterface::Constraint (pose_graph_interface.h:36-53), 2D pose.
struct Constraint {
  SubmapId submap_id;
  NodeId node_id;
  Rigid2d relative_pose;  // submap <- node (Embed3D of this in the reference)
  double translation_weight = 0., rotation_weight = 0.;
  enum Tag { INTRA_SUBMAP, INTER_SUBMAP } tag = INTER_SUBMAP;
  float score = 0.f;
};

inline Rigid2d Compose(const Rigid2d& a, const Rigid2d& b) {
  const double c = std::cos(a.theta), s = std::sin(a.theta);
  return Rigid2d{c * b.x + (-s) * b.y + a.x, s * b.x + c * b.y + a.y, a.theta + b.theta};
}
inline Rigid2d Inverse(const Rigid2d& a) {
  const double c = std::cos(-a.theta), s = std::sin(-a.theta);
  return Rigid2d{-(c * a.x + (-s) * a.y), -(s * a.x + c * a.y), -a.theta};
}

struct ConstraintBuilder2DTraits {
  using Constraint = cartographer_amd::Constraint;
  using Record = ConstraintRecord;
  using Matcher = FastCorrelativeScanMatcher2D;
  struct Payload {
    const Submap2DView* submap;
    const PointCloud* cloud;
    Rigid2d initial;  // the search start, map <- node
  };
  static constexpr const char* kName = "ConstraintBuilder2D";
  static constexpr const char* kMetricPrefix = "mapping_constraints_constraint_builder_2d";
  static constexpr const char* kScoreKinds[] = {nullptr};
  static constexpr int kClaimNamespace = 0;
};

class ConstraintBuilder2D
    : public ConstraintBuilderBase<ConstraintBuilder2D, ConstraintBuilder2DTraits> {
 public:
  explicit ConstraintBuilder2D(const ConstraintBuilderOptions& options,
                               csm_context* context = nullptr)
      : ConstraintBuilderBase(options, context) {}

  ~ConstraintBuilder2D() {
    if (scans_) csm_scan_set_destroy(scans_);
  }

  void MaybeAddConstraint(const SubmapId& submap_id, const Submap2DView* submap,
                          const NodeId& node_id, const PointCloud* cloud,
                          const Rigid2d& initial_relative_pose) {
    if (std::hypot(initial_relative_pose.x, initial_relative_pose.y) >
        options_.max_constraint_distance)
      return;
    if (!Sample(submap_id)) return;
    Enqueue(submap_id, node_id, false,
            Payload{submap, cloud, Compose(submap->local_pose, initial_relative_pose)});
  }

  void MaybeAddGlobalConstraint(const SubmapId& submap_id, const Submap2DView* submap,
                                const NodeId& node_id, const PointCloud* cloud) {
    Enqueue(submap_id, node_id, true, Payload{submap, cloud, Rigid2d::Identity()});
  }

 private:
  friend class ConstraintBuilderBase<ConstraintBuilder2D, ConstraintBuilder2DTraits>;

  // DispatchScanMatcherConstruction (constraint_builder_2d.cc:165-186).
  std::shared_ptr<FastCorrelativeScanMatcher2D> MakeMatcher(const Payload& p) {
    return std::make_shared<FastCorrelativeScanMatcher2D>(
        p.submap->grid, options_.fast_correlative_scan_matcher_options, context_);
  }

  static ConstraintRecord ToRecord(const Constraint& c) {
    ConstraintRecord r{};
    r.submap_trajectory = c.submap_id.trajectory_id;
    r.submap_index = c.submap_id.submap_index;
    r.node_trajectory = c.node_id.trajectory_id;
    r.node_index = c.node_id.node_index;
    r.x = c.relative_pose.x;
    r.y = c.relative_pose.y;
    r.theta = c.relative_pose.theta;
    r.score = c.score;
    r.tag = static_cast<int32_t>(c.tag);
    return r;
  }
  static Constraint FromRecord(const ConstraintRecord& r) {
    Constraint c;
    c.submap_id = SubmapId{r.submap_trajectory, r.submap_index};
    c.node_id = NodeId{r.node_trajectory, r.node_index};
    c.relative_pose = Rigid2d{r.x, r.y, r.theta};
    c.tag = static_cast<Constraint::Tag>(r.tag);
    c.score = r.score;
    return c;
  }

  void LogWhenDone(size_t computations, size_t constraints) {  // RunWhenDoneCallback (:289-293)
    log_(std::to_string(computations) + " computations resulted in " +
         std::to_string(constraints) + " additional constraints.");
    log_("Score histogram:\n" + score_histograms_[0].ToString(10));
  }

  // Device index of every pending_[which_pending[k]]'s cloud in scans_, which
  // keeps node clouds resident across flushes: clouds not seen before (or a
  // node whose cloud changed) are appended in one upload.
  // A cached cloud is reused only if it is the same PointCloud with the same
  // size and content hash, so a caller refilling one PointCloud object for a
  // node is uploaded again (the Python mirror compares the points).
  static uint64_t CloudHash(const PointCloud& c) {
    uint64_t h = 1469598103934665603ull;  // FNV-1a over the float bytes
    const unsigned char* b = reinterpret_cast<const unsigned char*>(c.xyz.data());
    for (size_t i = 0, n = c.xyz.size() * sizeof(float); i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
  }
  std::vector<int32_t> ResidentScans(const std::vector<size_t>& which_pending) {
    std::map<const PointCloud*, uint64_t> hashes;
    auto hash_of = [&](const PointCloud* c) {
      auto it = hashes.find(c);
      if (it == hashes.end()) it = hashes.emplace(c, CloudHash(*c)).first;
      return it->second;
    };
    auto stale = [&](const CachedScan& c, const PointCloud* cloud) {
      return c.index == kUnset || c.cloud != cloud || c.size != cloud->size() ||
             c.hash != hash_of(cloud);
    };
    int64_t fresh_points = 0;
    for (size_t i : which_pending) {
      auto c = scan_cache_.find(pending_[i].node_id);
      if (c == scan_cache_.end() || stale(c->second, pending_[i].cloud))
        fresh_points += static_cast<int64_t>(pending_[i].cloud->size());
    }
    if (scans_ && cached_points_ + fresh_points > options_.scan_cache_points) {
      csm_scan_set_destroy(scans_);
      scans_ = nullptr;
      scan_cache_.clear();
      cached_points_ = 0;
    }
    if (!scans_) {
      const int64_t zero = 0;
      CheckOk(csm_scan_set_create(context_, nullptr, &zero, 0, &scans_), "csm_scan_set_create");
    }
    std::vector<float> xyz;
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> index;  // >= 0: resident; < 0: -1 - (k-th cloud of this upload)
    std::vector<CachedScan*> fresh;
    for (size_t i : which_pending) {
      const Pending& p = pending_[i];
      CachedScan& c = scan_cache_[p.node_id];
      if (stale(c, p.cloud)) {
        c.cloud = p.cloud;
        c.size = p.cloud->size();
        c.hash = hash_of(p.cloud);
        c.index = -static_cast<int32_t>(offsets.size());
        fresh.push_back(&c);
        xyz.insert(xyz.end(), p.cloud->xyz.begin(), p.cloud->xyz.end());
        offsets.push_back(offsets.back() + static_cast<int64_t>(p.cloud->size()));
      }
      index.push_back(c.index);
    }
    if (offsets.size() > 1) {
      int32_t first = 0;
      CheckOk(csm_scan_set_append(scans_, xyz.data(), offsets.data(),
                                  static_cast<int32_t>(offsets.size() - 1), &first),
              "csm_scan_set_append");
      cached_points_ += offsets.back();
      for (int32_t& k : index)
        if (k < 0) k = first - 1 - k;
      for (CachedScan* c : fresh) c->index = first - 1 - c->index;
    }
    return index;
  }

  // Searches (and refines) pending_[which] as one batch over `held`'s matchers.
  std::vector<Outcome> RunBatch(const std::vector<size_t>& which_pending, const Held& held) {
    const std::vector<int32_t> scan_index = ResidentScans(which_pending);
    std::vector<csm_fast2d*> handles;
    std::map<SubmapId, int> slot_of;
    std::vector<csm_pair2d> pairs;
    for (size_t k = 0; k < which_pending.size(); ++k) {
      const Pending& p = pending_[which_pending[k]];
      auto s = slot_of.find(p.submap_id);
      if (s == slot_of.end()) {
        s = slot_of.emplace(p.submap_id, static_cast<int>(handles.size())).first;
        handles.push_back(held.at(p.submap_id)->handle());
      }
      csm_pair2d q{};
      q.submap = s->second;
      q.scan = scan_index[k];
      q.full_submap = p.full ? 1 : 0;
      q.min_score = p.full ? options_.global_localization_min_score : options_.min_score;
      q.initial = csm_pose2d{p.initial.x, p.initial.y, p.initial.theta};
      pairs.push_back(q);
    }
    std::vector<csm_result2d> results(pairs.size());
    CheckOk(csm_fast2d_match_batch(context_, handles.data(), static_cast<int32_t>(handles.size()),
                                   scans_, pairs.data(), static_cast<int64_t>(pairs.size()),
                                   results.data()),
            "csm_fast2d_match_batch");
    // CeresScanMatcher2D::Match(pose.translation(), pose, cloud, grid) on the accepted ones.
    if (options_.refine_with_ceres) {
      std::vector<csm_refine2d> items;
      std::vector<size_t> which;
      for (size_t i = 0; i < pairs.size(); ++i)
        if (results[i].status == CSM_OK) {
          items.push_back(csm_refine2d{pairs[i].submap, pairs[i].scan, results[i].pose,
                                       results[i].pose.x, results[i].pose.y});
          which.push_back(i);
        }
      std::vector<csm_pose2d> out(items.size());
      if (!items.empty())
        CheckOk(csm_ceres2d_refine_batch(context_, handles.data(),
                                         static_cast<int32_t>(handles.size()), scans_,
                                         items.data(), static_cast<int64_t>(items.size()),
                                         &options_.ceres_scan_matcher_options, out.data(),
                                         nullptr),
                "csm_ceres2d_refine_batch");
      for (size_t k = 0; k < which.size(); ++k) results[which[k]].pose = out[k];
    }
    std::vector<Outcome> outcomes(results.size());
    for (size_t i = 0; i < results.size(); ++i) {
      const Pending& p = pending_[which_pending[i]];
      Outcome& o = outcomes[i];
      o.status = results[i].status;
      if (o.status != CSM_OK) continue;
      o.scores[0] = results[i].score;
      const Rigid2d pose{results[i].pose.x, results[i].pose.y, results[i].pose.theta};
      Constraint& c = o.constraint;
      c.submap_id = p.submap_id;
      c.node_id = p.node_id;
      c.relative_pose = Compose(Inverse(p.submap->local_pose), pose);
      c.translation_weight = options_.loop_closure_translation_weight;
      c.rotation_weight = options_.loop_closure_rotation_weight;
      c.tag = Constraint::INTER_SUBMAP;
      c.score = results[i].score;
      if (options_.log_matches) o.match_line = MatchLine(p, pose, results[i].score);
    }
    return outcomes;
  }

  // ComputeConstraint's log_matches line (:260-276); `pose` is the refined
  // pose_estimate (map <- node), p.initial the search start.
  static std::string MatchLine(const Pending& p, const Rigid2d& pose, float score) {
    char buf[160];
    std::string info = "Node (" + std::to_string(p.node_id.trajectory_id) + ", " +
                       std::to_string(p.node_id.node_index) + ") with " +
                       std::to_string(p.cloud->size()) + " points on submap (" +
                       std::to_string(p.submap_id.trajectory_id) + ", " +
                       std::to_string(p.submap_id.submap_index) + ")";
    if (p.full) {
      info += " matches";
    } else {
      const Rigid2d d = Compose(Inverse(p.initial), pose);
      double a = d.theta;  // common::NormalizeAngleDifference
      while (a > M_PI) a -= 2. * M_PI;
      while (a < -M_PI) a += 2. * M_PI;
      std::snprintf(buf, sizeof(buf), " differs by translation %.2f rotation %.3f",
                    std::hypot(d.x, d.y), std::abs(a));
      info += buf;
    }
    std::snprintf(buf, sizeof(buf), " with score %.1f%%.", 100. * score);
    return info + buf;
  }

  struct CachedScan {
    const PointCloud* cloud = nullptr;
    size_t size = 0;
    uint64_t hash = 0;
    int32_t index = kUnset;
  };
  static constexpr int32_t kUnset = INT32_MIN;
  csm_scan_set* scans_ = nullptr;         // node clouds resident across flushes
  std::map<NodeId, CachedScan> scan_cache_;
  int64_t cached_points_ = 0;
};

}  // namespace cartographer_amd

#endif  // CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_2D_H_
