// ConstraintBuilder3D drop-in over the batched 3D C-ABI.
//
// Mirrors mapping/internal/constraints/constraint_builder_3d.{h,cc}: the
// public methods; MaybeAddConstraint's distance filter on the global
// translations and its per-submap FixedRatioSampler (:79-114);
// MaybeAddGlobalConstraint with the poses reduced to their rotations
// (:116-142); NotifyEndOfNode (:144-156); WhenDone (:158-168) with results in
// submission order and failed searches dropped (RunWhenDoneCallback
// :307-333); GetNumFinishedNodes (:335-338); DeleteScanMatcher (:340-349); the
// per-submap matcher cache (DispatchScanMatcherConstruction :170-198, which
// reads the submap's high/low-resolution grids and rotational histogram); and
// the metrics (:46-59, counters and score lists). Pending pairs are searched
// as one GPU batch when a node ends (or once `flush_pairs` are pending)
// instead of one Task per pair. Accepted matches are then refined as one
// batch by the CeresScanMatcher3D restatement (:264-275;
// csm_ceres3d_refine_batch, parity with Ceres unpinned) unless
// options.refine_with_ceres is off.
//
// Lifetimes as ConstraintBuilder2D: a Submap3DView and a node's data must stay
// valid until the flush that searches the pair (matchers may be built, or
// rebuilt after the budgeted cache dropped them, at that flush).
//
// Multi-GPU (set_communicator), as ConstraintBuilder2D: every rank makes the
// same calls; a rank builds matchers for and searches only the submaps it
// owns (ShardOwner, Sharding::kStatic) or the chunks of each flush it claims
// (Sharding::kClaim) on its own device; WhenDone gathers the accepted
// constraints to rank 0 as ConstraintRecord3D in submission order
// (constraint_gather.h), sums the counters and reduces last_error over the
// ranks. The score lists (constraint_scores, global_constraint_scores,
// rotational_scores, low_resolution_scores) are appended at WhenDone from the
// delivered result, in submission order, so on rank 0 they cover every rank.
//
// All of that but the 3D types, the device batch, the score lists and the log
// texts lives in ConstraintBuilderBase (constraint_builder_base.h).
#ifndef CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_3D_H_
#define CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_3D_H_

#include <cmath>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "constraint_builder_base.h"
#include "scan_matching_3d.h"

namespace cartographer_amd {

// What the builder reads of a Submap3D (submap_3d.h:57-73).
struct Submap3DView {
  HybridGridView high_resolution_hybrid_grid;
  HybridGridView low_resolution_hybrid_grid;
  std::vector<float> rotational_scan_matcher_histogram;
};

// PoseGraphInterface::Constraint (pose_graph_interface.h:36-53).
struct Constraint3D {
  SubmapId submap_id;
  NodeId node_id;
  Rigid3d relative_pose;  // zbar_ij: submap <- node
  double translation_weight = 0., rotation_weight = 0.;
  enum Tag { INTRA_SUBMAP, INTER_SUBMAP } tag = INTER_SUBMAP;
  float score = 0.f, rotational_score = 0.f, low_resolution_score = 0.f;
  bool global = false;  // found by MaybeAddGlobalConstraint (the metrics split)
};

// SubmapScanMatcher (constraint_builder_3d.h:117-123): device grids and the
// matcher built from them.
struct SubmapScanMatcher3D {
  std::unique_ptr<HybridGrid3D> high, low;
  std::unique_ptr<FastCorrelativeScanMatcher3D> matcher;
  int64_t device_bytes() const {
    return high->device_bytes() + low->device_bytes() + matcher->device_bytes();
  }
};

struct ConstraintBuilder3DTraits {
  using Constraint = Constraint3D;
  using Record = ConstraintRecord3D;
  using Matcher = SubmapScanMatcher3D;
  struct Payload {
    const Submap3DView* submap;
    const TrajectoryNodeData3D* data;
    Rigid3d node_pose, submap_pose;
  };
  static constexpr const char* kName = "ConstraintBuilder3D";
  static constexpr const char* kMetricPrefix = "mapping_constraints_constraint_builder_3d";
  static constexpr const char* kScoreKinds[] = {"score", "rotational_score",
                                                "low_resolution_score"};
  static constexpr int kClaimNamespace = 1;
};

class ConstraintBuilder3D
    : public ConstraintBuilderBase<ConstraintBuilder3D, ConstraintBuilder3DTraits> {
 public:
  explicit ConstraintBuilder3D(const ConstraintBuilderOptions& options,
                               csm_context* context = nullptr)
      : ConstraintBuilderBase(options, context) {}

  void MaybeAddConstraint(const SubmapId& submap_id, const Submap3DView* submap,
                          const NodeId& node_id, const TrajectoryNodeData3D* constant_data,
                          const Rigid3d& global_node_pose, const Rigid3d& global_submap_pose) {
    const double dx = global_node_pose.t[0] - global_submap_pose.t[0],
                 dy = global_node_pose.t[1] - global_submap_pose.t[1],
                 dz = global_node_pose.t[2] - global_submap_pose.t[2];
    if (std::sqrt(dx * dx + dy * dy + dz * dz) > options_.max_constraint_distance) return;
    if (!Sample(submap_id)) return;
    Enqueue(submap_id, node_id, false,
            Payload{submap, constant_data, global_node_pose, global_submap_pose});
  }

  void MaybeAddGlobalConstraint(const SubmapId& submap_id, const Submap3DView* submap,
                                const NodeId& node_id, const TrajectoryNodeData3D* constant_data,
                                const Quaterniond& global_node_rotation,
                                const Quaterniond& global_submap_rotation) {
    Enqueue(submap_id, node_id, true,
            Payload{submap, constant_data, Rigid3d::Rotation(global_node_rotation),
                    Rigid3d::Rotation(global_submap_rotation)});
  }

  // The base's WhenDone, and the score lists (constraint_builder_3d.cc:46-59)
  // appended from the delivered result in submission order.
  void WhenDone(const std::function<void(const Result&)>& callback) {
    ConstraintBuilderBase::WhenDone([&](const Result& result) {
      for (const Constraint3D& c : result) {
        (c.global ? global_constraint_scores : constraint_scores).push_back(c.score);
        rotational_scores.push_back(c.rotational_score);
        low_resolution_scores.push_back(c.low_resolution_score);
      }
      callback(result);
    });
  }

  // rotational_score_histogram_, low_resolution_score_histogram_ (:257-259).
  const ScoreHistogram& rotational_score_histogram() const { return score_histograms_[1]; }
  const ScoreHistogram& low_resolution_score_histogram() const { return score_histograms_[2]; }

  std::vector<float> constraint_scores, global_constraint_scores;
  std::vector<float> rotational_scores, low_resolution_scores;

 private:
  friend class ConstraintBuilderBase<ConstraintBuilder3D, ConstraintBuilder3DTraits>;
  using SubmapScanMatcher = SubmapScanMatcher3D;

  // DispatchScanMatcherConstruction (constraint_builder_3d.cc:170-198).
  std::shared_ptr<SubmapScanMatcher> MakeMatcher(const Payload& p) {
    auto m = std::make_shared<SubmapScanMatcher>();
    m->high.reset(new HybridGrid3D(p.submap->high_resolution_hybrid_grid, context_));
    m->low.reset(new HybridGrid3D(p.submap->low_resolution_hybrid_grid, context_));
    m->matcher.reset(new FastCorrelativeScanMatcher3D(
        *m->high, m->low.get(), &p.submap->rotational_scan_matcher_histogram,
        options_.fast_correlative_scan_matcher_options_3d, context_));
    return m;
  }

  static ConstraintRecord3D ToRecord(const Constraint3D& c) {
    ConstraintRecord3D r{};
    r.submap_trajectory = c.submap_id.trajectory_id;
    r.submap_index = c.submap_id.submap_index;
    r.node_trajectory = c.node_id.trajectory_id;
    r.node_index = c.node_id.node_index;
    for (int a = 0; a < 3; ++a) r.t[a] = c.relative_pose.t[a];
    const Quaterniond& q = c.relative_pose.rotation;
    r.q[0] = q.w;
    r.q[1] = q.x;
    r.q[2] = q.y;
    r.q[3] = q.z;
    r.score = c.score;
    r.rotational_score = c.rotational_score;
    r.low_resolution_score = c.low_resolution_score;
    r.tag = static_cast<int32_t>(c.tag);
    r.global = c.global ? 1 : 0;
    return r;
  }
  static Constraint3D FromRecord(const ConstraintRecord3D& r) {
    Constraint3D c;
    c.submap_id = SubmapId{r.submap_trajectory, r.submap_index};
    c.node_id = NodeId{r.node_trajectory, r.node_index};
    for (int a = 0; a < 3; ++a) c.relative_pose.t[a] = r.t[a];
    c.relative_pose.rotation = Quaterniond{r.q[0], r.q[1], r.q[2], r.q[3]};
    c.tag = static_cast<Constraint3D::Tag>(r.tag);
    c.score = r.score;
    c.rotational_score = r.rotational_score;
    c.low_resolution_score = r.low_resolution_score;
    c.global = r.global != 0;
    return c;
  }

  void LogWhenDone(size_t computations, size_t constraints) {  // RunWhenDoneCallback (:317-326)
    log_(std::to_string(computations) + " computations resulted in " +
         std::to_string(constraints) + " additional constraints.\nScore histogram:\n" +
         score_histograms_[0].ToString(10) + "\nRotational score histogram:\n" +
         score_histograms_[1].ToString(10) + "\nLow resolution score histogram:\n" +
         score_histograms_[2].ToString(10));
  }

  // Searches (and refines) pending_[which] as one batch over `held`'s matchers.
  std::vector<Outcome> RunBatch(const std::vector<size_t>& which_pending, const Held& held) {
    std::vector<csm_fast3d*> handles;
    std::vector<const SubmapScanMatcher*> keep;
    std::map<SubmapId, int> slot_of;
    std::map<const TrajectoryNodeData3D*, int32_t> node_of;  // a node's data uploads once
    std::vector<csm_node3d> nodes;
    std::vector<csm_pair3d> pairs;
    for (size_t i : which_pending) {
      const Pending& p = pending_[i];
      auto s = slot_of.find(p.submap_id);
      if (s == slot_of.end()) {
        s = slot_of.emplace(p.submap_id, static_cast<int>(handles.size())).first;
        const SubmapScanMatcher* m = held.at(p.submap_id).get();
        handles.push_back(m->matcher->handle());
        keep.push_back(m);
      }
      auto n = node_of.find(p.data);
      if (n == node_of.end()) {
        n = node_of.emplace(p.data, static_cast<int32_t>(nodes.size())).first;
        nodes.push_back(p.data->ToC());
      }
      csm_pair3d q{};
      q.submap = s->second;
      q.node = n->second;
      q.full_submap = p.full ? 1 : 0;
      q.min_score = p.full ? options_.global_localization_min_score : options_.min_score;
      q.node_pose = p.node_pose.ToC();
      q.submap_pose = p.submap_pose.ToC();
      pairs.push_back(q);
    }
    std::vector<csm_result3d> results(pairs.size());
    CheckOk(csm_fast3d_match_batch(context_, handles.data(), static_cast<int32_t>(handles.size()),
                                   nodes.data(), static_cast<int32_t>(nodes.size()), pairs.data(),
                                   static_cast<int64_t>(pairs.size()), results.data()),
            "csm_fast3d_match_batch");
    if (options_.refine_with_ceres) {
      // ceres_scan_matcher_.Match(pose.translation(), pose, {high, low}) (:264-275).
      std::vector<const csm_hybrid_grid*> grids;
      for (const auto& m : keep) {
        grids.push_back(m->high->handle());
        grids.push_back(m->low->handle());
      }
      std::vector<csm_refine3d> items;
      std::vector<size_t> which;
      for (size_t i = 0; i < pairs.size(); ++i)
        if (results[i].status == CSM_OK) {
          csm_refine3d it{};
          it.high_grid = 2 * pairs[i].submap;
          it.low_grid = 2 * pairs[i].submap + 1;
          it.node = pairs[i].node;
          it.initial = results[i].pose;
          for (int a = 0; a < 3; ++a) it.target[a] = results[i].pose.t[a];
          items.push_back(it);
          which.push_back(i);
        }
      std::vector<csm_pose3d> out(items.size());
      if (!items.empty())
        CheckOk(csm_ceres3d_refine_batch(context_, grids.data(), static_cast<int32_t>(grids.size()),
                                         nodes.data(), static_cast<int32_t>(nodes.size()),
                                         items.data(), static_cast<int64_t>(items.size()),
                                         &options_.ceres_scan_matcher_options_3d, out.data(),
                                         nullptr),
                "csm_ceres3d_refine_batch");
      for (size_t k = 0; k < which.size(); ++k) results[which[k]].pose = out[k];
    }
    std::vector<Outcome> outcomes(results.size());
    for (size_t i = 0; i < results.size(); ++i) {
      const Pending& p = pending_[which_pending[i]];
      Outcome& o = outcomes[i];
      o.status = results[i].status;
      if (o.status != CSM_OK) continue;
      o.scores[0] = results[i].score;
      o.scores[1] = results[i].rotational_score;
      o.scores[2] = results[i].low_resolution_score;
      Constraint3D& c = o.constraint;
      c.submap_id = p.submap_id;
      c.node_id = p.node_id;
      c.relative_pose = Rigid3d::FromC(results[i].pose);
      c.translation_weight = options_.loop_closure_translation_weight;
      c.rotation_weight = options_.loop_closure_rotation_weight;
      c.tag = Constraint3D::INTER_SUBMAP;
      c.score = results[i].score;
      c.rotational_score = results[i].rotational_score;
      c.low_resolution_score = results[i].low_resolution_score;
      c.global = p.full;
      if (options_.log_matches) o.match_line = MatchLine(p, c.relative_pose, results[i].score);
    }
    return outcomes;
  }

  // ComputeConstraint's log_matches line (:284-303). difference =
  // global_node_pose^-1 * global_submap_pose * constraint_transform; its
  // angle is transform::GetAngle (2 atan2(|vec|, |w|)).
  static std::string MatchLine(const Pending& p, const Rigid3d& constraint, float score) {
    char buf[160];
    std::string info = "Node (" + std::to_string(p.node_id.trajectory_id) + ", " +
                       std::to_string(p.node_id.node_index) + ") with " +
                       std::to_string(p.data->high_resolution_point_cloud.size()) +
                       " points on submap (" + std::to_string(p.submap_id.trajectory_id) + ", " +
                       std::to_string(p.submap_id.submap_index) + ")";
    if (p.full) {
      info += " matches";
    } else {
      const Rigid3d d = Mul(Mul(Inv(p.node_pose), p.submap_pose), constraint);
      const Quaterniond& q = d.rotation;
      const double angle = 2. * std::atan2(std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z),
                                           std::abs(q.w));
      std::snprintf(buf, sizeof(buf), " differs by translation %.2f rotation %.3f",
                    std::sqrt(d.t[0] * d.t[0] + d.t[1] * d.t[1] + d.t[2] * d.t[2]), angle);
      info += buf;
    }
    std::snprintf(buf, sizeof(buf), " with score %.1f%%.", 100. * score);
    return info + buf;
  }
  // transform::Rigid3d operator* and inverse (rigid_transform.h:163-200) in double.
  static Quaterniond QMul(const Quaterniond& a, const Quaterniond& b) {
    return Quaterniond{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
                       a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                       a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                       a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
  }
  static void QRot(const Quaterniond& q, const double v[3], double out[3]) {
    const Quaterniond p{0., v[0], v[1], v[2]};
    const Quaterniond r = QMul(QMul(q, p), Quaterniond{q.w, -q.x, -q.y, -q.z});
    const double n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    out[0] = r.x / n;
    out[1] = r.y / n;
    out[2] = r.z / n;
  }
  static Rigid3d Mul(const Rigid3d& a, const Rigid3d& b) {
    Rigid3d r;
    QRot(a.rotation, b.t, r.t);
    for (int k = 0; k < 3; ++k) r.t[k] += a.t[k];
    r.rotation = QMul(a.rotation, b.rotation);
    return r;
  }
  static Rigid3d Inv(const Rigid3d& a) {
    const Quaterniond& q = a.rotation;
    const double n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
    Rigid3d r;
    r.rotation = Quaterniond{q.w / n, -q.x / n, -q.y / n, -q.z / n};
    QRot(r.rotation, a.t, r.t);
    for (int k = 0; k < 3; ++k) r.t[k] = -r.t[k];
    return r;
  }
};

}  // namespace cartographer_amd

#endif  // CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_3D_H_
