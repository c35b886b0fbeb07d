// The host skeleton of the ConstraintBuilder2D / 3D drop-ins: everything the
// two do alike, once. That is the submission slots and their order, the
// per-submap samplers and the budgeted matcher cache, flushing (when a node
// ends, or once `flush_pairs` are pending), the cut of a flush into claim
// chunks (Sharding::kClaim) and into sub-batches whose matchers fit the cache
// budget, the walk over a searched batch (counters, metrics, histograms,
// storing, logging, the "pairs skipped" line), DeleteScanMatcher, and WhenDone
// with the gather to rank 0 (constraint_gather.h).
//
// ConstraintBuilderBase<Derived, Traits> is a CRTP base without virtual
// functions, so Metrics() is one static per dimension, as the reference's
// k*Metric statics are. Traits names
//   Constraint, Record   the delivered constraint and its wire record
//   Matcher              what the cache holds per submap (has device_bytes())
//   Payload              what a pending pair carries besides ids, `full`, slot
//   kName                the class name in stderr and default-log messages
//   kMetricPrefix        the metric families' common prefix
//   kScoreKinds          the `kind` label of every score of a match ({nullptr}:
//                        one score, labelled with its search_region alone)
//   kClaimNamespace      set_communicator's default claim_namespace
// and Derived provides (private, with the base as a friend)
//   std::shared_ptr<Matcher> MakeMatcher(const Payload&)
//   std::vector<Outcome> RunBatch(const std::vector<size_t>& which_pending, const Held&)
//       searches and refines pending_[which_pending] as one device batch
//   Record ToRecord(const Constraint&), Constraint FromRecord(const Record&)
//       the fields but `slot` and the weights, which the base fills in
//   void LogWhenDone(size_t computations, size_t constraints)
#ifndef CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_BASE_H_
#define CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_BASE_H_

#include <algorithm>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "constraint_builder_common.h"
#include "constraint_gather.h"
#include "metrics.h"

namespace cartographer_amd {

template <typename Derived, typename Traits>
class ConstraintBuilderBase {
 public:
  using Constraint = typename Traits::Constraint;
  using Result = std::vector<Constraint>;
  static constexpr int kNumScores =
      static_cast<int>(sizeof(Traits::kScoreKinds) / sizeof(Traits::kScoreKinds[0]));

  // Shards the search over the ranks of `comm` (not owned; outlives the
  // builder). Call before the first MaybeAdd*. kClaim needs
  // csm_comm_claim_open on `comm`; builders that share a communicator in
  // kClaim mode need distinct `claim_namespace`s (their counters' keys).
  void set_communicator(csm_comm* comm, Sharding sharding = Sharding::kStatic,
                        int chunk_submaps = 4, int claim_namespace = Traits::kClaimNamespace) {
    comm_ = comm;
    sharding_ = sharding;
    chunk_submaps_ = chunk_submaps;
    claim_key_ = static_cast<int64_t>(claim_namespace) << 40;
  }

  void NotifyEndOfNode() {
    ++num_started_nodes_;
    if (static_cast<int>(pending_.size()) >= options_.flush_pairs) Flush();
  }

  void WhenDone(const std::function<void(const Result&)>& callback) {
    Flush();
    Result result;
    if (comm_ && csm_comm_size(comm_) > 1) {
      GatherToRoot(&result);
    } else {
      for (auto& c : constraints_)
        if (c) result.push_back(*c);
    }
    if (options_.log_matches) derived().LogWhenDone(constraints_.size(), result.size());
    constraints_.clear();
    Metrics().queue_length->Set(constraints_.size());
    callback(result);
  }

  int GetNumFinishedNodes() const { return num_finished_nodes_; }

  // Also drops the submap's pairs still pending (they yield no constraint):
  // the reference's tasks would read the deleted matcher, and a pending pair
  // must not make the builder rebuild it from a submap the caller is trimming.
  void DeleteScanMatcher(const SubmapId& submap_id) {
    matchers_.Erase(submap_id);
    samplers_.erase(submap_id);
    Metrics().num_submap_scan_matchers->Set(matchers_.size());
    const size_t before = pending_.size();
    pending_.erase(std::remove_if(pending_.begin(), pending_.end(),
                                  [&](const Pending& p) {
                                    return !(p.submap_id < submap_id) &&
                                           !(submap_id < p.submap_id);
                                  }),
                   pending_.end());
    if (pending_.size() != before)
      std::fprintf(stderr,
                   "%s: DeleteScanMatcher dropped %zu pending pairs of a deleted submap\n",
                   Traits::kName, before - pending_.size());
  }

  // kNumSubmapScanMatchersMetric, and the cache's device bytes and churn.
  int num_submap_scan_matchers() const { return static_cast<int>(matchers_.size()); }
  int64_t matcher_cache_bytes() const { return matchers_.bytes(); }
  int64_t matcher_builds() const { return matchers_.builds; }
  int64_t matcher_evictions() const { return matchers_.evictions; }

  // The reference's metric families (constraint_builder_2d.cc:318-343,
  // _3d.cc:351-386): the same names and labels. Until called, the metrics are
  // Null ones. Shared by every builder of one dimension in the process, as
  // the reference's statics.
  static void RegisterMetrics(metrics::FamilyFactory* factory) {
    MetricSet& m = Metrics();
    const std::string prefix = Traits::kMetricPrefix;
    auto* counts = factory->NewCounterFamily(prefix + "_constraints", "Constraints computed");
    m.searched[0] = counts->Add({{"search_region", "local"}, {"matcher", "searched"}});
    m.found[0] = counts->Add({{"search_region", "local"}, {"matcher", "found"}});
    m.searched[1] = counts->Add({{"search_region", "global"}, {"matcher", "searched"}});
    m.found[1] = counts->Add({{"search_region", "global"}, {"matcher", "found"}});
    m.queue_length = factory->NewGaugeFamily(prefix + "_queue_length", "Queue length")->Add({});
    auto* scores = factory->NewHistogramFamily(prefix + "_scores", "Constraint scores built",
                                               metrics::Histogram::FixedWidth(0.05, 20));
    for (int g = 0; g < 2; ++g)
      for (int k = 0; k < kNumScores; ++k) {
        metrics::Labels labels{{"search_region", g ? "global" : "local"}};
        if (Traits::kScoreKinds[k]) labels["kind"] = Traits::kScoreKinds[k];
        m.scores[g][k] = scores->Add(labels);
      }
    m.num_submap_scan_matchers =
        factory->NewGaugeFamily(prefix + "_num_submap_scan_matchers",
                                "Current number of constructed submap scan matchers")->Add({});
  }

  // score_histogram_: every accepted match's score, over the builder's life.
  const ScoreHistogram& score_histogram() const { return score_histograms_[0]; }
  // Where the log_matches lines go (LOG(INFO) in the reference).
  void set_log_sink(LogSink sink) { log_ = std::move(sink); }

  // Counters of this builder (the metric counters above are process-wide).
  int64_t constraints_searched = 0, constraints_found = 0;
  int64_t global_constraints_searched = 0, global_constraints_found = 0;
  // Pairs skipped because the device search returned an error (not counted
  // as searched), and the last such status.
  int64_t constraints_failed = 0;
  // Sharding::kClaim: chunks this rank searched (not summed over ranks).
  int64_t chunks_claimed = 0;
  int last_error = CSM_OK;

 protected:
  using Matcher = typename Traits::Matcher;
  using Payload = typename Traits::Payload;
  using Record = typename Traits::Record;
  using Held = std::map<SubmapId, std::shared_ptr<Matcher>>;

  struct Pending : Payload {
    SubmapId submap_id;
    NodeId node_id;
    bool full;
    size_t slot;
  };

  // What RunBatch hands back per pair. `status` < 0: the device path could
  // not search it; CSM_OK: a match, with its scores, its constraint and (if
  // options.log_matches) ComputeConstraint's log line; else no match.
  struct Outcome {
    int status = CSM_OK;
    float scores[kNumScores] = {};
    Constraint constraint;
    std::string match_line;
  };

  ConstraintBuilderBase(const ConstraintBuilderOptions& options, csm_context* context)
      : options_(options),
        context_(context ? context : ThreadContext()),
        matchers_(options.matcher_cache_bytes) {}

  // MaybeAddConstraint's per-submap FixedRatioSampler.
  bool Sample(const SubmapId& submap_id) {
    auto it = samplers_.emplace(submap_id, FixedRatioSampler(options_.sampling_ratio)).first;
    return it->second.Pulse();
  }

  void Enqueue(const SubmapId& submap_id, const NodeId& node_id, bool full,
               const Payload& payload) {
    constraints_.emplace_back();
    Metrics().queue_length->Set(constraints_.size());
    if (!Owned(submap_id)) return;  // another rank searches it; the slot keeps submission order
    if (!Claiming()) EnsureMatcher(submap_id, payload);  // claimed chunks build theirs
    pending_.push_back(Pending{payload, submap_id, node_id, full, constraints_.size() - 1});
  }

  bool Claiming() const {
    return comm_ && csm_comm_size(comm_) > 1 && sharding_ == Sharding::kClaim;
  }
  bool Owned(const SubmapId& id) const {
    return !comm_ || csm_comm_size(comm_) <= 1 || sharding_ == Sharding::kClaim ||
           ShardOwner(id.trajectory_id, id.submap_index, csm_comm_size(comm_)) ==
               csm_comm_rank(comm_);
  }

  ConstraintBuilderOptions options_;
  csm_context* context_;
  ScoreHistogram score_histograms_[kNumScores];
  LogSink log_ = DefaultLogSink(Traits::kName);
  std::vector<Pending> pending_;

 private:
  Derived& derived() { return *static_cast<Derived*>(this); }

  // DispatchScanMatcherConstruction, through the budgeted cache (a dropped
  // matcher is rebuilt from the submap on its next use).
  std::shared_ptr<Matcher> EnsureMatcher(const SubmapId& submap_id, const Payload& payload) {
    auto m = matchers_.Get(
        submap_id, [&] { return derived().MakeMatcher(payload); },
        [](const Matcher& m) { return m.device_bytes(); });
    Metrics().num_submap_scan_matchers->Set(matchers_.size());
    return m;
  }

  // Rank 0 receives every rank's accepted constraints in slot order; the
  // counter deltas since the last WhenDone are summed over the ranks.
  void GatherToRoot(Result* result) {
    CheckSameSubmissions(comm_, static_cast<int64_t>(constraints_.size()));
    last_error = ReduceLastError(comm_, last_error);
    std::vector<Record> local;
    for (size_t slot = 0; slot < constraints_.size(); ++slot) {
      if (!constraints_[slot]) continue;
      local.push_back(derived().ToRecord(*constraints_[slot]));
      local.back().slot = static_cast<int64_t>(slot);
    }
    const std::vector<Record> all = GatherRecords(comm_, local);
    int64_t* counters[5] = {&constraints_searched, &constraints_found, &global_constraints_searched,
                            &global_constraints_found, &constraints_failed};
    int64_t d[5];
    for (int k = 0; k < 5; ++k) d[k] = *counters[k] - reduced_[k];
    CommCheck(csm_comm_allreduce_i64(comm_, d, 5, CSM_REDUCE_SUM), "csm_comm_allreduce_i64");
    for (int k = 0; k < 5; ++k) {
      reduced_[k] += d[k];
      *counters[k] = reduced_[k];
    }
    for (const Record& r : all) {
      result->push_back(derived().FromRecord(r));
      result->back().translation_weight = options_.loop_closure_translation_weight;
      result->back().rotation_weight = options_.loop_closure_rotation_weight;
    }
  }

  void Flush() {
    if (pending_.empty()) {
      num_finished_nodes_ = num_started_nodes_;
      return;
    }
    if (Claiming()) {
      const std::vector<std::vector<size_t>> chunks = ClaimChunks(pending_, chunk_submaps_);
      ForClaimedChunks(comm_, claim_key_++, chunks.size(), [&](size_t c) {
        ++chunks_claimed;
        Search(chunks[c]);
      });
    } else {
      std::vector<size_t> all(pending_.size());
      for (size_t i = 0; i < all.size(); ++i) all[i] = i;
      Search(all);
    }
    pending_.clear();
    num_finished_nodes_ = num_started_nodes_;
  }

  // Cuts pending_[which] into sub-batches whose matchers fit the matcher
  // cache's budget together (one batch when unbounded or when they fit),
  // whole submaps per sub-batch, and searches each.
  void Search(const std::vector<size_t>& which_pending) {
    std::vector<size_t> order(which_pending);
    if (matchers_.bounded())
      std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        return pending_[a].submap_id < pending_[b].submap_id;
      });
    std::vector<size_t> part;
    Held held;
    int64_t held_bytes = 0;
    for (size_t i : order) {
      const Pending& p = pending_[i];
      if (!held.count(p.submap_id)) {
        auto m = EnsureMatcher(p.submap_id, p);
        const int64_t b = m->device_bytes();
        if (!part.empty() && matchers_.bounded() && held_bytes + b > matchers_.budget()) {
          SearchBatch(part, held);
          part.clear();
          held.clear();
          held_bytes = 0;
          matchers_.Trim();  // the searched part's matchers are no longer held
        }
        held.emplace(p.submap_id, std::move(m));
        held_bytes += b;
      }
      part.push_back(i);
    }
    if (!part.empty()) SearchBatch(part, held);
    held.clear();
    matchers_.Trim();
  }

  // One device batch over `held`'s matchers, then the walk over its outcomes.
  void SearchBatch(const std::vector<size_t>& which_pending, const Held& held) {
    const std::vector<Outcome> outcomes = derived().RunBatch(which_pending, held);
    MetricSet& m = Metrics();
    int64_t failed_this_flush = 0;
    for (size_t i = 0; i < which_pending.size(); ++i) {
      const Pending& p = pending_[which_pending[i]];
      const Outcome& o = outcomes[i];
      if (o.status < 0) {
        // A pair the device path could not search (CSM_ERANGE: a cloud or
        // window past the kernels' limits) yields no
        // constraint; it is counted and reported, never fatal.
        ++constraints_failed;
        ++failed_this_flush;
        last_error = o.status;
        continue;
      }
      (p.full ? global_constraints_searched : constraints_searched) += 1;
      m.searched[p.full]->Increment();
      if (o.status != CSM_OK) continue;
      (p.full ? global_constraints_found : constraints_found) += 1;
      m.found[p.full]->Increment();
      for (int k = 0; k < kNumScores; ++k) {
        m.scores[p.full][k]->Observe(o.scores[k]);
        score_histograms_[k].Add(o.scores[k]);
      }
      constraints_[p.slot].reset(new Constraint(o.constraint));
      if (options_.log_matches) log_(o.match_line);
    }
    if (failed_this_flush)
      std::fprintf(stderr, "%s: %lld of %zu pairs skipped (%s)\n", Traits::kName,
                   static_cast<long long>(failed_this_flush), which_pending.size(),
                   csm_strerror(last_error));
  }

  // The process-wide metrics (the reference's static k*Metric pointers);
  // [local, global], the histograms also by score kind.
  struct MetricSet {
    metrics::Counter* searched[2] = {metrics::Counter::Null(), metrics::Counter::Null()};
    metrics::Counter* found[2] = {metrics::Counter::Null(), metrics::Counter::Null()};
    metrics::Gauge* queue_length = metrics::Gauge::Null();
    metrics::Histogram* scores[2][kNumScores];
    metrics::Gauge* num_submap_scan_matchers = metrics::Gauge::Null();
    MetricSet() {
      for (auto& region : scores)
        for (auto& h : region) h = metrics::Histogram::Null();
    }
  };
  static MetricSet& Metrics() {
    static MetricSet m;
    return m;
  }

  MatcherCache<Matcher> matchers_;
  std::map<SubmapId, FixedRatioSampler> samplers_;
  std::vector<std::unique_ptr<Constraint>> constraints_;
  int num_started_nodes_ = 0, num_finished_nodes_ = 0;
  csm_comm* comm_ = nullptr;
  Sharding sharding_ = Sharding::kStatic;
  int chunk_submaps_ = 4;
  int64_t claim_key_ = 0;                  // kClaim: the next flush's counter
  int64_t reduced_[5] = {0, 0, 0, 0, 0};  // counter totals over ranks at the last WhenDone
};

}  // namespace cartographer_amd

#endif  // CARTOGRAPHER_AMD_CONSTRAINT_BUILDER_BASE_H_
