// The constraint builders' shared host skeleton (ConstraintBuilderBase,
// include/cartographer_amd/constraint_builder_base.h) driven by a stub
// dimension that never touches a device: its matcher is a byte size, its
// search records the pairs it was given and returns the statuses the test
// scripted. tests/test_constraint_builder_skeleton.py builds and runs this on
// the CPU, checks the stderr lines, and drives the same scripts through a stub
// subclass of the Python base.
//
// Usage: constraint_builder_skeleton_test <case>; exits 0 when every check of
// the case holds and prints the failing checks otherwise.
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "cartographer_amd/constraint_builder_base.h"

using namespace cartographer_amd;

static int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: EXPECT(%s)\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

struct StubMatcher {
  int64_t bytes;
  int64_t device_bytes() const { return bytes; }
};
struct StubConstraint {
  SubmapId submap_id;
  NodeId node_id;
  double translation_weight = 0., rotation_weight = 0.;
  int id = -1;
};
struct StubRecord {
  int64_t slot;
  int32_t id;
};
struct StubTraits {
  using Constraint = StubConstraint;
  using Record = StubRecord;
  using Matcher = StubMatcher;
  struct Payload {
    int id;      // the test's name for the pair
    int status;  // what the "device" answers for it
    int64_t matcher_bytes;
  };
  static constexpr const char* kName = "StubBuilder";
  static constexpr const char* kMetricPrefix = "stub";
  static constexpr const char* kScoreKinds[] = {nullptr};
  static constexpr int kClaimNamespace = 2;
};

class StubBuilder : public ConstraintBuilderBase<StubBuilder, StubTraits> {
 public:
  // A placeholder context: nothing here ever uses one.
  explicit StubBuilder(const ConstraintBuilderOptions& options)
      : ConstraintBuilderBase(options, reinterpret_cast<csm_context*>(uintptr_t{1})) {
    set_log_sink([this](const std::string& line) { log.push_back(line); });
  }

  void Add(int id, int submap, int node, bool full, int status = CSM_OK, int64_t bytes = 10) {
    const SubmapId submap_id{0, submap};
    if (!full && !Sample(submap_id)) return;
    Enqueue(submap_id, NodeId{0, node}, full, Payload{id, status, bytes});
  }

  struct Batch {
    std::vector<int> ids, submaps;  // per pair, in the order given
    int64_t held_bytes = 0;
    size_t held_submaps = 0;
  };
  std::vector<Batch> batches;
  std::vector<std::string> log;
  using ConstraintBuilderBase::Claiming;
  using ConstraintBuilderBase::Owned;

 private:
  friend class ConstraintBuilderBase<StubBuilder, StubTraits>;

  std::shared_ptr<StubMatcher> MakeMatcher(const Payload& p) {
    return std::make_shared<StubMatcher>(StubMatcher{p.matcher_bytes});
  }
  std::vector<Outcome> RunBatch(const std::vector<size_t>& which_pending, const Held& held) {
    Batch b;
    for (const auto& h : held) b.held_bytes += h.second->device_bytes();
    b.held_submaps = held.size();
    std::vector<Outcome> outcomes;
    for (size_t i : which_pending) {
      const Pending& p = pending_[i];
      EXPECT(held.count(p.submap_id) == 1);
      b.ids.push_back(p.id);
      b.submaps.push_back(p.submap_id.submap_index);
      Outcome o;
      o.status = p.status;
      o.scores[0] = 0.5f;
      o.constraint.submap_id = p.submap_id;
      o.constraint.node_id = p.node_id;
      o.constraint.id = p.id;
      o.match_line = "match " + std::to_string(p.id);
      outcomes.push_back(o);
    }
    batches.push_back(b);
    return outcomes;
  }
  static StubRecord ToRecord(const StubConstraint& c) { return StubRecord{0, c.id}; }
  static StubConstraint FromRecord(const StubRecord& r) {
    StubConstraint c;
    c.id = r.id;
    return c;
  }
  void LogWhenDone(size_t computations, size_t constraints) {
    log_("done " + std::to_string(computations) + " " + std::to_string(constraints));
  }
};

using Ids = std::vector<int>;

static ConstraintBuilderOptions Options(int flush_pairs, double sampling_ratio = 1.,
                                        int64_t matcher_cache_bytes = 0) {
  ConstraintBuilderOptions o;
  o.flush_pairs = flush_pairs;
  o.sampling_ratio = sampling_ratio;
  o.matcher_cache_bytes = matcher_cache_bytes;  // 0: one batch per flush, submission order
  return o;
}

static Ids Done(StubBuilder* b) {
  Ids ids;
  int calls = 0;
  b->WhenDone([&](const StubBuilder::Result& r) {
    ++calls;
    for (const StubConstraint& c : r) ids.push_back(c.id);
  });
  EXPECT(calls == 1);
  return ids;
}

// flush_pairs = 0: every NotifyEndOfNode searches exactly that node's pairs.
static void FlushEveryNode() {
  StubBuilder b(Options(0));
  EXPECT(b.GetNumFinishedNodes() == 0);
  for (int node = 0; node < 3; ++node) {
    b.Add(2 * node, 0, node, false);
    b.Add(2 * node + 1, 1, node, true);
    EXPECT(b.batches.size() == static_cast<size_t>(node));
    b.NotifyEndOfNode();
    EXPECT(b.batches.size() == static_cast<size_t>(node) + 1);
    EXPECT((b.batches.back().ids == Ids{2 * node, 2 * node + 1}));
    EXPECT(b.GetNumFinishedNodes() == node + 1);
  }
  b.NotifyEndOfNode();  // a node without pairs finishes at once
  EXPECT(b.batches.size() == 3 && b.GetNumFinishedNodes() == 4);
  EXPECT((Done(&b) == Ids{0, 1, 2, 3, 4, 5}));
  EXPECT(b.batches.size() == 3);
}

// flush_pairs = 5, two pairs per node: nothing is searched until five are
// pending, GetNumFinishedNodes lags until then, WhenDone searches the rest.
static void FlushAtFive() {
  StubBuilder b(Options(5));
  const int finished_after[4] = {0, 0, 3, 3};
  for (int node = 0; node < 4; ++node) {
    b.Add(2 * node, 0, node, false);
    b.Add(2 * node + 1, 1, node, true);
    b.NotifyEndOfNode();
    EXPECT(b.GetNumFinishedNodes() == finished_after[node]);
    EXPECT(b.batches.size() == (node < 2 ? 0u : 1u));
  }
  EXPECT((b.batches[0].ids == Ids{0, 1, 2, 3, 4, 5}));
  EXPECT((Done(&b) == Ids{0, 1, 2, 3, 4, 5, 6, 7}));
  EXPECT(b.batches.size() == 2 && (b.batches[1].ids == Ids{6, 7}));
  EXPECT(b.GetNumFinishedNodes() == 4);
}

// Statuses mixed over local and global pairs, three nodes, one batch each:
//   node 0: 0 local OK, 1 global NO_MATCH, 2 global ERANGE, 3 local OK
//   node 1: 4 local NO_MATCH, 5 global OK, 6 local ERANGE, 7 local ERANGE
//   node 2: 8 global OK, 9 local OK
// local: searched 0 3 4 9, found 0 3 9; global: searched 1 5 8, found 5 8;
// failed 2 6 7. stderr (checked by the Python test): "1 of 4" and "2 of 4".
static void OrderAndCounters() {
  StubBuilder b(Options(0));
  metrics::InMemoryFamilyFactory factory;
  StubBuilder::RegisterMetrics(&factory);
  b.Add(0, 0, 0, false, CSM_OK);
  b.Add(1, 1, 0, true, CSM_NO_MATCH);
  b.Add(2, 0, 0, true, CSM_ERANGE);
  b.Add(3, 1, 0, false, CSM_OK);
  b.NotifyEndOfNode();
  EXPECT(b.last_error == CSM_ERANGE && b.constraints_failed == 1);
  b.Add(4, 0, 1, false, CSM_NO_MATCH);
  b.Add(5, 1, 1, true, CSM_OK);
  b.Add(6, 1, 1, false, CSM_ERANGE);
  b.Add(7, 0, 1, false, CSM_ERANGE);
  b.NotifyEndOfNode();
  b.Add(8, 0, 2, true, CSM_OK);
  b.Add(9, 1, 2, false, CSM_OK);
  b.NotifyEndOfNode();
  EXPECT(factory.gauge("stub_queue_length")->value() == 10);
  EXPECT((Done(&b) == Ids{0, 3, 5, 8, 9}));
  EXPECT(b.constraints_searched == 4 && b.constraints_found == 3);
  EXPECT(b.global_constraints_searched == 3 && b.global_constraints_found == 2);
  EXPECT(b.constraints_failed == 3 && b.last_error == CSM_ERANGE);
  EXPECT(b.score_histogram().size() == 5);
  // "computations" counts the slots, not the results.
  EXPECT((b.log == std::vector<std::string>{"match 0", "match 3", "match 5", "match 8", "match 9",
                                            "done 10 5"}));
  auto count = [&](const char* region, const char* what) {
    return factory.counter("stub_constraints", {{"search_region", region}, {"matcher", what}})
        ->value();
  };
  EXPECT(count("local", "searched") == 4 && count("local", "found") == 3);
  EXPECT(count("global", "searched") == 3 && count("global", "found") == 2);
  EXPECT(factory.histogram("stub_scores", {{"search_region", "local"}})->count() == 3);
  EXPECT(factory.histogram("stub_scores", {{"search_region", "global"}})->count() == 2);
  EXPECT(factory.gauge("stub_queue_length")->value() == 0);
  EXPECT(factory.gauge("stub_num_submap_scan_matchers")->value() == 2);
  // The next WhenDone starts from no slots.
  EXPECT(Done(&b).empty() && b.log.back() == "done 0 0");
}

// DeleteScanMatcher between enqueue and flush, sampling_ratio 0.5 (a sampler
// takes its first pulse and drops its second):
//   0 A local (taken), 1 B local (taken), 2 A global, 3 B global, delete A,
//   4 A local (taken only by a fresh sampler), 5 B local (dropped).
static void DeleteBeforeFlush() {
  StubBuilder b(Options(100, 0.5));
  b.Add(0, 0, 0, false);
  b.Add(1, 1, 0, false);
  b.Add(2, 0, 0, true);
  b.Add(3, 1, 0, true);
  b.NotifyEndOfNode();
  EXPECT(b.num_submap_scan_matchers() == 2 && b.matcher_builds() == 2);
  b.DeleteScanMatcher(SubmapId{0, 0});  // stderr: "dropped 2 pending pairs"
  EXPECT(b.num_submap_scan_matchers() == 1 && b.matcher_cache_bytes() == 10);
  b.Add(4, 0, 1, false);
  b.Add(5, 1, 1, false);
  b.NotifyEndOfNode();
  EXPECT(b.num_submap_scan_matchers() == 2 && b.matcher_builds() == 3);
  EXPECT(b.batches.empty() && b.GetNumFinishedNodes() == 0);
  EXPECT((Done(&b) == Ids{1, 3, 4}));
  EXPECT(b.batches.size() == 1 && (b.batches[0].ids == Ids{1, 3, 4}));
  EXPECT(b.log.back() == "done 5 3");  // the dropped pairs' slots still count
  EXPECT(b.constraints_searched == 2 && b.global_constraints_searched == 1);
  EXPECT(b.GetNumFinishedNodes() == 2);
}

// Pair k goes to submap kSubmapOf[k]: five submaps of 10 bytes, interleaved.
static const int kSubmapOf[10] = {3, 0, 4, 1, 3, 2, 0, 4, 1, 2};

// Budget 25. Every enqueue after the second builds a matcher and evicts the
// least recent one (10 builds, 8 evictions, {1, 2} cached). The flush walks
// the submaps in id order; each of the five is rebuilt (15 builds). 0 and 1
// each evict one idle matcher on arrival (10 evictions); 2 finds everything
// held, does not fit beside 0 and 1, so {0, 1} are searched and 0 goes (11);
// 3 evicts 1 (12); 4 does not fit beside 2 and 3, which are searched, and 2
// goes (13); 4 is searched alone. {3, 4} stay cached.
static void Budget() {
  StubBuilder b(Options(100, 1., 25));
  for (int k = 0; k < 10; ++k) b.Add(k, kSubmapOf[k], k / 4, k % 2 == 0);
  EXPECT(b.matcher_builds() == 10 && b.matcher_evictions() == 8);
  EXPECT((Done(&b) == Ids{0, 1, 2, 3, 4, 5, 6, 7, 8, 9}));
  EXPECT(b.batches.size() == 3);
  if (b.batches.size() == 3) {
    EXPECT((b.batches[0].ids == Ids{1, 6, 3, 8}));
    EXPECT((b.batches[1].ids == Ids{5, 9, 0, 4}));
    EXPECT((b.batches[2].ids == Ids{2, 7}));
  }
  std::set<int> seen;
  for (const StubBuilder::Batch& batch : b.batches) {
    EXPECT(batch.held_bytes <= 25 || batch.held_submaps == 1);
    const std::set<int> here(batch.submaps.begin(), batch.submaps.end());
    EXPECT(here.size() == batch.held_submaps);
    for (int s : here) EXPECT(seen.insert(s).second);  // a submap is in one batch, whole
  }
  EXPECT(seen.size() == 5);
  EXPECT(b.matcher_builds() == 15 && b.matcher_evictions() == 13);
  EXPECT(b.num_submap_scan_matchers() == 2 && b.matcher_cache_bytes() == 20);

  // A submap larger than the budget is searched alone.
  StubBuilder big(Options(100, 1., 25));
  big.Add(0, 0, 0, true);
  big.Add(1, 1, 0, true, CSM_OK, 30);
  big.Add(2, 2, 0, true);
  EXPECT((Done(&big) == Ids{0, 1, 2}));
  EXPECT(big.batches.size() == 3 && big.batches[1].held_bytes == 30 &&
         big.batches[1].held_submaps == 1);

  // Budget 0: unbounded, one batch in plain submission order.
  StubBuilder u(Options(100, 1., 0));
  for (int k = 0; k < 10; ++k) u.Add(k, kSubmapOf[k], k / 4, k % 2 == 0);
  EXPECT((Done(&u) == Ids{0, 1, 2, 3, 4, 5, 6, 7, 8, 9}));
  EXPECT(u.batches.size() == 1 && (u.batches[0].ids == Ids{0, 1, 2, 3, 4, 5, 6, 7, 8, 9}));
  EXPECT(u.matcher_builds() == 5 && u.matcher_evictions() == 0);
  EXPECT(u.num_submap_scan_matchers() == 5 && u.matcher_cache_bytes() == 50);
}

// Without a communicator, or in a world of one, a builder owns every submap
// and claims nothing, whatever the sharding mode.
static void ShardingAlone() {
  StubBuilder none(Options(0));
  csm_comm* comm = nullptr;
  EXPECT(csm_comm_create_tcp(0, 1, nullptr, 1, &comm) == CSM_OK);  // a world of 1 opens no socket
  StubBuilder fixed(Options(0)), claim(Options(0));
  fixed.set_communicator(comm, Sharding::kStatic);
  claim.set_communicator(comm, Sharding::kClaim);
  for (StubBuilder* b : {&none, &fixed, &claim}) {
    EXPECT(!b->Claiming());
    for (int s = 0; s < 7; ++s) EXPECT(b->Owned(SubmapId{s % 2, s}));
    for (int k = 0; k < 4; ++k) b->Add(k, k, 0, true);
    EXPECT((Done(b) == Ids{0, 1, 2, 3}));
    EXPECT(b->chunks_claimed == 0 && b->batches.size() == 1);
  }
  csm_comm_destroy(comm);
}

int main(int argc, char** argv) {
  const std::string which = argc == 2 ? argv[1] : "";
  if (which == "flush_every_node") FlushEveryNode();
  else if (which == "flush_at_five") FlushAtFive();
  else if (which == "order_and_counters") OrderAndCounters();
  else if (which == "delete_before_flush") DeleteBeforeFlush();
  else if (which == "budget") Budget();
  else if (which == "sharding_alone") ShardingAlone();
  else {
    std::fprintf(stderr, "usage: %s <case>\n", argv[0]);
    return 2;
  }
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
