// single_coalesce.h's leader/follower protocol with a fake `run` that records
// what it sees, and host_pool.h's worker pool, on the CPU. Built twice by
// tests/test_single_coalesce.py: under AddressSanitizer + UBSan and under
// ThreadSanitizer.
//
// Arrival order is what the coalescer's queue holds, so the test makes it
// observable: a caller takes its arrival number under the test's own lock
// once the previous number's request is in the queue (CoalesceState::arrived
// says so), and only then queues its own.
//
// A watchdog thread ends the program if it has not finished after
// kWatchdogSeconds, naming the case that was running, so a lost wake-up
// fails the test instead of hanging it. Measured run time of the whole
// program on 8 cores: 5 s under ThreadSanitizer, 3 s under ASan + UBSan.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../cartographer-1_amd/csrc/host_pool.h"
#include "../../cartographer-1_amd/csrc/single_coalesce.h"

namespace {

using csm::CoalesceKnobs;
using csm::CoalesceState;

constexpr int kWatchdogSeconds = 120;

std::mutex case_mu;
std::string case_name = "start";
void Case(const std::string& name) {
  std::lock_guard<std::mutex> g(case_mu);
  case_name = name;
}
std::string CaseName() {
  std::lock_guard<std::mutex> g(case_mu);
  return case_name;
}

int failures = 0;  // main thread only
#define CHECK(cond, ...)                                                 \
  do {                                                                   \
    if (!(cond)) {                                                       \
      ++failures;                                                        \
      std::printf("FAIL [%s] %s: ", CaseName().c_str(), #cond);          \
      std::printf(__VA_ARGS__);                                          \
      std::printf("\n");                                                 \
    }                                                                    \
  } while (0)

struct Req : csm::CoalesceReq {
  uint64_t arrival = 0;  // its place in the queue's arrival order
  int batch = -1;        // the run that had it
};
using Coalescer = csm::SingleCoalescer<Req>;
using Rule = int (*)(const CoalesceState&, const CoalesceKnobs&);

thread_local Req* my_req = nullptr;  // the calling thread's request in flight

// What the fake run saw, under mu.
struct Record {
  std::mutex mu;
  uint64_t issued = 0;                         // arrival numbers given out
  std::vector<std::vector<uint64_t>> batches;  // arrival numbers per run, in run order
  std::vector<int> rc;                         // what each run answered (or CSM_ENOMEM: it threw)
  int running = 0, max_running = 0, max_running_after_throw = 0;
  int throws = 0, led_for_others = 0;
  int min_leaders_running = 1 << 30, max_leaders_running = 0;
};

// Queues `r` as the next arrival.
template <typename Run>
void Arrive(Coalescer* co, Record* rec, Req* r, const CoalesceKnobs& knobs, Rule rule, Run run) {
  {
    std::lock_guard<std::mutex> g(rec->mu);
    while (co->state().arrived != rec->issued) std::this_thread::yield();
    r->arrival = rec->issued++;
  }
  my_req = r;
  co->Call(r, knobs, rule, run);
  my_req = nullptr;
}

// A run that records its batch, stays `sleep_us`, and throws on every
// `throw_every`-th call.
auto FakeRun(Record* rec, int sleep_us, int throw_every) {
  return [=](const std::vector<Req*>& batch, int leaders_running) {
    int rc;
    bool thrown;
    {
      std::lock_guard<std::mutex> g(rec->mu);
      const int idx = static_cast<int>(rec->batches.size());
      thrown = throw_every && (idx + 1) % throw_every == 0;
      rc = thrown ? CSM_ENOMEM : idx + 1;
      rec->rc.push_back(rc);
      rec->batches.emplace_back();
      bool mine = false;
      for (Req* q : batch) {
        rec->batches.back().push_back(q->arrival);
        q->batch = idx;
        mine |= q == my_req;
      }
      rec->led_for_others += !mine;
      rec->max_running = std::max(rec->max_running, ++rec->running);
      if (rec->throws) rec->max_running_after_throw = std::max(rec->max_running_after_throw, rec->running);
      rec->throws += thrown;
      rec->min_leaders_running = std::min(rec->min_leaders_running, leaders_running);
      rec->max_leaders_running = std::max(rec->max_leaders_running, leaders_running);
    }
    if (sleep_us) std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
    {
      std::lock_guard<std::mutex> g(rec->mu);
      --rec->running;
    }
    if (thrown) throw std::bad_alloc();
    return rc;
  };
}

// The invariants of every run of `total` calls. exact_order: the runs were
// recorded in the order their batches were taken (one leader).
void CheckRecord(const Record& rec, const CoalesceKnobs& knobs, uint64_t total, bool exact_order) {
  std::vector<int> seen(total, 0);
  uint64_t next = 0;
  for (const auto& b : rec.batches) {
    // A batch may be empty: another leader took the queue, this leader's own
    // request with it, while this one waited for more callers.
    CHECK(b.size() <= static_cast<size_t>(knobs.cap), "batch of %zu, cap %d", b.size(), knobs.cap);
    for (size_t k = 0; k < b.size(); ++k) {
      if (b[k] < total) ++seen[b[k]];
      // The queue is the arrivals less the prefixes taken, so a prefix of it
      // is a run of consecutive arrival numbers.
      CHECK(b[k] == b[0] + k, "batch is no FIFO prefix: element %zu is arrival %llu after %llu", k,
            static_cast<unsigned long long>(b[k]), static_cast<unsigned long long>(b[0]));
    }
    if (exact_order && !b.empty()) {
      CHECK(b[0] == next, "batch starts at arrival %llu, the queue's head was %llu",
            static_cast<unsigned long long>(b[0]), static_cast<unsigned long long>(next));
      next = b[0] + b.size();
    }
  }
  for (uint64_t a = 0; a < total; ++a) CHECK(seen[a] == 1, "arrival %llu was in %d batches", static_cast<unsigned long long>(a), seen[a]);
  CHECK(rec.max_running <= knobs.leaders, "%d runs at once, leaders %d", rec.max_running, knobs.leaders);
  CHECK(rec.min_leaders_running >= 1 && rec.max_leaders_running <= knobs.leaders, "leaders_running in [%d, %d], leaders %d",
        rec.min_leaders_running, rec.max_leaders_running, knobs.leaders);
}

struct LoadResult {
  int max_running, max_running_after_throw, throws;
  size_t batches;
};

// `threads` threads calling `calls` times each, back to back.
LoadResult Load(const CoalesceKnobs& knobs, Rule rule, int threads, int calls, int sleep_us, int throw_every) {
  Coalescer co;
  Record rec;
  std::atomic<int> unanswered{0}, wrong_rc{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&] {
      auto run = FakeRun(&rec, sleep_us, throw_every);
      for (int c = 0; c < calls; ++c) {
        Req r;
        Arrive(&co, &rec, &r, knobs, rule, run);
        if (!r.done || !r.taken || r.batch < 0) {
          ++unanswered;
          continue;
        }
        std::lock_guard<std::mutex> g(rec.mu);
        wrong_rc += r.rc != rec.rc[r.batch];
      }
    });
  for (auto& th : pool) th.join();
  const uint64_t total = static_cast<uint64_t>(threads) * calls;
  CHECK(unanswered == 0, "%d requests came back unanswered", unanswered.load());
  CHECK(wrong_rc == 0, "%d requests do not carry their batch's return code", wrong_rc.load());
  CheckRecord(rec, knobs, total, knobs.leaders == 1);
  const CoalesceState s = co.state();
  CHECK(s.leaders == 0 && s.in_flight == 0 && s.arrived == total, "state after the load: leaders %d in_flight %d arrived %llu",
        s.leaders, s.in_flight, static_cast<unsigned long long>(s.arrived));
  return {rec.max_running, rec.max_running_after_throw, rec.throws, rec.batches.size()};
}

std::string Name(const char* what, Rule rule, const CoalesceKnobs& k) {
  return std::string(what) + (rule == csm::WantLastBatch ? " 2D" : " 3D") + " leaders " + std::to_string(k.leaders) + " cap " +
         std::to_string(k.cap) + " window " + std::to_string(k.window_us);
}

void TestLoad() {
  for (Rule rule : {Rule(csm::WantLastBatch), Rule(csm::WantShareOfCallers)})
    for (int leaders : {1, 2, 3})
      for (int cap : {3, 512})
        for (int window_us : {0, 150}) {
          const CoalesceKnobs knobs{true, leaders, window_us, cap};
          Case(Name("load", rule, knobs));
          Load(knobs, rule, 16, 200, 0, 0);
        }
}

// A run that takes 300 us: the concurrency bound is reached, not only kept,
// also after batches that throw.
void TestBoundReached() {
  for (Rule rule : {Rule(csm::WantLastBatch), Rule(csm::WantShareOfCallers)})
    for (int leaders : {1, 2, 3})
      for (int throw_every : {0, 5}) {
        const CoalesceKnobs knobs{true, leaders, 150, 512};
        Case(Name(throw_every ? "throwing runs" : "slow runs", rule, knobs));
        const LoadResult r = Load(knobs, rule, 16, 40, 300, throw_every);
        CHECK(r.max_running == leaders, "at most %d runs at once, leaders %d", r.max_running, leaders);
        if (throw_every) {
          CHECK(r.throws > 0, "no run threw in %zu batches", r.batches);
          CHECK(r.max_running_after_throw == leaders, "at most %d runs at once after a throw, leaders %d",
                r.max_running_after_throw, leaders);
        }
      }
}

// Eight callers arriving one by one while the first one's batch runs: with
// one leader the batches are exactly the queue's prefixes.
void TestStagedFifo() {
  for (int cap : {1, 3, 512}) {
    const CoalesceKnobs knobs{true, 1, 0, cap};
    Case(Name("staged arrivals", csm::WantLastBatch, knobs));
    Coalescer co;
    Record rec;
    std::mutex gate_mu;
    std::condition_variable gate_cv;
    bool open = false;
    auto record = FakeRun(&rec, 0, 0);
    auto run = [&](const std::vector<Req*>& batch, int leaders_running) {
      const int rc = record(batch, leaders_running);
      std::unique_lock<std::mutex> g(gate_mu);
      gate_cv.wait(g, [&] { return open; });
      return rc;
    };
    constexpr int kCallers = 8;
    std::vector<Req> reqs(kCallers);
    std::vector<std::thread> pool;
    for (int t = 0; t < kCallers; ++t) {
      pool.emplace_back([&, t] { Arrive(&co, &rec, &reqs[t], knobs, csm::WantLastBatch, run); });
      while (co.state().arrived != static_cast<uint64_t>(t + 1)) std::this_thread::yield();
    }
    {
      std::lock_guard<std::mutex> g(gate_mu);
      open = true;
    }
    gate_cv.notify_all();
    for (auto& th : pool) th.join();
    CheckRecord(rec, knobs, kCallers, true);
    // The first caller led alone at once; the rest were cut at the cap.
    const size_t expect = 1 + (kCallers - 1 + cap - 1) / cap;
    CHECK(rec.batches.size() == expect, "%zu batches, expected %zu", rec.batches.size(), expect);
    for (int t = 0; t < kCallers; ++t) {
      CHECK(reqs[t].arrival == static_cast<uint64_t>(t), "caller %d arrived as %llu", t, static_cast<unsigned long long>(reqs[t].arrival));
      CHECK(reqs[t].done && reqs[t].batch == (t == 0 ? 0 : 1 + (t - 1) / cap), "caller %d done %d in batch %d", t, reqs[t].done, reqs[t].batch);
    }
  }
}

// A cap of 3 and a leader whose own request is fourth in the queue: it serves
// the three before it, leads again and serves itself. Callers 1 to 3 may not
// lead (their knob allows no leader), so who leads is not left to the
// scheduler.
void TestSmallCap() {
  Case("small cap");
  Coalescer co;
  Record rec;
  std::mutex gate_mu;
  std::condition_variable gate_cv;
  bool open = false;
  auto record = FakeRun(&rec, 0, 0);
  auto run = [&](const std::vector<Req*>& batch, int leaders_running) {
    const int rc = record(batch, leaders_running);
    std::unique_lock<std::mutex> g(gate_mu);
    gate_cv.wait(g, [&] { return open; });
    return rc;
  };
  const CoalesceKnobs leads{true, 1, 0, 3}, follows{true, 0, 0, 3};
  std::vector<Req> reqs(5);
  std::vector<std::thread> pool;
  for (int t = 0; t < 5; ++t) {
    pool.emplace_back([&, t] { Arrive(&co, &rec, &reqs[t], t == 0 || t == 4 ? leads : follows, csm::WantLastBatch, run); });
    while (co.state().arrived != static_cast<uint64_t>(t + 1)) std::this_thread::yield();
  }
  {
    std::lock_guard<std::mutex> g(gate_mu);
    open = true;
  }
  gate_cv.notify_all();
  for (auto& th : pool) th.join();
  CheckRecord(rec, leads, 5, true);
  CHECK(rec.batches.size() == 3 && rec.batches[1].size() == 3 && rec.batches[2].size() == 1, "%zu batches", rec.batches.size());
  CHECK(rec.led_for_others == 1, "%d batches without their leader's request", rec.led_for_others);
  for (int t = 0; t < 5; ++t)
    CHECK(reqs[t].done && reqs[t].batch == (t == 0 ? 0 : t == 4 ? 2 : 1), "caller %d done %d in batch %d", t, reqs[t].done, reqs[t].batch);
}

// One caller after a batch of four: it waits for four, for the window.
void TestLoneCaller() {
  for (int window_us : {0, 150}) {
    Case("lone caller, window " + std::to_string(window_us));
    Coalescer co;
    Record rec;
    auto run = FakeRun(&rec, 0, 0);
    const CoalesceKnobs gather{true, 1, 5 * 1000 * 1000, 512};  // one leader waiting for all four
    std::vector<Req> reqs(4);
    std::vector<std::thread> pool;
    for (int t = 0; t < 4; ++t)
      pool.emplace_back([&, t] { Arrive(&co, &rec, &reqs[t], gather, [](const CoalesceState&, const CoalesceKnobs&) { return 4; }, run); });
    for (auto& th : pool) th.join();
    CHECK(co.state().last_batch == 4, "the batch before had %d", co.state().last_batch);
    const CoalesceKnobs knobs{true, 3, window_us, 512};
    static int wanted;  // what the rule asked the lone caller to wait for
    wanted = 0;
    Req r;
    const auto t0 = std::chrono::steady_clock::now();
    Arrive(&co, &rec, &r, knobs, [](const CoalesceState& s, const CoalesceKnobs& k) { return wanted = csm::WantLastBatch(s, k); }, run);
    const auto waited = std::chrono::steady_clock::now() - t0;
    CHECK(wanted == 4, "the lone caller waited for %d", wanted);
    CHECK(r.done && r.rc == 2, "done %d rc %d", r.done, r.rc);
    CHECK(rec.batches.size() == 2 && rec.batches[1].size() == 1, "%zu batches", rec.batches.size());
    CHECK(waited >= std::chrono::microseconds(window_us), "returned before the window");
    CHECK(co.state().last_batch == 1, "last_batch %d after a batch of one", co.state().last_batch);
  }
}

// Coalescing off: the call itself runs its one request.
void TestOff() {
  Case("off");
  Coalescer co;
  const CoalesceKnobs knobs{false, 3, 150, 512};
  const std::thread::id main_thread = std::this_thread::get_id();
  for (bool throws : {false, true}) {
    Req r;
    int runs = 0;
    co.Call(&r, knobs, csm::WantLastBatch, [&](const std::vector<Req*>& batch, int leaders_running) {
      ++runs;
      CHECK(batch.size() == 1 && batch[0] == &r, "batch of %zu", batch.size());
      CHECK(leaders_running == 1, "leaders_running %d", leaders_running);
      CHECK(std::this_thread::get_id() == main_thread, "run on another thread");
      if (throws) throw std::bad_alloc();
      return 7;
    });
    CHECK(runs == 1 && r.done && r.rc == (throws ? CSM_ENOMEM : 7), "runs %d done %d rc %d", runs, r.done, r.rc);
  }
  const CoalesceState s = co.state();
  CHECK(s.arrived == 0 && s.in_flight == 0 && s.leaders == 0, "the queue's state was touched");
}

// The two rules and the state updates, without threads.
void TestRules() {
  Case("rules");
  const CoalesceKnobs k2{true, 3, 150, 512}, k3{true, 2, 300, 512};
  CoalesceState s;
  CHECK(csm::WantLastBatch(s, k2) == 1, "a fresh queue's leader waits for %d", csm::WantLastBatch(s, k2));
  for (int last : {-1, 0, 1, 2, 7, 512}) {
    s.last_batch = last;
    CHECK(csm::WantLastBatch(s, k2) == std::max(1, last), "last_batch %d: want %d", last, csm::WantLastBatch(s, k2));
  }
  s = CoalesceState{};
  for (int i = 1; i <= 16; ++i) {
    csm::CoalesceArrive(&s);
    CHECK(s.in_flight == i && s.callers == i && s.arrived == static_cast<uint64_t>(i), "arrival %d: in_flight %d callers %d", i, s.in_flight, s.callers);
  }
  s.leaders = 0;
  CHECK(csm::WantShareOfCallers(s, k3) == 8, "16 callers over 2 leaders: %d", csm::WantShareOfCallers(s, k3));
  for (int callers = 0; callers <= 40; ++callers)
    for (int leaders = 1; leaders <= 4; ++leaders) {
      CoalesceState c;
      c.callers = callers;
      const int want = csm::WantShareOfCallers(c, CoalesceKnobs{true, leaders, 0, 512});
      CHECK(want * leaders >= callers && (want - 1) * leaders < callers, "ceil(%d / %d) = %d", callers, leaders, want);
    }
  // Ten of the sixteen return: callers stays at the high-water mark, then
  // drops by one per batch down to the calls still in flight.
  s.in_flight = 6;
  for (int batch = 1; batch <= 14; ++batch) {
    csm::CoalesceLead(&s);
    CHECK(s.leaders == batch, "leaders %d after %d leads", s.leaders, batch);
    CHECK(s.callers == std::max(6, 16 - batch), "batch %d: callers %d", batch, s.callers);
  }
  csm::CoalesceArrive(&s);
  CHECK(s.in_flight == 7 && s.callers == 7, "in_flight %d callers %d", s.in_flight, s.callers);
}

void TestHostPool() {
  Case("HostPool");
  auto visit_once = [](int64_t num, bool pool_only) {
    std::vector<std::atomic<int>> hits(static_cast<size_t>(num));
    for (auto& h : hits) h = 0;
    const std::function<void(int64_t)> f = [&](int64_t i) { ++hits[static_cast<size_t>(i)]; };
    if (pool_only) {
      csm::HostPool::Get().Run(num, f);
    } else {
      csm::ParallelPairs(num, f);
    }
    int64_t wrong = 0;
    for (auto& h : hits) wrong += h != 1;
    return wrong;
  };
  for (int repeat = 0; repeat < 3; ++repeat)
    for (int64_t num : {0, 1, 63, 64, 10000})
      for (bool pool_only : {true, false}) {
        const int64_t wrong = visit_once(num, pool_only);
        CHECK(wrong == 0, "%lld of %lld indices not visited once", static_cast<long long>(wrong), static_cast<long long>(num));
      }
  std::atomic<int64_t> wrong{0};
  std::vector<std::thread> two;
  for (int t = 0; t < 2; ++t)
    two.emplace_back([&] {
      for (int repeat = 0; repeat < 20; ++repeat)
        for (int64_t num : {0, 1, 63, 64, 10000}) wrong += visit_once(num, repeat % 2 == 0);
    });
  for (auto& th : two) th.join();
  CHECK(wrong == 0, "%lld indices not visited once from two threads", static_cast<long long>(wrong.load()));
}

}  // namespace

int main() {
  std::mutex wd_mu;
  std::condition_variable wd_cv;
  bool finished = false;
  std::thread watchdog([&] {
    std::unique_lock<std::mutex> g(wd_mu);
    if (wd_cv.wait_for(g, std::chrono::seconds(kWatchdogSeconds), [&] { return finished; })) return;
    std::printf("WATCHDOG: still in [%s] after %d s\n", CaseName().c_str(), kWatchdogSeconds);
    std::fflush(stdout);
    std::_Exit(3);
  });
  TestRules();
  TestOff();
  TestLoneCaller();
  TestStagedFifo();
  TestSmallCap();
  TestLoad();
  TestBoundReached();
  TestHostPool();
  {
    std::lock_guard<std::mutex> g(wd_mu);
    finished = true;
  }
  wd_cv.notify_all();
  watchdog.join();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("single coalesce OK\n");
  return 0;
}
