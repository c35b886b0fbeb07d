// Coalescing of concurrent single Match / MatchFullSubmap calls, 2D and 3D.
// Host-only and pure: no device type and no getenv, so that
// tests/cpp/single_coalesce_test.cc runs the protocol on the CPU under
// ThreadSanitizer, AddressSanitizer and UBSan (tests/test_single_coalesce.py).
//
// The reference's tasks call Match / MatchFullSubmap concurrently from
// ThreadPool workers (constraint_builder_2d.cc:100-111, :188-215;
// constraint_builder_3d.cc:200-241). One call is one pair, far too little to
// fill the GPU, so concurrent callers of one owner context are coalesced: each
// queues its pair; a caller that finds fewer than `leaders` batches running
// becomes a leader, waits up to `window_us` until the queue holds as many
// requests as its rule asks for, takes the queue (`cap` requests at most,
// oldest first) and searches it as one batch, then wakes the callers it
// served. A pair's result does not depend on the batch it lands in.
//
// The two rules for how many queued requests a leader waits for:
//   2D, WantLastBatch: as many as the previous batch had. A lone caller never
//   waits (its previous batch had one pair).
//   3D, WantShareOfCallers: ceil(callers / leaders), `callers` being the
//   recent high-water mark of calls in flight (one less per batch). With T
//   threads calling back to back, `leaders` batches of about T / leaders
//   alternate, one searching while another's callers return and queue again.
//   A 3D pair costs a few microseconds of device time against ~0.3 ms of
//   fixed latency per batch (the pipeline's launches, copies and
//   synchronizations), so batch size, not device time, sets the single-call
//   rate: under the 2D rule with 3 leaders 3D settled at ~2 pairs per batch
//   (profiles/r6h/).
#ifndef CSM_SINGLE_COALESCE_H_
#define CSM_SINGLE_COALESCE_H_

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/csm_amd.h"

namespace csm {

// What the coalescer keeps in a queued call; the request types derive from it.
struct CoalesceReq {
  int rc = CSM_OK;     // its batch's return code
  bool taken = false;  // in some leader's batch: no longer queued
  bool done = false;   // answered
};

struct CoalesceKnobs {
  bool on;        // false: every call runs alone, on its caller's thread
  int leaders;    // batches in flight at most
  int window_us;  // a leader's longest wait for more callers
  int cap;        // requests per batch at most
};

struct CoalesceState {
  int leaders = 0;       // batches running, their leaders' waits included
  int last_batch = 1;    // the size of the batch taken last
  int in_flight = 0;     // calls between queueing and their return
  int callers = 0;       // recent high-water of in_flight (one less per batch)
  uint64_t arrived = 0;  // calls queued so far (nothing here reads it: it lets a test order arrivals)
};

inline void CoalesceArrive(CoalesceState* s) {
  s->callers = std::max(s->callers, ++s->in_flight);
  ++s->arrived;
}
inline void CoalesceLead(CoalesceState* s) {
  ++s->leaders;
  s->callers = std::max(s->in_flight, s->callers - 1);
}
inline int WantLastBatch(const CoalesceState& s, const CoalesceKnobs&) {
  return std::max(1, s.last_batch);
}
inline int WantShareOfCallers(const CoalesceState& s, const CoalesceKnobs& k) {
  return (s.callers + k.leaders - 1) / k.leaders;
}

// One owner context's queue of single calls of one dimension. Req derives
// from CoalesceReq.
template <typename Req>
class SingleCoalescer {
 public:
  // Answers `req` (rc, done) as part of some batch. want(state, knobs) is one
  // of the rules above; run(batch, leaders_running) searches a batch and
  // returns its code, leaders_running counting this batch's leader.
  template <typename Want, typename Run>
  void Call(Req* req, const CoalesceKnobs& knobs, Want want, Run run) {
    if (!knobs.on) {
      req->rc = Guarded(run, std::vector<Req*>{req}, 1);
      req->done = true;
      return;
    }
    std::unique_lock<std::mutex> lk(mu_);
    queue_.push_back(req);
    CoalesceArrive(&state_);
    cv_.notify_all();
    while (!req->done) {
      if (req->taken || state_.leaders >= knobs.leaders) {
        cv_.wait(lk);
        continue;
      }
      CoalesceLead(&state_);
      const size_t want_n = static_cast<size_t>(want(state_, knobs));
      const auto deadline =
          std::chrono::steady_clock::now() + std::chrono::microseconds(knobs.window_us);
      while (queue_.size() < want_n && cv_.wait_until(lk, deadline) != std::cv_status::timeout) {
      }
      // The oldest requests, which need not include this leader's own (cap):
      // it then leads again on its next turn.
      const size_t take_n = std::min(queue_.size(), static_cast<size_t>(knobs.cap));
      const std::vector<Req*> take(queue_.begin(), queue_.begin() + take_n);
      queue_.erase(queue_.begin(), queue_.begin() + take_n);
      for (Req* q : take) q->taken = true;
      state_.last_batch = static_cast<int>(take_n);
      const int leaders_running = state_.leaders;
      lk.unlock();
      const int rc = Guarded(run, take, leaders_running);
      lk.lock();
      for (Req* q : take) {
        q->rc = rc;
        q->done = true;
      }
      --state_.leaders;
      cv_.notify_all();
    }
    --state_.in_flight;
  }

  CoalesceState state() {
    std::lock_guard<std::mutex> g(mu_);
    return state_;
  }

 private:
  // Whatever happens in the batch (an allocation that throws), every request
  // taken is answered and the leader slot given back; otherwise their callers
  // would wait on cv_ forever, and no exception crosses the C-ABI.
  template <typename Run>
  static int Guarded(Run& run, const std::vector<Req*>& batch, int leaders_running) {
    try {
      return run(batch, leaders_running);
    } catch (...) {
      return CSM_ENOMEM;
    }
  }

  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Req*> queue_;
  CoalesceState state_;
};

}  // namespace csm

#endif  // CSM_SINGLE_COALESCE_H_
