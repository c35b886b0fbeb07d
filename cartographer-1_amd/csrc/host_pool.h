// Host worker pool for a batch's per-pair host phases (host3d.cc). Host-only:
// no device type, so that tests/cpp/single_coalesce_test.cc runs it on the CPU
// under ThreadSanitizer, AddressSanitizer and UBSan.
#ifndef CSM_HOST_POOL_H_
#define CSM_HOST_POOL_H_

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace csm {

// A persistent pool of host workers for the batch's per-pair host phases
// (spawning threads per phase cost ~1 ms per phase on the GPU box).
class HostPool {
 public:
  static HostPool& Get() {
    static HostPool pool;
    return pool;
  }
  // Runs f(i) for i in [0, num) on the workers and the calling thread.
  void Run(int64_t num, const std::function<void(int64_t)>& f) {
    if (num <= 0) return;
    std::unique_lock<std::mutex> lock(mu_);  // one batch phase at a time
    {
      std::lock_guard<std::mutex> g(state_);
      f_ = &f;
      num_ = num;
      next_.store(0);
      active_ = static_cast<int>(workers_.size());
      ++epoch_;
    }
    cv_.notify_all();
    Work(f, num);
    std::unique_lock<std::mutex> g(state_);
    done_.wait(g, [&] { return active_ == 0; });
    f_ = nullptr;
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> g(state_);
      stop_ = true;
      ++epoch_;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }

 private:
  HostPool() {
    const int nt = static_cast<int>(
        std::max<unsigned>(1, std::min<unsigned>(16, std::thread::hardware_concurrency())));
    for (int t = 1; t < nt; ++t) workers_.emplace_back([this] { Loop(); });
  }
  void Work(const std::function<void(int64_t)>& f, int64_t num) {
    for (int64_t i = next_.fetch_add(1); i < num; i = next_.fetch_add(1)) f(i);
  }
  void Loop() {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(int64_t)>* f;
      int64_t num;
      {
        std::unique_lock<std::mutex> g(state_);
        cv_.wait(g, [&] { return stop_ || epoch_ != seen; });
        if (stop_) return;
        seen = epoch_;
        f = f_;
        num = num_;
      }
      Work(*f, num);
      std::lock_guard<std::mutex> g(state_);
      if (--active_ == 0) done_.notify_one();
    }
  }
  std::mutex mu_, state_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> workers_;
  const std::function<void(int64_t)>* f_ = nullptr;
  int64_t num_ = 0;
  std::atomic<int64_t> next_{0};
  int active_ = 0;
  uint64_t epoch_ = 0;
  bool stop_ = false;
};

template <typename F>
void ParallelPairs(int64_t num, F&& f) {
  if (num < 64) {  // not worth waking the pool
    for (int64_t i = 0; i < num; ++i) f(i);
    return;
  }
  const std::function<void(int64_t)> fn = f;
  HostPool::Get().Run(num, fn);
}

}  // namespace csm

#endif  // CSM_HOST_POOL_H_
