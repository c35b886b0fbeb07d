// The host skeleton the three range-data inserters share (insert2d.hip,
// insert_tsdf2d.hip, insert3d.hip) around their own kernels; DESIGN.md, "The
// inserters' shared host skeleton", has the steps in order. The rule they keep:
// whatever can refuse a call or fail cleanly (validation, planning, every
// allocation, ReserveUpload) comes before the first enqueue, and the planned
// buffers then go back to ctx->pool, so the grids stay as they were. A HIP
// failure after that leaves the stream's state unknown: the call returns
// CSM_EHIP at once and destructors free the planned and retired buffers, so a
// buffer a half-enqueued kernel may write never returns to the pool.
// Everything here has internal linkage.
#ifndef CSM_INSERT_HOST_H_
#define CSM_INSERT_HOST_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "csm_internal.h"

namespace csm {
namespace {

constexpr int64_t kMaxScanPoints = 1 << 24;  // returns (or misses) of one scan
constexpr int kMaxGridY = 65535;             // scans or jobs per launch (gridDim.y)
constexpr size_t kPlanThreads = 8;           // most threads a call is planned on
constexpr int64_t kPlanThreaded = 32768;     // returns per call from which threads pay off

inline int EnsureDevice(csm_context* ctx) {
  return hipSetDevice(ctx->device) == hipSuccess ? CSM_OK : CSM_EHIP;
}

inline bool Finite3(const float* p) {
  return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
}

inline unsigned Blocks(int64_t items, int per_block, int cap) {
  const int64_t b = (items + per_block - 1) / per_block;
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(b, cap)));
}

inline size_t Align(size_t n) { return (n + 255) & ~size_t(255); }

// probability_values.h:32-35.
inline float Odds(float p) { return p / (1.f - p); }
inline float ProbabilityFromOdds(float odds) { return odds / (odds + 1.f); }

// The hit and miss tables of a (hit, miss) probability pair in `tabs` (hit
// first, 32768 entries each, no update marker), re-made when the pair is not
// `key`. make(odds, out) is the inserter's ComputeLookupTableToApplyOdds.
template <typename Make>
int EnsureOddsTables(csm_context* ctx, float hit, float miss, const Make& make, DevBuf* tabs,
                     float* key) {
  if (key[0] == hit && key[1] == miss) return CSM_OK;
  std::vector<uint16_t> t(2 * 32768);
  make(Odds(hit), t.data());
  make(Odds(miss), t.data() + 32768);
  for (uint16_t& v : t) v &= 0x7fff;
  // Earlier inserts on the stream may still read the previous tables.
  CSM_HIP(hipStreamSynchronize(ctx->stream));
  if (int rc = tabs->Reserve(t.size() * sizeof(uint16_t))) return rc;
  CSM_HIP(hipMemcpy(tabs->ptr, t.data(), t.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  key[0] = hit;
  key[1] = miss;
  return CSM_OK;
}

// One point array of a call's scans: offsets from 0 that never fall, at most
// kMaxScanPoints per scan, every point finite.
inline bool ValidPoints(int32_t num_scans, const int64_t* off, const float* xyz) {
  if (off[0] != 0) return false;
  for (int s = 0; s < num_scans; ++s)
    if (off[s + 1] < off[s] || off[s + 1] - off[s] > kMaxScanPoints) return false;
  const int64_t total = off[num_scans];
  if (total > 0 && !xyz) return false;
  for (int64_t i = 0; i < total; ++i)
    if (!Finite3(xyz + 3 * i)) return false;
  return true;
}

// The origins and returns of num_scans > 0 scans.
inline bool ValidScans(int32_t num_scans, const float* origins, const int64_t* ret_off,
                       const float* returns) {
  for (int s = 0; s < num_scans; ++s)
    if (!Finite3(origins + 3 * s)) return false;
  return ValidPoints(num_scans, ret_off, returns);
}

// Every grid belongs to ctx and none is given twice.
template <typename Grid>
bool ValidHandles(const csm_context* ctx, Grid* const* grids, int32_t num_grids) {
  for (int g = 0; g < num_grids; ++g) {
    if (grids[g]->ctx != ctx) return false;
    for (int h = 0; h < g; ++h)
      if (grids[h] == grids[g]) return false;
  }
  return true;
}

// task(0) .. task(num_tasks - 1), each once: on up to kPlanThreads threads
// when the call has kPlanThreaded returns or more, else on this one.
template <typename Task>
void RunPlanTasks(size_t num_tasks, int64_t total_returns, const Task& task) {
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (size_t t; (t = next.fetch_add(1)) < num_tasks;) task(t);
  };
  const size_t hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t nthreads =
      total_returns >= kPlanThreaded ? std::min<size_t>({num_tasks, hw, kPlanThreads}) : 1;
  std::vector<std::thread> pool;
  try {
    for (size_t t = 1; t < nthreads; ++t) pool.emplace_back(work);
  } catch (...) {  // no more threads: the ones there are share the tasks
  }
  work();
  for (std::thread& t : pool) t.join();
}

// A staging slot of `bytes` and room for them in `dev`, the inserter's
// per-context device buffer. Before the first enqueue of the call.
inline int ReserveUpload(csm_context* ctx, StageRing* ring, DevBuf* dev, size_t bytes,
                         StageRing::Slot** slot) {
  const int rc = ring->Take(bytes, slot);
  if (rc != CSM_OK || dev->bytes >= bytes) return rc;
  // The buffer is replaced: earlier inserts on the stream may still read it.
  CSM_HIP(hipStreamSynchronize(ctx->stream));
  return dev->Reserve(bytes + bytes / 2);
}

// The call's one upload, once the slot is filled.
inline int Upload(csm_context* ctx, StageRing::Slot* slot, DevBuf* dev, size_t bytes) {
  CSM_HIP(hipMemcpyAsync(dev->ptr, slot->buf.ptr, bytes, hipMemcpyHostToDevice, ctx->stream));
  CSM_HIP(hipEventRecord(slot->copied, ctx->stream));
  return CSM_OK;
}

// The scans or jobs of a round go out kMaxGridY at a time: how many from y0.
inline unsigned ChunkOf(int y0, int end) {
  return static_cast<unsigned>(std::min(kMaxGridY, end - y0));
}

}  // namespace
}  // namespace csm

#endif  // CSM_INSERT_HOST_H_
