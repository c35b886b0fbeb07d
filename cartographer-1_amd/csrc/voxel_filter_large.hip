// Voxel filters for clouds too large for LDS, on gfx950: sensor::VoxelFilter
// and sensor::AdaptiveVoxelFilter (reference sensor/internal/voxel_filter.cc)
// for one cloud of up to 2^20 points, the size of a 3D sweep
// (local_trajectory_builder_3d.cc:682-683 and :734-745). voxel_filter.hip keeps
// a cloud of up to 8192 points in one workgroup's LDS; this file is the same
// method spread over the device, with the same kept set: the reference's
// RandomizedVoxelFilterIndices (:136-162), draw for draw.
//
// One VoxelFilter over n points (tiles of 1024 points, 4 per thread):
//   vfl_keys         one thread per point: the 64-bit voxel key, and the
//                    point's index as the value.
//   rocprim::radix_sort_pairs on all 64 bits; stable, so each voxel's run
//                    ascends by point index.
//   vfl_ranks        run heads are the sorted positions whose key differs from
//                    the predecessor's; a position's head is the max-scan of
//                    head positions (a block scan; a block's carry-in, the
//                    head of the run that crosses into it, is the lower bound
//                    of its first key in the sorted keys before it). The rank,
//                    position minus head, is scattered to input order.
//   vfl_draw_counts  per tile of input order, the points of rank > 0: each
//                    makes one uniform_int_distribution(1, rank + 1) draw.
//   vfl_draw         a point's stream position is the number of drawing points
//                    before it (tile counts before the block, a block scan
//                    within). Each thread jumps minstd_rand0 to the position of
//                    its first drawing point (MinstdJump) and steps through
//                    its four. A rejected output (libstdc++ draws again, which
//                    moves every later draw one place on) is reported by an
//                    integer atomicMin of the point's index.
//   vfl_pick         per voxel the last successful point, else the first: an
//                    integer atomicMax of the sorted position into the run
//                    head's slot.
//   vfl_mask         the keep mask in input order and the kept count.
// The host reads eight bytes back per draw pass: the first rejected point and
// the count. With no rejection, which is the usual case (a draw with k
// outcomes is rejected with probability below k / 2^31), that is the only
// synchronise of the filter. Otherwise the draws before the rejected point
// stand, and vfl_draw runs again from that point on with every position
// shifted by the rejections so far (the point's own redraw is its old position
// plus one), then vfl_pick and vfl_mask again: passes = rejections + 1, and
// no pass is a one-lane walk over the cloud.
//
// AdaptiveVoxelFilter: vfl_range_mask and an ordered compaction are
// FilterByMaxRange (:31-36); the host walks AdaptivelyVoxelFiltered's lengths
// (:38-76, VfLengthSearch in voxel_filter_dev.h, shared with the LDS kernel)
// and runs one VoxelFilter per length on the range-filtered cloud, keeping the
// accepted mask; vfl_scatter_mask writes it back over the input's points.
// Synchronises: one for the range-filtered count, one per VoxelFilter pass.
//
// The ordered compaction (vfl_sel_counts, vfl_compact) is what the 3D front
// end (range_data3d.hip) also uses: per-tile counts, the counts of the tiles
// before a block summed by the block, a block scan, a scatter. No atomics
// decide an order anywhere.

#include <hip/hip_runtime.h>
// The radix sort alone: rocprim.hpp also pulls in texture iterators.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstring>

#include "csm_internal.h"
#include "voxel_filter_dev.h"

namespace csm {
namespace {

constexpr int kVflThreads = 256;
constexpr int kVflPer = 4;                        // consecutive points per thread
constexpr int kVflTile = kVflThreads * kVflPer;   // 1024
constexpr int kVflMaxTiles = static_cast<int>(kVflMaxPoints / kVflTile);  // 1024
constexpr uint32_t kNoRejection = 0xffffffffu;

// What a pass reports: the first point with a rejected draw, the kept count.
struct VflReport {
  uint32_t first_rejected;
  int32_t kept;
};

size_t Align256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

// The working set of one cloud of up to `cap` points, carved from vfl_work.
struct VflWork {
  uint64_t *keys, *sorted_keys;
  uint32_t *idx, *sorted_idx, *head, *rank, *index;  // index: range-filtered point -> input point
  int32_t* best;
  uint8_t *ok, *cur, *res, *sel;
  uint32_t* tile_counts;  // [kVflMaxTiles]
  VflReport* report;
  int32_t* count;
  size_t bytes;
  VflWork(char* base, size_t cap) {
    size_t at = 0;
    auto take = [&](size_t n) {
      char* p = base ? base + at : nullptr;
      at += Align256(n);
      return p;
    };
    keys = reinterpret_cast<uint64_t*>(take(8 * cap));
    sorted_keys = reinterpret_cast<uint64_t*>(take(8 * cap));
    idx = reinterpret_cast<uint32_t*>(take(4 * cap));
    sorted_idx = reinterpret_cast<uint32_t*>(take(4 * cap));
    head = reinterpret_cast<uint32_t*>(take(4 * cap));
    rank = reinterpret_cast<uint32_t*>(take(4 * cap));
    index = reinterpret_cast<uint32_t*>(take(4 * cap));
    best = reinterpret_cast<int32_t*>(take(4 * cap));
    ok = reinterpret_cast<uint8_t*>(take(cap));
    cur = reinterpret_cast<uint8_t*>(take(cap));
    res = reinterpret_cast<uint8_t*>(take(cap));
    sel = reinterpret_cast<uint8_t*>(take(cap));
    tile_counts = reinterpret_cast<uint32_t*>(take(4 * kVflMaxTiles));
    report = reinterpret_cast<VflReport*>(take(sizeof(VflReport)));
    count = reinterpret_cast<int32_t*>(take(sizeof(int32_t)));
    bytes = at;
  }
};

// Block scans over one value per thread (4 waves). Every thread calls them.
__device__ __forceinline__ uint32_t BlockExclusiveSum(uint32_t v, uint32_t* total, uint32_t* tmp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) tmp[w] = x;
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int i = 0; i < kVflThreads / 64; ++i) {
    if (i < w) off += tmp[i];
    tot += tmp[i];
  }
  __syncthreads();
  *total = tot;
  return off + x - v;
}

__device__ __forceinline__ int BlockExclusiveMax(int v, int* tmp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x = max(x, y);
  }
  int ex = __shfl_up(x, 1, 64);
  if (lane == 0) ex = -1;
  if (lane == 63) tmp[w] = x;
  __syncthreads();
  for (int i = 0; i < w; ++i) ex = max(ex, tmp[i]);
  __syncthreads();
  return ex;
}

// The sum of counts[0, blockIdx.x): what the tiles before this block hold.
__device__ __forceinline__ uint32_t TilesBefore(const uint32_t* __restrict__ counts, uint32_t* tmp) {
  uint32_t v = 0;
  for (unsigned i = threadIdx.x; i < blockIdx.x; i += kVflThreads) v += counts[i];
  uint32_t total = 0;
  (void)BlockExclusiveSum(v, &total, tmp);
  return total;
}

__global__ void __launch_bounds__(kVflThreads)
vfl_keys(const float* __restrict__ xyz, int n, float resolution, uint64_t* __restrict__ keys,
         uint32_t* __restrict__ idx, VflReport* __restrict__ report) {
  const int i = blockIdx.x * kVflThreads + threadIdx.x;
  if (i == 0) {
    report->first_rejected = kNoRejection;
    report->kept = 0;
  }
  if (i >= n) return;
  const size_t at = 3 * static_cast<size_t>(i);
  keys[i] = VoxelKey(xyz[at], xyz[at + 1], xyz[at + 2], resolution);
  idx[i] = static_cast<uint32_t>(i);
}

__global__ void vfl_reset_report(VflReport* __restrict__ report) {
  report->first_rejected = kNoRejection;
  report->kept = 0;
}

__global__ void __launch_bounds__(kVflThreads)
vfl_ranks(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ sorted_idx, int n,
          uint32_t* __restrict__ head, uint32_t* __restrict__ rank) {
  __shared__ int tmp[kVflThreads / 64];
  __shared__ int carry;
  const int base = blockIdx.x * kVflTile;
  if (threadIdx.x == 0) {
    // The head of the run this tile starts in: the first position holding the
    // tile's first key (base < n: the grid covers n).
    int lo = base;
    if (base > 0 && keys[base - 1] == keys[base]) {
      const uint64_t k = keys[base];
      int hi = base - 1;  // keys[hi] == k
      lo = 0;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
      }
    }
    carry = lo;
  }
  const int s0 = base + static_cast<int>(threadIdx.x) * kVflPer;
  uint64_t k[kVflPer];
  uint32_t heads = 0;
  uint64_t prev = (s0 > 0 && s0 <= n) ? keys[s0 - 1] : 0;
#pragma unroll
  for (int e = 0; e < kVflPer; ++e) {
    const int s = s0 + e;
    k[e] = s < n ? keys[s] : 0;
    if (s < n && (s == 0 || k[e] != prev)) heads |= 1u << e;
    prev = k[e];
  }
  const int last_head = heads ? s0 + 31 - __clz(heads) : -1;
  int start = BlockExclusiveMax(last_head, tmp);  // orders `carry` too
  start = max(start, carry);
#pragma unroll
  for (int e = 0; e < kVflPer; ++e) {
    const int s = s0 + e;
    if (s >= n) break;
    if (heads & (1u << e)) start = s;
    head[s] = static_cast<uint32_t>(start);
    rank[sorted_idx[s]] = static_cast<uint32_t>(s - start);
  }
}

__global__ void __launch_bounds__(kVflThreads)
vfl_draw_counts(const uint32_t* __restrict__ rank, int n, uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t tmp[kVflThreads / 64];
  const int j0 = blockIdx.x * kVflTile + static_cast<int>(threadIdx.x) * kVflPer;
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < kVflPer; ++e)
    if (j0 + e < n && rank[j0 + e] > 0) ++c;
  uint32_t total = 0;
  (void)BlockExclusiveSum(c, &total, tmp);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// Draws for the points from `start` on, `shift` rejections into the stream.
__global__ void __launch_bounds__(kVflThreads)
vfl_draw(const uint32_t* __restrict__ rank, int n, const uint32_t* __restrict__ tile_counts,
         int start, uint32_t shift, uint8_t* __restrict__ ok, int32_t* __restrict__ best,
         VflReport* __restrict__ report) {
  __shared__ uint32_t tmp[kVflThreads / 64];
  const int j0 = blockIdx.x * kVflTile + static_cast<int>(threadIdx.x) * kVflPer;
  uint32_t r[kVflPer];
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < kVflPer; ++e) {
    r[e] = j0 + e < n ? rank[j0 + e] : 0;
    if (r[e] > 0) ++c;
  }
  const uint32_t before = TilesBefore(tile_counts, tmp);
  uint32_t total = 0;
  uint32_t pos = before + BlockExclusiveSum(c, &total, tmp);
  uint32_t state = 0;
  bool seeded = false;
#pragma unroll
  for (int e = 0; e < kVflPer; ++e) {
    const int j = j0 + e;
    if (j >= n) break;
    best[j] = -1;  // the voxels' slots, for vfl_pick (any one-to-one cover of [0, n) does)
    if (r[e] == 0) {
      ok[j] = 0;
      continue;
    }
    if (j >= start) {
      if (!seeded) {
        state = MinstdJump(pos + shift);
        seeded = true;
      }
      state = MulMod(state, kMinstdA);
      const int d = Draw(state, r[e] + 1u);
      if (d == 2) atomicMin(&report->first_rejected, static_cast<uint32_t>(j));
      ok[j] = d == 1;
    }
    ++pos;
  }
}

__global__ void __launch_bounds__(kVflThreads)
vfl_pick(const uint32_t* __restrict__ sorted_idx, const uint32_t* __restrict__ head,
         const uint8_t* __restrict__ ok, int n, int32_t* __restrict__ best) {
  const int s = blockIdx.x * kVflThreads + threadIdx.x;
  if (s >= n) return;
  const uint32_t h = head[s];
  if (h == static_cast<uint32_t>(s) || ok[sorted_idx[s]]) atomicMax(&best[h], s);
}

__global__ void __launch_bounds__(kVflThreads)
vfl_mask(const uint32_t* __restrict__ sorted_idx, const uint32_t* __restrict__ head,
         const int32_t* __restrict__ best, int n, uint8_t* __restrict__ keep,
         VflReport* __restrict__ report) {
  const int s = blockIdx.x * kVflThreads + threadIdx.x;
  bool kept = false;
  if (s < n) {
    kept = best[head[s]] == s;
    keep[sorted_idx[s]] = kept;
  }
  const unsigned long long b = __ballot(kept);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&report->kept, __popcll(b));
}

__global__ void __launch_bounds__(kVflThreads)
vfl_range_mask(const float* __restrict__ xyz, int n, float max_range, uint8_t* __restrict__ sel) {
  const int i = blockIdx.x * kVflThreads + threadIdx.x;
  if (i >= n) return;
  const size_t at = 3 * static_cast<size_t>(i);
  sel[i] = VfWithinRange(xyz[at], xyz[at + 1], xyz[at + 2], max_range);
}

__global__ void __launch_bounds__(kVflThreads)
vfl_sel_counts(const uint8_t* __restrict__ sel, uint8_t want, int n,
               uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t tmp[kVflThreads / 64];
  const int i0 = blockIdx.x * kVflTile + static_cast<int>(threadIdx.x) * kVflPer;
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < kVflPer; ++e)
    if (i0 + e < n && sel[i0 + e] == want) ++c;
  uint32_t total = 0;
  (void)BlockExclusiveSum(c, &total, tmp);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kVflThreads)
vfl_compact(const uint8_t* __restrict__ sel, uint8_t want, int n,
            const uint32_t* __restrict__ tile_counts, const float* __restrict__ xyz,
            const float* __restrict__ intensities, float* __restrict__ out_xyz,
            float* __restrict__ out_intensities, uint32_t* __restrict__ index_out,
            int32_t* __restrict__ count) {
  __shared__ uint32_t tmp[kVflThreads / 64];
  const int i0 = blockIdx.x * kVflTile + static_cast<int>(threadIdx.x) * kVflPer;
  uint32_t picked = 0, c = 0;
#pragma unroll
  for (int e = 0; e < kVflPer; ++e)
    if (i0 + e < n && sel[i0 + e] == want) {
      picked |= 1u << e;
      ++c;
    }
  const uint32_t before = TilesBefore(tile_counts, tmp);
  uint32_t total = 0;
  uint32_t pos = before + BlockExclusiveSum(c, &total, tmp);  // pos + c <= n
#pragma unroll
  for (int e = 0; e < kVflPer; ++e) {
    if (!(picked & (1u << e))) continue;
    const size_t from = 3 * static_cast<size_t>(i0 + e), to = 3 * static_cast<size_t>(pos);
    out_xyz[to] = xyz[from];
    out_xyz[to + 1] = xyz[from + 1];
    out_xyz[to + 2] = xyz[from + 2];
    if (intensities) out_intensities[pos] = intensities[i0 + e];
    if (index_out) index_out[pos] = static_cast<uint32_t>(i0 + e);
    ++pos;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = static_cast<int32_t>(before + total);
}

__global__ void __launch_bounds__(kVflThreads)
vfl_scatter_mask(const uint8_t* __restrict__ res, const uint32_t* __restrict__ index, int m,
                 uint8_t* __restrict__ keep) {
  const int j = blockIdx.x * kVflThreads + threadIdx.x;
  if (j < m) keep[index[j]] = res[j];
}

unsigned BlocksOf(int n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

// Reads `bytes` at d_src back through the pinned words and waits.
int ReadBack(csm_context* ctx, const void* d_src, void* dst, size_t bytes) {
  CSM_HIP(hipMemcpyAsync(ctx->vfl_rb.ptr, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  CSM_HIP(hipStreamSynchronize(ctx->stream));
  std::memcpy(dst, ctx->vfl_rb.ptr, bytes);
  return CSM_OK;
}

// vfl_pick and vfl_mask after a draw pass, and its report.
int PickAndReport(csm_context* ctx, const VflWork& w, int n, uint8_t* d_keep, VflReport* out) {
  hipStream_t st = ctx->stream;
  const unsigned blocks = BlocksOf(n, kVflThreads);
  hipLaunchKernelGGL(vfl_pick, dim3(blocks), dim3(kVflThreads), 0, st, w.sorted_idx, w.head, w.ok,
                     n, w.best);
  hipLaunchKernelGGL(vfl_mask, dim3(blocks), dim3(kVflThreads), 0, st, w.sorted_idx, w.head,
                     w.best, n, d_keep, w.report);
  CSM_HIP(hipGetLastError());
  return ReadBack(ctx, w.report, out, sizeof(*out));
}

// One VoxelFilter of the n > 0 points at d_xyz (working memory reserved).
int FilterPass(csm_context* ctx, const VflWork& w, const float* d_xyz, int n, float resolution,
               uint8_t* d_keep, int32_t* kept) {
  hipStream_t st = ctx->stream;
  const unsigned blocks = BlocksOf(n, kVflThreads), tiles = BlocksOf(n, kVflTile);
  hipLaunchKernelGGL(vfl_keys, dim3(blocks), dim3(kVflThreads), 0, st, d_xyz, n, resolution,
                     w.keys, w.idx, w.report);
  CSM_HIP(hipGetLastError());
  // The sort's scratch for this size (a host-side query; the sort picks its
  // method by size, so a smaller cloud need not need less).
  size_t scratch = 0;
  CSM_HIP(rocprim::radix_sort_pairs(nullptr, scratch, w.keys, w.sorted_keys, w.idx, w.sorted_idx,
                                    static_cast<unsigned>(n), 0u, 64u, st));
  if (scratch > ctx->vfl_sort.bytes) {
    CSM_HIP(hipStreamSynchronize(st));
    int rc = ctx->vfl_sort.Reserve(scratch);
    if (rc) return rc;
  }
  scratch = ctx->vfl_sort.bytes;
  CSM_HIP(rocprim::radix_sort_pairs(ctx->vfl_sort.ptr, scratch, w.keys, w.sorted_keys, w.idx,
                                    w.sorted_idx, static_cast<unsigned>(n), 0u, 64u, st));
  hipLaunchKernelGGL(vfl_ranks, dim3(tiles), dim3(kVflThreads), 0, st, w.sorted_keys, w.sorted_idx,
                     n, w.head, w.rank);
  hipLaunchKernelGGL(vfl_draw_counts, dim3(tiles), dim3(kVflThreads), 0, st, w.rank, n,
                     w.tile_counts);
  hipLaunchKernelGGL(vfl_draw, dim3(tiles), dim3(kVflThreads), 0, st, w.rank, n, w.tile_counts, 0,
                     0u, w.ok, w.best, w.report);
  CSM_HIP(hipGetLastError());
  VflReport report;
  int rc;
  if ((rc = PickAndReport(ctx, w, n, d_keep, &report))) return rc;
  uint32_t shift = 0;
  while (report.first_rejected != kNoRejection) {
    // The draws before this point stand; from it on the stream is one further.
    if (report.first_rejected >= static_cast<uint32_t>(n)) return CSM_EHIP;
    ++shift;
    hipLaunchKernelGGL(vfl_reset_report, dim3(1), dim3(1), 0, st, w.report);
    hipLaunchKernelGGL(vfl_draw, dim3(tiles), dim3(kVflThreads), 0, st, w.rank, n, w.tile_counts,
                       static_cast<int>(report.first_rejected), shift, w.ok, w.best, w.report);
    CSM_HIP(hipGetLastError());
    if ((rc = PickAndReport(ctx, w, n, d_keep, &report))) return rc;
  }
  if (report.kept < 0 || report.kept > n) return CSM_EHIP;
  *kept = report.kept;
  return CSM_OK;
}

VflWork WorkOf(csm_context* ctx) {
  return VflWork(ctx->vfl_work.as<char>(), static_cast<size_t>(ctx->vfl_capacity));
}

// The host entry points' shared body: upload, filter, download.
int HostFilterLarge(csm_context* ctx, const float* xyz, int64_t n,
                    const csm_adaptive_voxel_filter_options* adaptive, float resolution,
                    uint8_t* keep, int64_t* count) {
  if (!ctx || n < 0 || !count) return CSM_EINVAL;
  if (n > kVflMaxPoints) return CSM_ERANGE;
  if (n == 0) {
    *count = 0;
    return CSM_OK;
  }
  if (!xyz || !keep) return CSM_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);
  int rc;
  if ((rc = VflReserve(ctx, n))) return rc;
  const size_t np = static_cast<size_t>(n);
  if ((rc = ctx->vf_points.Reserve(12 * np))) return rc;
  if ((rc = ctx->vf_keep.Reserve(np))) return rc;
  hipStream_t st = ctx->stream;
  CSM_HIP(hipMemcpyAsync(ctx->vf_points.ptr, xyz, 12 * np, hipMemcpyHostToDevice, st));
  int32_t kept = 0;
  const int32_t n32 = static_cast<int32_t>(n);
  if (adaptive)
    rc = VflAdaptiveVoxelFilter(ctx, ctx->vf_points.as<float>(), n32, adaptive,
                                ctx->vf_keep.as<uint8_t>(), &kept);
  else
    rc = VflVoxelFilter(ctx, ctx->vf_points.as<float>(), n32, resolution,
                        ctx->vf_keep.as<uint8_t>(), &kept);
  if (rc) return rc;
  CSM_HIP(hipMemcpyAsync(keep, ctx->vf_keep.ptr, np, hipMemcpyDeviceToHost, st));
  CSM_HIP(hipStreamSynchronize(st));
  *count = kept;
  return CSM_OK;
}

}  // namespace

int VflReserve(csm_context* ctx, int64_t n) {
  if (n > kVflMaxPoints) return CSM_ERANGE;
  int rc;
  if ((rc = ctx->vfl_rb.Reserve(64))) return rc;
  if (n <= ctx->vfl_capacity) return CSM_OK;
  // Earlier work on the stream may still use the buffers about to be replaced.
  CSM_HIP(hipStreamSynchronize(ctx->stream));
  // Grow by half again, so a sequence of slowly growing sweeps reallocates rarely.
  const int64_t cap = std::min<int64_t>(kVflMaxPoints, std::max<int64_t>(n + n / 2, 16384));
  size_t need = 0;
  CSM_HIP(rocprim::radix_sort_pairs(nullptr, need, static_cast<uint64_t*>(nullptr),
                                    static_cast<uint64_t*>(nullptr),
                                    static_cast<uint32_t*>(nullptr),
                                    static_cast<uint32_t*>(nullptr), static_cast<unsigned>(cap), 0u,
                                    64u, ctx->stream));
  ctx->vfl_capacity = 0;
  if ((rc = ctx->vfl_sort.Reserve(std::max<size_t>(need, 256)))) return rc;
  if ((rc = ctx->vfl_work.Reserve(VflWork(nullptr, static_cast<size_t>(cap)).bytes))) return rc;
  if ((rc = ctx->vfl_cloud.Reserve(12 * static_cast<size_t>(cap)))) return rc;
  ctx->vfl_capacity = cap;
  return CSM_OK;
}

int VflVoxelFilter(csm_context* ctx, const float* d_xyz, int32_t n, float resolution,
                   uint8_t* d_keep, int32_t* count) {
  if (!ctx || n < 0 || !count || !(resolution > 0.f)) return CSM_EINVAL;
  *count = 0;
  if (n == 0) return CSM_OK;
  if (!d_xyz || !d_keep) return CSM_EINVAL;
  int rc;
  if ((rc = VflReserve(ctx, n))) return rc;
  return FilterPass(ctx, WorkOf(ctx), d_xyz, n, resolution, d_keep, count);
}

int VflCompact(csm_context* ctx, const uint8_t* d_sel, uint8_t want, int32_t n,
               const float* d_xyz, const float* d_intensities, float* d_out_xyz,
               float* d_out_intensities, uint32_t* d_index_out, int32_t* d_count) {
  if (!ctx || n < 0 || !d_count) return CSM_EINVAL;
  if (n == 0) {
    CSM_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), ctx->stream));
    return CSM_OK;
  }
  if (!d_sel || !d_xyz || !d_out_xyz || (d_intensities && !d_out_intensities)) return CSM_EINVAL;
  int rc;
  if ((rc = VflReserve(ctx, n))) return rc;
  const VflWork w = WorkOf(ctx);
  const unsigned tiles = BlocksOf(n, kVflTile);
  hipLaunchKernelGGL(vfl_sel_counts, dim3(tiles), dim3(kVflThreads), 0, ctx->stream, d_sel, want, n,
                     w.tile_counts);
  hipLaunchKernelGGL(vfl_compact, dim3(tiles), dim3(kVflThreads), 0, ctx->stream, d_sel, want, n,
                     w.tile_counts, d_xyz, d_intensities, d_out_xyz, d_out_intensities,
                     d_index_out, d_count);
  CSM_HIP(hipGetLastError());
  return CSM_OK;
}

int VflAdaptiveVoxelFilter(csm_context* ctx, const float* d_xyz, int32_t n,
                           const csm_adaptive_voxel_filter_options* options, uint8_t* d_keep,
                           int32_t* count) {
  if (!ctx || n < 0 || !count || !options || !(options->max_length > 0.f)) return CSM_EINVAL;
  *count = 0;
  if (n == 0) return CSM_OK;
  if (!d_xyz || !d_keep) return CSM_EINVAL;
  int rc;
  if ((rc = VflReserve(ctx, n))) return rc;
  const VflWork w = WorkOf(ctx);
  hipStream_t st = ctx->stream;
  float* cloud = ctx->vfl_cloud.as<float>();
  // FilterByMaxRange: the cloud the search filters, and where its points came from.
  hipLaunchKernelGGL(vfl_range_mask, dim3(BlocksOf(n, kVflThreads)), dim3(kVflThreads), 0, st,
                     d_xyz, n, options->max_range, w.sel);
  CSM_HIP(hipGetLastError());
  if ((rc = VflCompact(ctx, w.sel, 1, n, d_xyz, nullptr, cloud, nullptr, w.index, w.count)))
    return rc;
  int32_t m = 0;
  if ((rc = ReadBack(ctx, w.count, &m, sizeof(m)))) return rc;
  if (m < 0 || m > n) return CSM_EHIP;
  CSM_HIP(hipMemsetAsync(d_keep, 0, static_cast<size_t>(n), st));
  if (m == 0) return CSM_OK;
  uint8_t *cur = w.cur, *res = w.res;
  int32_t kept = m;
  if (static_cast<float>(m) <= options->min_num_points) {
    CSM_HIP(hipMemsetAsync(res, 1, static_cast<size_t>(m), st));  // already sparse enough
  } else {
    VfLengthSearch search(options->max_length, options->min_num_points);
    while (!search.Done()) {
      int32_t cand = 0;
      if ((rc = FilterPass(ctx, w, cloud, m, search.Length(), cur, &cand))) return rc;
      if (search.Step(cand)) {
        kept = cand;
        std::swap(cur, res);
      }
    }
  }
  hipLaunchKernelGGL(vfl_scatter_mask, dim3(BlocksOf(m, kVflThreads)), dim3(kVflThreads), 0, st,
                     res, w.index, m, d_keep);
  CSM_HIP(hipGetLastError());
  *count = kept;
  return CSM_OK;
}

}  // namespace csm

extern "C" {

int csm_voxel_filter_large(csm_context* ctx, const float* xyz, int64_t n, float resolution,
                           uint8_t* keep, int64_t* count) {
  if (!(resolution > 0.f)) return CSM_EINVAL;
  return csm::HostFilterLarge(ctx, xyz, n, nullptr, resolution, keep, count);
}

int csm_adaptive_voxel_filter_large(csm_context* ctx, const float* xyz, int64_t n,
                                    const csm_adaptive_voxel_filter_options* options,
                                    uint8_t* keep, int64_t* count) {
  if (!options || !(options->max_length > 0.f)) return CSM_EINVAL;
  return csm::HostFilterLarge(ctx, xyz, n, options, 0.f, keep, count);
}

}  // extern "C"
