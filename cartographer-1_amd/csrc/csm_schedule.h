// Host side of the v4/v5 search kernel's work queues (csm_device.h
// WorkQueues2, DESIGN.md §5 "Rotation chunks"): which queue a pair goes to,
// and the interleaved order of a queue's (pair, rotation chunk) items. Plain
// C++ so that a stand-alone program can check it (tests/cpp/schedule_test.cc).
#ifndef CSM_SCHEDULE_H_
#define CSM_SCHEDULE_H_

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <numeric>
#include <vector>

#include "csm_device.h"

#ifndef CSM_SCHED_BLOCK
// Pairs per block: consecutive positions of a pair are this many claims
// apart, so at least the workgroups that serve one queue (grid / 8, 192 on
// MI355X at 6 per CU). EXPERIMENTS.md "Interleaved rotation chunks".
#define CSM_SCHED_BLOCK 256
#endif
#ifndef CSM_SCHED_GOLDEN
// 1: position j of a pair is chunk j * stride mod chunks, stride near
// 0.618 chunks; 0: chunk j (the A/B alternative).
#define CSM_SCHED_GOLDEN 1
#endif

namespace csm {

// Per-XCD queues: submap s -> queue s % 8 so a submap's pyramid stays in one
// XCD's L2; pairs within a queue in submap order. With spreading, a batch of
// fewer than 8 submaps (the C3 chunks hold 4) puts each submap's pairs on
// 8 / S queues, so every XCD starts on a submap of its own instead of the
// empty queues' workgroups all stealing from the first one: C3 chunk launch
// 591 -> 570 ms (profiles/r4o/).
inline std::vector<std::vector<int32_t>> AssignQueues(const std::vector<int32_t>& submap,
                                                      bool spread) {
  const int np = static_cast<int>(submap.size());
  int nsub = 0;
  for (int i = 0; i < np; ++i) nsub = std::max(nsub, submap[i] + 1);
  const int reps = spread && nsub > 0 && nsub < kNumXcd ? kNumXcd / nsub : 1;
  std::vector<int32_t> seen(reps > 1 ? nsub : 0, 0);
  std::vector<std::vector<int32_t>> q(kNumXcd);
  for (int i = 0; i < np; ++i) {
    const int sm = submap[i];
    const int qi = reps > 1 ? sm + nsub * (seen[sm]++ % reps) : sm % kNumXcd;
    q[qi].push_back(i);
  }
  for (auto& v : q)
    std::stable_sort(v.begin(), v.end(), [&](int a, int b) { return submap[a] < submap[b]; });
  return q;
}

// A stride coprime to `chunks` near 0.618 chunks: j * stride mod chunks,
// j = 0, 1, ..., then leaves gaps of about chunks / j everywhere on the
// circle (three-distance theorem). The gaps' spread follows the partial
// quotients of stride / chunks' continued fraction (the golden section: all
// 1), and the coprime number nearest to 0.618 chunks can have a large one
// (219 / 350 = [0; 1, 1, 1, 2, 21, 2]), so among the coprime strides within 8
// of it the one with the smallest largest quotient is taken, then the nearest.
inline int32_t GoldenStrideSearch(int32_t chunks) {
  if (chunks <= 2) return 1;
  const int32_t s0 = static_cast<int32_t>(chunks * 0.6180339887498949 + 0.5);
  int32_t best = 1, best_q = chunks + 1;
  for (int32_t d = 0; d <= 8; ++d)
    for (int32_t s : {s0 + d, s0 - d}) {
      if (s < 1 || s >= chunks) continue;
      int32_t a = chunks, b = s, q = 0;
      while (b > 0) {
        q = std::max(q, a / b);
        const int32_t r = a % b;
        a = b;
        b = r;
      }
      if (a == 1 && q < best_q) best = s, best_q = q;  // a = gcd(chunks, s)
    }
  return best;
}
inline int32_t GoldenStride(int32_t chunks) {
  static const std::vector<int32_t> table = [] {
    std::vector<int32_t> t(kMaxRotations + 1);
    for (int32_t n = 0; n <= kMaxRotations; ++n) t[n] = GoldenStrideSearch(n);
    return t;
  }();
  return chunks >= 0 && chunks <= kMaxRotations ? table[chunks] : GoldenStrideSearch(chunks);
}

struct Schedule {
  std::vector<SchedEntry> entries;
  std::vector<SchedRect> rects;
  std::vector<int32_t> hint;
  WorkQueues2 wq{};  // the three pointers are left null
  int64_t items = 0;        // (pair, chunk) items
  int64_t empty_slots = 0;  // slots of all queues - items
};

// Cuts a block (chunk counts c[0..n), descending) into rectangles: the next
// one spans the pairs still unfinished and ends at one of their counts, the
// largest at which it holds at most `cap` empty slots. Returns the empty slots.
inline int64_t CutBlock(const int32_t* c, int n, int64_t cap, int32_t first, int64_t* slot,
                        std::vector<SchedRect>* out) {
  int64_t empty = 0;
  int32_t pos = 0;
  for (;;) {
    while (n > 0 && c[n - 1] <= pos) --n;  // finished pairs
    if (n == 0) break;
    int m = n - 1;
    int64_t waste = 0;
    while (m > 0) {
      const int64_t more = waste + static_cast<int64_t>(n - m) * (c[m - 1] - c[m]);
      if (more > cap) break;
      waste = more;
      --m;
    }
    const int32_t top = c[m];
    if (out) {
      SchedRect r{};
      r.slot_begin = *slot;
      r.slot_end = *slot + static_cast<int64_t>(n) * (top - pos);
      r.first = first;
      r.width = n;
      r.pos0 = pos;
      out->push_back(r);
      *slot = r.slot_end;
    }
    empty += waste;
    pos = top;
  }
  return empty;
}

// queues: AssignQueues' result; chunks: per pair (0: no item). A block's empty slots
// stay within 1 % of its items.
inline Schedule BuildSchedule(const std::vector<std::vector<int32_t>>& queues,
                              const std::vector<int32_t>& submap,
                              const std::vector<int32_t>& chunks, int rot_chunk,
                              int block_pairs = CSM_SCHED_BLOCK, bool golden = CSM_SCHED_GOLDEN) {
  Schedule s;
  s.wq.rot_chunk = rot_chunk;
  block_pairs = std::max(1, std::min(block_pairs, 1 << 16));  // a rectangle: < 2^31 slots
  std::vector<int32_t> run, counts;
  std::vector<int32_t> queue_rect_begin(kNumXcd + 1, 0);
  int64_t max_slots = 0;
  for (int x = 0; x < kNumXcd; ++x) {
    queue_rect_begin[x] = static_cast<int32_t>(s.rects.size());
    const std::vector<int32_t>& q = queues[x];
    int64_t slot = 0;
    for (size_t b = 0; b < q.size();) {
      size_t e = b;
      while (e < q.size() && submap[q[e]] == submap[q[b]]) ++e;
      run.assign(q.begin() + b, q.begin() + e);
      std::stable_sort(run.begin(), run.end(),
                       [&](int a, int c) { return chunks[a] > chunks[c]; });
      for (size_t k = 0; k < run.size(); k += block_pairs) {
        const int n = static_cast<int>(std::min<size_t>(block_pairs, run.size() - k));
        const int32_t first = static_cast<int32_t>(s.entries.size());
        counts.clear();
        int64_t items = 0;
        for (int i = 0; i < n; ++i) {
          const int32_t pair = run[k + i], c = chunks[pair];
          s.entries.push_back(SchedEntry{pair, c, golden ? GoldenStride(c) : 1, 0});
          counts.push_back(c);
          items += c;
        }
        // Fewer, larger rectangles first; halve the cap until the block's
        // empty slots fit (cap 0: one rectangle per distinct count, none empty).
        const int64_t budget = items / 100;
        int64_t cap = budget;
        while (CutBlock(counts.data(), n, cap, first, nullptr, nullptr) > budget) cap /= 2;
        s.empty_slots += CutBlock(counts.data(), n, cap, first, &slot, &s.rects);
        s.items += items;
      }
      b = e;
    }
    s.wq.queue_slots[x] = slot;
    max_slots = std::max(max_slots, slot);
  }
  queue_rect_begin[kNumXcd] = static_cast<int32_t>(s.rects.size());
  // Hints: at most 1024 per queue, at least 64 slots each.
  int shift = 6;
  while ((max_slots >> shift) >= 1024) ++shift;
  s.wq.hint_shift = shift;
  for (int x = 0; x < kNumXcd; ++x) {
    s.wq.hint_offset[x] = static_cast<int32_t>(s.hint.size());
    int r = queue_rect_begin[x];
    for (int64_t at = 0; at < s.wq.queue_slots[x]; at += int64_t{1} << shift) {
      while (s.rects[r].slot_end <= at) ++r;
      s.hint.push_back(r);
    }
  }
  return s;
}

}  // namespace csm

#endif  // CSM_SCHEDULE_H_
