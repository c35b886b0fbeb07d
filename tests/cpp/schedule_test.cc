// The v4/v5 search kernel's interleaved work queues (csm_schedule.h
// BuildSchedule, csm_device.h DecodeSlot): on random ragged batches every
// (pair, chunk) is decoded from exactly one slot, the empty slots are as many
// as the builder reports and at most 1 % of the items per block, a
// rectangle's rows are `width` slots apart, and the golden-section order
// leaves no large gap on the circle of a pair's chunks. Built with
// -fsanitize=address,undefined (tests/test_schedule.py).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../cartographer-1_amd/csrc/csm_schedule.h"

namespace {

using namespace csm;

int failures = 0;
#define CHECK(cond, ...)                           \
  do {                                             \
    if (!(cond)) {                                 \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                    \
      std::printf("\n");                           \
      if (++failures > 20) std::exit(1);           \
    }                                              \
  } while (0)

void RunCase(int num_pairs, int num_submaps, int block, bool golden, bool spread, int rc,
             std::mt19937* rng) {
  // Odd rotation counts: with rc = 2 the last chunk holds one rotation.
  std::vector<int32_t> submap(num_pairs), scans(num_pairs), chunks(num_pairs);
  std::uniform_int_distribution<int> any_submap(0, num_submaps - 1), any_count(1, 2000);
  std::vector<int64_t> first(num_pairs + 1, 0);
  for (int i = 0; i < num_pairs; ++i) {
    submap[i] = i < num_submaps ? i : any_submap(*rng);  // every submap occurs when it can
    const int c = any_count(*rng);
    scans[i] = rc * c - (rc > 1 ? 1 : 0);
    chunks[i] = (scans[i] + rc - 1) / rc;
    CHECK(chunks[i] == c, "chunks");
    first[i + 1] = first[i] + chunks[i];
  }
  const auto queues = AssignQueues(submap, spread);
  Schedule s = BuildSchedule(queues, submap, chunks, rc, block, golden);
  WorkQueues2 wq = s.wq;
  wq.entries = s.entries.data();
  wq.rects = s.rects.data();
  wq.hint = s.hint.data();
  CHECK(s.items == first[num_pairs], "items %lld", static_cast<long long>(s.items));
  CHECK(static_cast<int>(s.entries.size()) == num_pairs, "entries");
  std::vector<uint8_t> seen(first[num_pairs], 0);
  int64_t empty = 0, slots = 0;
  for (int q = 0; q < kNumXcd; ++q) {
    CHECK(static_cast<size_t>(wq.hint_offset[q]) + ((wq.queue_slots[q] + (int64_t{1} << wq.hint_shift) - 1) >> wq.hint_shift) <= s.hint.size(), "hint table");
    for (int64_t slot = 0; slot < wq.queue_slots[q]; ++slot) {
      int pair = -1, chunk = -1;
      ++slots;
      if (!DecodeSlot(wq, q, slot, &pair, &chunk)) {
        ++empty;
        continue;
      }
      CHECK(pair >= 0 && pair < num_pairs, "pair %d", pair);
      if (pair < 0 || pair >= num_pairs) continue;
      CHECK(chunk >= 0 && chunk < chunks[pair], "chunk %d of pair %d", chunk, pair);
      if (chunk < 0 || chunk >= chunks[pair]) continue;
      CHECK(chunk * rc < scans[pair], "rotation past the pair's");
      CHECK(spread && num_submaps < kNumXcd ? q % num_submaps == submap[pair] && q < kNumXcd / num_submaps * num_submaps
                                            : q == submap[pair] % kNumXcd,
            "pair %d of submap %d on queue %d", pair, submap[pair], q);
      CHECK(!seen[first[pair] + chunk], "pair %d chunk %d twice", pair, chunk);
      seen[first[pair] + chunk] = 1;
    }
  }
  for (int i = 0; i < num_pairs; ++i)
    for (int c = 0; c < chunks[i]; ++c) CHECK(seen[first[i] + c], "pair %d chunk %d never", i, c);
  CHECK(empty == s.empty_slots, "empty slots %lld, reported %lld", static_cast<long long>(empty),
        static_cast<long long>(s.empty_slots));
  CHECK(slots == s.items + s.empty_slots, "slots");
  CHECK(empty * 100 <= s.items, "%lld empty slots of %lld items", static_cast<long long>(empty),
        static_cast<long long>(s.items));
  // Rectangles: contiguous per queue, no wider than a block, entries of one submap.
  for (const SchedRect& r : s.rects) {
    CHECK(r.width >= 1 && r.width <= block, "width %d", r.width);
    CHECK(r.slot_end > r.slot_begin && (r.slot_end - r.slot_begin) % r.width == 0, "rows");
    CHECK(r.slot_end - r.slot_begin < (int64_t{1} << 31), "32-bit slots");
    for (int k = 1; k < r.width; ++k)
      CHECK(submap[s.entries[r.first + k].pair] == submap[s.entries[r.first].pair], "submaps mixed");
  }
}

// Position j -> chunk j * stride mod n: a permutation whose first j chunks
// leave no circular gap above 4 n / j (the golden section's three distances
// stay within a factor 2.62 of n / j; the rounding to a coprime stride costs
// the rest).
void CheckGolden(int n) {
  const int s = GoldenStride(n);
  CHECK(s >= 1 && (n == 1 || s < n) && std::gcd(s, n) == 1, "stride %d of %d", s, n);
  std::vector<uint8_t> on(n, 0);
  int next_check = 4;
  for (int j = 0; j < n; ++j) {
    const int c = static_cast<int>(static_cast<uint32_t>(j) * static_cast<uint32_t>(s) % static_cast<uint32_t>(n));
    CHECK(!on[c], "not a permutation");
    on[c] = 1;
    if (j + 1 == next_check) {
      next_check *= 2;
      int gap = 0, run = 0, lead = -1;
      for (int c2 = 0; c2 < n; ++c2) {
        if (on[c2]) {
          if (lead < 0) lead = run;
          gap = std::max(gap, run + 1);
          run = 0;
        } else {
          ++run;
        }
      }
      gap = std::max(gap, run + lead + 1);  // across the wrap
      CHECK(gap <= (4 * n + j) / (j + 1) + 1, "n %d stride %d: gap %d after %d", n, s, gap, j + 1);
    }
  }
}

}  // namespace

int main() {
  std::mt19937 rng(20250127);
  for (int n = 1; n <= 2000; ++n) CheckGolden(n);
  CheckGolden(kMaxRotations);
  for (int block : {CSM_SCHED_BLOCK, 8})
    for (int submaps : {1, 3, 8, 11})
      for (int pairs : {1, block - 1, block, block + 1, 3 * block + 5})
        for (int golden = 0; golden < 2; ++golden) {
          if (pairs < 1) continue;
          RunCase(pairs, submaps, block, golden != 0, true, 2, &rng);
        }
  // Full blocks of every submap; no spreading; one and three rotations per item.
  RunCase(11 * (3 * 8 + 5), 11, 8, true, true, 2, &rng);
  RunCase(3 * (CSM_SCHED_BLOCK + 1), 3, CSM_SCHED_BLOCK, true, false, 2, &rng);
  RunCase(40, 3, 8, true, true, 1, &rng);
  RunCase(40, 8, 8, false, true, 3, &rng);
  if (failures) return 1;
  std::printf("schedule OK\n");
  return 0;
}
