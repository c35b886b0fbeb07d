// Which of a pair's exactly tied maximal leaves the reference's depth-first
// search reaches first: the decision of ResolveTies (csm_host.cc) and
// ResolveTies3d (host3d.cc), once for both, with no device type in it;
// tests/cpp/tie_order_test.cc checks it against a model of that search.
//
// The reference keeps the FIRST maximal leaf it visits: std::max keeps the
// incumbent on equal scores and later subtrees whose bound does not exceed it
// are cut (fast_correlative_scan_matcher_2d.cc:344-376, _3d.cc:377-440; in 3D
// a leaf also has to pass the low-resolution check, :384-401, so only passing
// leaves are given here). So among tied leaves the pick is the one whose chain
// of ancestors, lowest resolution first, comes first in the orders below.
#pragma once

#include <algorithm>
#include <cstdint>
#include <tuple>
#include <utility>
#include <vector>

#include "parallel_sort.h"

namespace csm {

// One entry of a tied leaf's chain of ancestors: rotation (2D) or yaw (3D),
// cell offsets (z = 0 in 2D) and the float score the reference compares.
struct TieNode {
  int32_t rot, x, y, z;
  float score;
};
inline bool SameNode(const TieNode& a, const TieNode& b) {
  return a.rot == b.rot && a.x == b.x && a.y == b.y && a.z == b.z;
}

// The chains of one pair's tied leaves, level 0 (the leaf; its score is never
// compared, all leaves tie) to level T (the lowest resolution).
struct TieChains {
  int T = 0;
  std::vector<TieNode> nodes;  // (T + 1) per leaf
  int count() const { return static_cast<int>(nodes.size()) / (T + 1); }
  TieNode& at(int leaf, int level) { return nodes[static_cast<size_t>(leaf) * (T + 1) + level]; }
  const TieNode& at(int leaf, int level) const { return const_cast<TieChains*>(this)->at(leaf, level); }
  // Appends a leaf with its ancestors, scores 0: the level-l one is the leaf's
  // offsets from its search box's corner `lo` rounded down to 2^l.
  void AddLeaf(int rot, int x, int y, int z, int lo_x, int lo_y, int lo_z) {
    for (int l = 0; l <= T; ++l)
      nodes.push_back(TieNode{rot, lo_x + (((x - lo_x) >> l) << l), lo_y + (((y - lo_y) >> l) << l),
                              lo_z + (((z - lo_z) >> l) << l), 0.f});
  }
};

// Siblings of one parent in generation order: 2D generates x, then y
// (_2d.cc:353-366); 3D z, then y, then x with x fastest (_3d.cc:412-430).
inline bool SiblingsXY(const TieNode& a, const TieNode& b) {
  return std::tie(a.x, a.y) < std::tie(b.x, b.y);
}
inline bool SiblingsZYX(const TieNode& a, const TieNode& b) {
  return std::tie(a.z, a.y, a.x) < std::tie(b.z, b.y, b.x);
}

// A pair's lowest-resolution list in generation order: per rotation (2D) or
// yaw (3D) a box of offsets walked in steps of 2^T by three nested loops. 2D
// (GenerateLowestResolutionCandidates, _2d.cc:276-312) loops x, then y over
// the rotation's own ShrinkToFit bounds; 3D (_3d.cc:297-330) z, then y, then x
// over +-wz, +-wxy. Index and Node are each other's inverse.
struct TopLattice {
  struct Box { int lo[3], hi[3]; };  // x, y, z (0 in 2D), inclusive
  int step, axis[3];  // the loops' axes, outermost first
  std::vector<Box> boxes;
  std::vector<int64_t> first = {0};  // per rotation its first index; back() = size
  TopLattice(int T, bool three_d) : step(1 << T), axis{2, three_d ? 1 : 0, three_d ? 0 : 1} {}
  int Count(const Box& b, int a) const { return b.hi[a] < b.lo[a] ? 0 : (b.hi[a] - b.lo[a]) / step + 1; }
  void AddRotation(const Box& b) {
    boxes.push_back(b);
    first.push_back(first.back() + static_cast<int64_t>(Count(b, 0)) * Count(b, 1) * Count(b, 2));
  }
  int64_t size() const { return first.back(); }
  template <typename Fn>
  void ForEachOfRotation(int r, Fn fn) const {  // fn(x, y, z)
    const Box b = boxes[r];
    for (int z = b.lo[2]; z <= b.hi[2]; z += step)
      if (axis[1] == 0) {
        for (int x = b.lo[0]; x <= b.hi[0]; x += step)
          for (int y = b.lo[1]; y <= b.hi[1]; y += step) fn(x, y, z);
      } else {
        for (int y = b.lo[1]; y <= b.hi[1]; y += step)
          for (int x = b.lo[0]; x <= b.hi[0]; x += step) fn(x, y, z);
      }
  }
  int64_t Index(const TieNode& n) const {
    const Box& b = boxes[n.rot];
    const int c[3] = {n.x, n.y, n.z};
    int64_t i = 0;
    for (const int a : axis) i = i * Count(b, a) + (c[a] - b.lo[a]) / step;
    return first[n.rot] + i;
  }
  TieNode Node(int64_t i) const {  // score 0
    const int r = static_cast<int>(std::upper_bound(first.begin(), first.end(), i) - first.begin()) - 1;
    const Box& b = boxes[r];
    int c[3];
    i -= first[r];
    for (int k = 2; k >= 0; i /= Count(b, axis[k]), --k)
      c[axis[k]] = b.lo[axis[k]] + static_cast<int>(i % Count(b, axis[k])) * step;
    return TieNode{r, c[0], c[1], c[2], 0.f};
  }
};

// The order the reference's ScoreCandidates leaves a lowest-resolution list
// of n candidates in: std::sort(greater<Candidate>) (an introsort, not stable)
// on the generation order (_2d.cc:331-332, _3d.cc:353-354). score_at(i) is the
// score of generation index i. The same algorithm and comparisons give the
// same permutation for any element type, so 8-byte (score, index) elements
// are sorted; IntroSort is that algorithm with independent partitions on
// `threads` threads.
struct TopOrder {
  std::vector<int32_t> order;  // sorted position -> generation index
  std::vector<int32_t> pos;    // generation index -> sorted position
};
template <typename ScoreAt>
TopOrder TopListOrder(int64_t n, ScoreAt score_at, int threads) {
  std::vector<std::pair<float, int32_t>> lst(n);
  ParallelRanges(n, threads, [&](std::ptrdiff_t lo, std::ptrdiff_t hi) {
    for (std::ptrdiff_t i = lo; i < hi; ++i) lst[i] = {score_at(i), static_cast<int32_t>(i)};
  });
  using Entry = std::pair<float, int32_t>;
  IntroSort(lst.data(), lst.data() + n, [](const Entry& a, const Entry& b) { return a.first > b.first; },
            threads);
  TopOrder o{std::vector<int32_t>(n), std::vector<int32_t>(n)};
  ParallelRanges(n, threads, [&](std::ptrdiff_t lo, std::ptrdiff_t hi) {
    for (std::ptrdiff_t i = lo; i < hi; ++i) {
      o.order[i] = lst[i].second;
      o.pos[lst[i].second] = static_cast<int32_t>(i);
    }
  });
  return o;
}

// A pair's whole lowest-resolution list: its lattice, the nodes' integer sums
// in generation order and the reference's order of their scores.
struct TopList {
  TopLattice lat;
  std::vector<int32_t> sums;
  TopOrder ord;
  int32_t Pos(const TieNode& n) const { return ord.pos[lat.Index(n)]; }
};

// The leaves that can come first. The reference visits the lowest-resolution
// candidates by descending score, so only leaves under a level-T ancestor of
// the highest score compete; the sorted top list is needed (need_perm) only
// when two distinct such ancestors share that score. At T = 0 the top list is
// the leaves themselves: all are live and the list is needed.
struct Live {
  std::vector<int> leaves;
  bool need_perm = false;
};
inline Live LiveLeaves(const TieChains& c) {
  Live live{{}, c.T == 0};
  const int n = c.count();
  float top = 0.f;
  for (int i = 0; i < n; ++i)
    if (i == 0 || c.at(i, c.T).score > top) top = c.at(i, c.T).score;
  for (int i = 0; i < n; ++i) {
    if (c.T > 0 && c.at(i, c.T).score != top) continue;
    if (!live.leaves.empty() && !SameNode(c.at(i, c.T), c.at(live.leaves[0], c.T))) live.need_perm = true;
    live.leaves.push_back(i);
  }
  return live;
}

// The leaf among `live` that the reference visits first. Two leaves part at
// the highest level where their ancestors differ. There the higher score
// goes first (children are visited by descending score); on equal scores, at
// level T the position top_pos(node) in the sorted top list decides (called
// only when need_perm), and below it the siblings' generation order
// (std::sort on <= 8 children is an insertion sort: stable).
template <typename TopPos, typename SiblingBefore>
int FirstVisitedLeaf(const TieChains& c, const std::vector<int>& live, TopPos top_pos,
                     SiblingBefore sibling_before) {
  auto first = [&](int a, int b) {
    for (int l = c.T; l >= 0; --l) {
      const TieNode &x = c.at(a, l), &y = c.at(b, l);
      if (SameNode(x, y)) continue;
      if (l > 0 && x.score != y.score) return x.score > y.score;
      if (l == c.T) return top_pos(x) < top_pos(y);
      return sibling_before(x, y);
    }
    return false;
  };
  int best = live[0];
  for (size_t i = 1; i < live.size(); ++i)
    if (first(live[i], best)) best = live[i];
  return best;
}

}  // namespace csm
