// tie_order.h against a brute-force model of the reference's branch-and-bound
// search, on random 2D and 3D trees with dense exact ties. The model is
// written from DESIGN.md's "Exactly tied maxima": lowest-resolution
// candidates in generation order ((rotation, x, y) in 2D, (yaw, z, y, x) in
// 3D) sorted with std::sort(greater); each node's children in generation
// order, stably sorted by descending score; the incumbent kept on equal
// scores; a subtree whose bound does not exceed it cut; in 3D a leaf also has
// to pass the low-resolution check, and the first passing child at depth 0
// wins. The header gets only the passing leaves at the maximum and has to
// name the model's leaf.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../cartographer-1_amd/csrc/tie_order.h"

namespace {

using csm::TieNode;

std::mt19937 rng(20261021u);
int Rand(int lo, int hi) { return lo + static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)); }

struct Cell {
  int r, x, y, z;
  float score;
  bool operator>(const Cell& o) const { return score > o.score; }
};

// One pair's search tree: per rotation an inclusive box of leaf offsets
// (z = 0 in 2D), per level the nodes' scores (the maximum over their leaves,
// so a valid bound), per leaf the pass bit.
struct World {
  int dim = 2, T = 0;
  struct Rot {
    int lo[3], hi[3];
    std::vector<std::vector<float>> score;  // [level], flat over the level's lattice
    std::vector<uint8_t> pass;              // leaves
    int n(int l, int a) const { return ((hi[a] - lo[a]) >> l) + 1; }
    size_t at(int l, int x, int y, int z) const {
      return (static_cast<size_t>((z - lo[2]) >> l) * n(l, 1) + ((y - lo[1]) >> l)) * n(l, 0) + ((x - lo[0]) >> l);
    }
  };
  std::vector<Rot> rots;
  float Score(int l, const Cell& c) const { return rots[c.r].score[l][rots[c.r].at(l, c.x, c.y, c.z)]; }
  bool Pass(const Cell& c) const { return rots[c.r].pass[rots[c.r].at(0, c.x, c.y, c.z)] != 0; }
  // The level-l ancestor of a leaf: offsets from the box's corner rounded down to 2^l.
  Cell Ancestor(int l, const Cell& c) const {
    const Rot& b = rots[c.r];
    Cell a{c.r, b.lo[0] + (((c.x - b.lo[0]) >> l) << l), b.lo[1] + (((c.y - b.lo[1]) >> l) << l),
           b.lo[2] + (((c.z - b.lo[2]) >> l) << l), 0.f};
    a.score = Score(l, a);
    return a;
  }
  void BuildLevels() {
    for (Rot& b : rots)
      for (int l = 1; l <= T; ++l) {
        b.score.emplace_back(static_cast<size_t>(b.n(l, 0)) * b.n(l, 1) * b.n(l, 2), -1.f);
        for (int z = b.lo[2]; z <= b.hi[2]; ++z)
          for (int y = b.lo[1]; y <= b.hi[1]; ++y)
            for (int x = b.lo[0]; x <= b.hi[0]; ++x) {
              float& s = b.score[l][b.at(l, x, y, z)];
              s = std::max(s, b.score[0][b.at(0, x, y, z)]);
            }
      }
  }
  // Generation order of the lowest-resolution list.
  std::vector<Cell> TopList() const {
    std::vector<Cell> out;
    const int step = 1 << T;
    for (int r = 0; r < static_cast<int>(rots.size()); ++r) {
      const Rot& b = rots[r];
      if (dim == 2) {
        for (int x = b.lo[0]; x <= b.hi[0]; x += step)
          for (int y = b.lo[1]; y <= b.hi[1]; y += step) out.push_back({r, x, y, 0, 0.f});
      } else {
        for (int z = b.lo[2]; z <= b.hi[2]; z += step)
          for (int y = b.lo[1]; y <= b.hi[1]; y += step)
            for (int x = b.lo[0]; x <= b.hi[0]; x += step) out.push_back({r, x, y, z, 0.f});
      }
    }
    for (Cell& c : out) c.score = Score(T, c);
    return out;
  }
  // Generation order of a level-l node's children (level l - 1).
  std::vector<Cell> Children(int l, const Cell& p) const {
    std::vector<Cell> out;
    const Rot& b = rots[p.r];
    const int h = 1 << (l - 1);
    if (dim == 2) {
      for (int dx = 0; dx <= h && p.x + dx <= b.hi[0]; dx += h)
        for (int dy = 0; dy <= h && p.y + dy <= b.hi[1]; dy += h) out.push_back({p.r, p.x + dx, p.y + dy, 0, 0.f});
    } else {
      for (int dz = 0; dz <= h && p.z + dz <= b.hi[2]; dz += h)
        for (int dy = 0; dy <= h && p.y + dy <= b.hi[1]; dy += h)
          for (int dx = 0; dx <= h && p.x + dx <= b.hi[0]; dx += h)
            out.push_back({p.r, p.x + dx, p.y + dy, p.z + dz, 0.f});
    }
    for (Cell& c : out) c.score = Score(l - 1, c);
    return out;
  }
};

// The model's search over a list of level-l nodes sorted by descending score.
void Search(const World& w, const std::vector<Cell>& list, int l, Cell* best, bool* found) {
  for (const Cell& c : list) {
    if (*found && c.score <= best->score) return;  // the incumbent stays on equal scores
    if (l == 0) {
      if (!w.Pass(c)) continue;
      *best = c;  // the first passing leaf above the incumbent
      *found = true;
      return;
    }
    std::vector<Cell> kids = w.Children(l, c);
    std::stable_sort(kids.begin(), kids.end(), std::greater<Cell>());
    Search(w, kids, l - 1, best, found);
  }
}

enum Mode { kDense, kSparse, kShadowed };

World RandomWorld(int dim, int T, Mode mode) {
  const bool sparse = mode != kDense;
  World w;
  w.dim = dim;
  w.T = T;
  const int nrot = Rand(1, 5), nvalues = Rand(2, 4);
  const int wxy = Rand(1, 9), wz = Rand(1, 9);
  for (int r = 0; r < nrot; ++r) {
    World::Rot b;
    if (dim == 2) {  // ShrinkToFit bounds: every rotation its own, 0 inside
      for (int a = 0; a < 2; ++a) b.lo[a] = -Rand(0, wxy), b.hi[a] = Rand(0, wxy);
      b.lo[2] = b.hi[2] = 0;
    } else {
      b.lo[0] = b.lo[1] = -wxy, b.hi[0] = b.hi[1] = wxy, b.lo[2] = -wz, b.hi[2] = wz;
    }
    const size_t n = static_cast<size_t>(b.n(0, 0)) * b.n(0, 1) * b.n(0, 2);
    b.score.emplace_back(n);
    b.pass.resize(n);
    // A sparse or shadowed world keeps the top value for a few planted leaves.
    for (size_t i = 0; i < n; ++i) {
      b.score[0][i] = 0.125f * static_cast<float>(3 + Rand(0, nvalues - (sparse ? 2 : 1)));
      b.pass[i] = dim == 2 || Rand(0, 9) < 7;
    }
    w.rots.push_back(b);
  }
  if (mode == kShadowed) {
    // 3D: one failing leaf at the top value next to a passing leaf at the
    // value below it. Its lowest-resolution ancestor alone has the highest
    // score, so of the many passing leaves tied at the lower value only the
    // ones under that ancestor are live, and no top list is needed.
    const int r0 = Rand(0, nrot - 1), m = (1 << T) - 1;
    World::Rot& b = w.rots[r0];
    const Cell c0{r0, Rand(b.lo[0], b.hi[0]), Rand(b.lo[1], b.hi[1]), Rand(b.lo[2], b.hi[2]), 0.f};
    Cell c = c0;
    c.x = std::min(b.hi[0], b.lo[0] + (((c0.x - b.lo[0]) & ~m) | Rand(0, m)));
    c.y = std::min(b.hi[1], b.lo[1] + (((c0.y - b.lo[1]) & ~m) | Rand(0, m)));
    c.z = std::min(b.hi[2], b.lo[2] + (((c0.z - b.lo[2]) & ~m) | Rand(0, m)));
    if (c.x != c0.x || c.y != c0.y || c.z != c0.z) {
      b.score[0][b.at(0, c0.x, c0.y, c0.z)] = 0.125f * static_cast<float>(3 + nvalues - 2);
      b.pass[b.at(0, c0.x, c0.y, c0.z)] = 1;
      b.score[0][b.at(0, c.x, c.y, c.z)] = 0.125f * static_cast<float>(3 + nvalues - 1);
      b.pass[b.at(0, c.x, c.y, c.z)] = 0;
    }
  } else if (sparse) {
    // 2-4 leaves at the top value, in one lowest-resolution block or (one
    // time in four) anywhere.
    const bool anywhere = Rand(0, 3) == 0;
    const int r0 = Rand(0, nrot - 1);
    const World::Rot& b0 = w.rots[r0];
    const Cell c0{r0, Rand(b0.lo[0], b0.hi[0]), Rand(b0.lo[1], b0.hi[1]), Rand(b0.lo[2], b0.hi[2]), 0.f};
    for (int k = Rand(2, 4); k > 0; --k) {
      Cell c = c0;
      if (anywhere) {
        c.r = Rand(0, nrot - 1);
        const World::Rot& b = w.rots[c.r];
        c.x = Rand(b.lo[0], b.hi[0]), c.y = Rand(b.lo[1], b.hi[1]), c.z = Rand(b.lo[2], b.hi[2]);
      } else if (k > 1) {  // the last one is c0 itself
        const int m = (1 << T) - 1;
        c.x = std::min(b0.hi[0], b0.lo[0] + (((c0.x - b0.lo[0]) & ~m) | Rand(0, m)));
        c.y = std::min(b0.hi[1], b0.lo[1] + (((c0.y - b0.lo[1]) & ~m) | Rand(0, m)));
        c.z = std::min(b0.hi[2], b0.lo[2] + (((c0.z - b0.lo[2]) & ~m) | Rand(0, m)));
      }
      World::Rot& b = w.rots[c.r];
      b.score[0][b.at(0, c.x, c.y, c.z)] = 0.125f * static_cast<float>(3 + nvalues - 1);
      b.pass[b.at(0, c.x, c.y, c.z)] = 1;
    }
  }
  w.BuildLevels();
  return w;
}

int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++failures <= 20) {                 \
        std::printf("FAIL %s: ", #cond);      \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

struct Counts {
  int need_perm = 0, no_perm = 0, t0 = 0, long_lists = 0;
};

void RunCase(int id, int dim, int T, Mode mode, Counts* counts) {
  const World w = RandomWorld(dim, T, mode);
  // The model.
  std::vector<Cell> top = w.TopList();
  const std::vector<Cell> generated = top;
  std::sort(top.begin(), top.end(), std::greater<Cell>());
  Cell want{};
  bool found = false;
  Search(w, top, T, &want, &found);
  if (!found) return;  // no leaf passes
  // The passing leaves at the maximum, as the collect search records them.
  std::vector<Cell> tied;
  float maximum = -1.f;
  for (int pass = 0; pass < 2; ++pass)
    for (int r = 0; r < static_cast<int>(w.rots.size()); ++r) {
      const World::Rot& b = w.rots[r];
      for (int z = b.lo[2]; z <= b.hi[2]; ++z)
        for (int y = b.lo[1]; y <= b.hi[1]; ++y)
          for (int x = b.lo[0]; x <= b.hi[0]; ++x) {
            Cell c{r, x, y, z, 0.f};
            c.score = w.Score(0, c);
            if (!w.Pass(c)) continue;
            if (pass == 0) maximum = std::max(maximum, c.score);
            else if (c.score == maximum) tied.push_back(c);
          }
    }
  CHECK(want.score == maximum, "case %d: the model stopped at %g, maximum %g", id, want.score, maximum);
  if (tied.size() < 2) return;
  std::shuffle(tied.begin(), tied.end(), rng);  // the record's order means nothing
  csm::TieChains chains;
  chains.T = T;
  for (size_t i = 0; i < tied.size(); ++i) {
    const World::Rot& b = w.rots[tied[i].r];
    chains.AddLeaf(tied[i].r, tied[i].x, tied[i].y, tied[i].z, b.lo[0], b.lo[1], b.lo[2]);
    // The level-0 score is never compared: any value must do.
    chains.at(static_cast<int>(i), 0).score = static_cast<float>(Rand(0, 99));
    for (int l = 1; l <= T; ++l) {
      const Cell a = w.Ancestor(l, tied[i]);
      TieNode& node = chains.at(static_cast<int>(i), l);
      CHECK(csm::SameNode(node, TieNode{a.r, a.x, a.y, a.z, 0.f}), "case %d: level %d ancestor of leaf %zu", id, l, i);
      node.score = a.score;
    }
  }
  CHECK(chains.count() == static_cast<int>(tied.size()), "case %d", id);
  const csm::Live live = csm::LiveLeaves(chains);
  // The header's lattice and sorted top list against the model's.
  csm::TopLattice lat(T, dim == 3);
  std::vector<float> scores;
  for (int r = 0; r < static_cast<int>(w.rots.size()); ++r) {
    const World::Rot& b = w.rots[r];
    lat.AddRotation({{b.lo[0], b.lo[1], b.lo[2]}, {b.hi[0], b.hi[1], b.hi[2]}});
    lat.ForEachOfRotation(r, [&](int x, int y, int z) {
      const size_t k = scores.size();
      CHECK(k < generated.size() && csm::SameNode(TieNode{r, x, y, z, 0.f},
                                                  TieNode{generated[k].r, generated[k].x, generated[k].y, generated[k].z, 0.f}),
            "case %d: generated entry %zu", id, k);
      scores.push_back(w.Score(T, Cell{r, x, y, z, 0.f}));
    });
  }
  const int64_t n = lat.size();
  CHECK(n == static_cast<int64_t>(generated.size()) && n == static_cast<int64_t>(scores.size()),
        "case %d: lattice of %lld, the model generates %zu", id, static_cast<long long>(n), generated.size());
  if (n != static_cast<int64_t>(generated.size())) return;
  auto index = [&](const TieNode& t) { return lat.Index(t); };
  for (int64_t i = 0; i < n; ++i) {
    const Cell& g = generated[i];
    CHECK(csm::SameNode(lat.Node(i), TieNode{g.r, g.x, g.y, g.z, 0.f}) && index(lat.Node(i)) == i && scores[i] == g.score,
          "case %d: lattice entry %lld", id, static_cast<long long>(i));
  }
  const csm::TopOrder ord = csm::TopListOrder(n, [&](int64_t i) { return scores[i]; }, 1 + id % 3);
  for (int64_t i = 0; i < n; ++i) {
    const Cell& g = generated[ord.order[i]];
    CHECK(g.r == top[i].r && g.x == top[i].x && g.y == top[i].y && g.z == top[i].z && ord.pos[ord.order[i]] == i,
          "case %d: sorted position %lld", id, static_cast<long long>(i));
  }
  // The pick. The top list's order may be asked for only when LiveLeaves
  // said it is needed.
  int stray = 0;
  auto top_pos = [&](const TieNode& t) {
    if (!live.need_perm) ++stray;
    return ord.pos[index(t)];
  };
  auto pick = [&](const std::vector<int>& among, auto pos) {
    return dim == 2 ? csm::FirstVisitedLeaf(chains, among, pos, csm::SiblingsXY)
                    : csm::FirstVisitedLeaf(chains, among, pos, csm::SiblingsZYX);
  };
  auto same = [&](int leaf) {
    const Cell& c = tied[leaf];
    return c.r == want.r && c.x == want.x && c.y == want.y && c.z == want.z;
  };
  const int got = pick(live.leaves, top_pos);
  CHECK(same(got), "case %d (%dD, T %d, %zu tied, %zu live, need_perm %d): picked (%d, %d, %d, %d), the model (%d, %d, %d, %d)",
        id, dim, T, tied.size(), live.leaves.size(), live.need_perm, tied[got].r, tied[got].x, tied[got].y,
        tied[got].z, want.r, want.x, want.y, want.z);
  CHECK(stray == 0, "case %d: top list asked for %d times without need_perm", id, stray);
  // The comparison orders any two tied leaves, live or not: over all of them
  // the pick is the same. Without need_perm the score alone separates the
  // lowest-resolution ancestors that matter, so any position will do.
  std::vector<int> all(tied.size());
  for (size_t i = 0; i < all.size(); ++i) all[i] = static_cast<int>(i);
  const int got_all = live.need_perm || T == 0
                          ? pick(all, [&](const TieNode& t) { return ord.pos[index(t)]; })
                          : pick(all, [&](const TieNode& t) { return static_cast<int32_t>((index(t) * 2654435761u) >> 7 & 0xffff); });
  CHECK(same(got_all), "case %d (%dD, T %d, need_perm %d): over all %zu tied leaves picked (%d, %d, %d, %d), the model (%d, %d, %d, %d)",
        id, dim, T, live.need_perm, tied.size(), tied[got_all].r, tied[got_all].x, tied[got_all].y, tied[got_all].z,
        want.r, want.x, want.y, want.z);
  // Whether LiveLeaves is right about the top list: two distinct
  // lowest-resolution nodes of the highest score hold a tied leaf.
  if (T == 0) {
    CHECK(live.need_perm && live.leaves.size() == tied.size(), "case %d: T = 0", id);
    ++counts->t0;
  } else {
    (live.need_perm ? counts->need_perm : counts->no_perm) += 1;
  }
  int at_top = 0;
  for (int64_t i = 0; i < n && top[i].score == top[0].score; ++i) ++at_top;
  if (n > 16 && at_top >= 3 && live.need_perm) ++counts->long_lists;
}

}  // namespace

int main() {
  Counts c2, c3;
  for (int id = 0; id < 1600; ++id) {
    const int T = id % 4;
    RunCase(id, 2, T, (id / 4) % 2 ? kSparse : kDense, &c2);
    RunCase(id, 3, T, static_cast<Mode>((id / 4) % 3), &c3);
  }
  std::printf("2D: %d need the top list, %d do not, %d at T = 0, %d long lists tied at the top\n", c2.need_perm,
              c2.no_perm, c2.t0, c2.long_lists);
  std::printf("3D: %d need the top list, %d do not, %d at T = 0, %d long lists tied at the top\n", c3.need_perm,
              c3.no_perm, c3.t0, c3.long_lists);
  for (const Counts& c : {c2, c3})
    if (c.need_perm < 200 || c.no_perm < 200 || c.t0 < 200 || c.long_lists < 200) {
      std::printf("FAIL: too few cases of a kind\n");
      ++failures;
    }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("tie order OK\n");
  return 0;
}
