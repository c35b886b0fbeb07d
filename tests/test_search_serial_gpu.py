"""GPU parity of the batch search's item and batch loops (csm_kernels.hip
fast2d_search_v4): the children sums' LDS layout, the pair's best that the
pop prunes with, and the claim of items from the XCD queues. Every pair of every batch is compared with the oracle's
MatchFullSubmap (fast_correlative_scan_matcher_2d.cc:220-235), or Match for
the local windows of the tie case: same decision, bit-identical score, the
reference's pose.

* Bench-shaped pairs (the C3 world of bench.py, 1080-beam scans on 400 x 400
  submaps): hex batches from levels 8 and 6 and full 64-node batches; each
  submap's own node is in the batch, so incumbents exist early and the
  pair's best prunes.
* Small worlds, where the oracle is fast, for the claim bookkeeping: fewer
  items than workgroups, more than 8 submaps (one queue per XCD, no
  spreading), fewer than 8 (spread queues and stealing), and pairs the host
  rejects (empty cloud, submap index out of range) next to valid ones.
* Zero-sum leaves on an all-unknown grid at min_score 0: the tie collect
  launch (kCollect) through the same combine pass and layout.
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from conftest import assert_search_ok
from test_fast2d_gpu import assert_fast_parity, full_submap_center

pytestmark = pytest.mark.gpu

SEED = 20250127  # bench.py's default --seed
LIN, ANG, DEPTH = 7.0, math.radians(30.0), 7  # bench.py's options


def _oracle_full(oracle, world, pairs_sn, min_score):
    """The oracle's MatchFullSubmap of every (submap, node), on a thread pool."""
    def ref(sn):
        s, n = sn
        g = world.grid(s)
        limits = (g.resolution, g.max_x, g.max_y)
        om = oracle.fast2d(limits, g.cells, LIN, ANG, DEPTH)
        cloud = world.cloud(n)
        return om, limits, g.cells, cloud, om.match_full_submap(cloud, min_score)

    with ThreadPoolExecutor(max_workers=12) as ex:
        return list(ex.map(ref, pairs_sn))


def _gpu_full(csm, world, pairs_sn, min_score):
    """The pairs as one match_batch over the submaps they name."""
    subs = sorted({s for s, _ in pairs_sn})
    local = {s: i for i, s in enumerate(subs)}
    opts = csm.FastCorrelativeScanMatcherOptions2D(LIN, ANG, DEPTH, 0)
    mats = [csm.FastCorrelativeScanMatcher2D(world.grid(s), opts) for s in subs]
    scans = csm.ScanSet(None, packed=(world.points, world.offsets))
    pairs = csm.make_pairs([local[s] for s, _ in pairs_sn], [n for _, n in pairs_sn], min_score,
                           full_submap=True)
    res = csm.match_batch(mats, scans, pairs)
    assert_search_ok(csm, res["status"])
    return res


def _compare(oracle, res, refs):
    kinds = []
    for k, (om, limits, cells, cloud, r) in enumerate(refs):
        gpu = (res[k]["status"] == 0, float(res[k]["score"]),
               (res[k]["x"], res[k]["y"], res[k]["theta"]))
        kinds.append(assert_fast_parity(oracle, om, limits, cells, gpu, r, True,
                                        full_submap_center(limits, cells), cloud))
    return kinds


# ------------------------------------------------------- bench-shaped pairs --

@pytest.fixture(scope="module")
def c3_world(csm):
    return csm.SyntheticWorld2D(num_nodes=2000, num_submaps=1000, submap_cells=400, beams=1080,
                                seed=SEED)


@pytest.fixture(scope="module")
def c3_case(oracle, c3_world):
    """3 submaps x 4 nodes: each submap's own node, its neighbour and two
    nodes from elsewhere in the queue; the oracle's results, computed once."""
    w = c3_world
    pairs_sn = []
    for s in (3, 417, 902):
        own = int(w.submap_nodes[s])
        nodes = [own, min(w.num_nodes - 1, own + 1), (own + 700) % w.num_nodes,
                 (own + 1300) % w.num_nodes]
        pairs_sn += [(s, n) for n in nodes]
    return pairs_sn, _oracle_full(oracle, w, pairs_sn, 0.55)


@pytest.mark.parametrize("order", ["default", "lifo"])
def test_bench_shaped_pairs_match_oracle(csm, oracle, c3_world, c3_case, monkeypatch, order):
    monkeypatch.delenv("CSM_SEARCH_ORDER", raising=False)
    if order != "default":
        monkeypatch.setenv("CSM_SEARCH_ORDER", order)  # read by the host per call
    pairs_sn, refs = c3_case
    res = _gpu_full(csm, c3_world, pairs_sn, 0.55)
    kinds = _compare(oracle, res, refs)
    assert kinds.count("nomatch") < len(kinds), kinds


# ------------------------------------------------------------ small worlds --

# 120-beam scans on 100 x 100 submaps; at min_score 0.35 the oracle accepts
# 15 of (b)'s 108 pairs and 22 of (c)'s 120 (counted with the oracle alone).
SMALL_MIN_SCORE = 0.35


@pytest.fixture(scope="module")
def small_world(csm):
    return csm.SyntheticWorld2D(num_nodes=120, num_submaps=12, submap_cells=100, beams=120,
                                seed=11)


def _nodes_near(world, s, count):
    """`count` consecutive nodes around the node submap s was built at."""
    c = int(world.submap_nodes[s])
    lo = max(0, min(world.num_nodes - count, c - count // 2))
    return list(range(lo, lo + count))


SMALL_BATCHES = {
    "one_pair": (1, 1, 0.0),        # fewer items than workgroups
    "nine_submaps": (9, 12, 0.1),   # more than 8 submaps: one queue per XCD
    "three_submaps": (3, 40, 0.1),  # fewer than 8: spread queues, stealing
}


@pytest.mark.parametrize("batch", list(SMALL_BATCHES))
def test_small_batches_match_oracle(csm, oracle, small_world, batch):
    num_s, per_s, share = SMALL_BATCHES[batch]
    w = small_world
    pairs_sn = [(s, n) for s in range(num_s) for n in _nodes_near(w, s, per_s)]
    refs = _oracle_full(oracle, w, pairs_sn, SMALL_MIN_SCORE)
    res = _gpu_full(csm, w, pairs_sn, SMALL_MIN_SCORE)
    kinds = _compare(oracle, res, refs)
    accepted = len(kinds) - kinds.count("nomatch")
    assert accepted >= share * len(kinds), (accepted, len(kinds))


def test_rejected_pairs_next_to_valid_ones(csm, oracle, small_world):
    """A pair with an empty cloud (CSM_NO_MATCH) and one whose submap index is
    out of range (CSM_EINVAL) never reach the device; their neighbours' items
    are claimed and searched as if they were not there."""
    w = small_world
    valid = [(s, n) for s in range(2) for n in _nodes_near(w, s, 3)]
    refs = _oracle_full(oracle, w, valid, SMALL_MIN_SCORE)
    opts = csm.FastCorrelativeScanMatcherOptions2D(LIN, ANG, DEPTH, 0)
    mats = [csm.FastCorrelativeScanMatcher2D(w.grid(s), opts) for s in range(2)]
    # Scan k < num_nodes is node k's cloud; scan num_nodes is empty.
    offsets = np.concatenate([w.offsets, w.offsets[-1:]])
    scans = csm.ScanSet(None, packed=(w.points, offsets))
    empty = w.num_nodes
    # valid[0..2], empty cloud, valid[3], bad submap, valid[4..5]
    sub = [s for s, _ in valid[:3]] + [0] + [valid[3][0]] + [2] + [s for s, _ in valid[4:]]
    node = [n for _, n in valid[:3]] + [empty] + [valid[3][1]] + [5] + [n for _, n in valid[4:]]
    res = csm.match_batch(mats, scans, csm.make_pairs(sub, node, SMALL_MIN_SCORE, full_submap=True))
    assert res[3]["status"] == csm.CSM_NO_MATCH
    assert res[5]["status"] == csm.CSM_EINVAL
    keep = [0, 1, 2, 4, 6, 7]
    assert_search_ok(csm, res["status"][keep])
    _compare(oracle, res[keep], refs)


# -------------------------------------------------------------------- ties --

@pytest.mark.parametrize("depth", [1, 2, 4])
def test_zero_sum_leaves_match_oracle(csm, oracle, depth):
    """The input of test_ties_walk.py::test_zero_sum_leaves_without_incumbent:
    clouds wholly in unknown cells at min_score 0, small local windows. Every
    leaf sums to 0 and ties; the pose must be the reference's pick."""
    cells = np.zeros((60, 60), np.uint16)
    cells[:12, :12] = 20000  # known cells far from the clouds
    limits = (1.0, 30.0, 30.0)
    grid = csm.ProbabilityGrid(*limits, cells)
    rng = np.random.default_rng(17 + depth)
    clouds = [np.array([[0.3, -0.2, 0.0]], np.float32),
              rng.uniform(-2, 2, (5, 3)).astype(np.float32)]
    mats, sub, scan, init, refs = [], [], [], [], []
    for lin in (1.0, 2.0, 3.0):
        for ang in (0.0, math.radians(2.0)):
            m = csm.FastCorrelativeScanMatcher2D(grid, csm.FastCorrelativeScanMatcherOptions2D(
                lin, ang, depth))
            om = oracle.fast2d(limits, cells, lin, ang, depth)
            for i, c in enumerate(clouds):
                start = (-10.0 + 0.3 * i, -12.0, 0.1)
                sub.append(len(mats))
                scan.append(i)
                init.append(start)
                refs.append(om.match(start, c, 0.0))
            mats.append(m)
    pairs = csm.make_pairs(sub, scan, 0.0, full_submap=False, initial=init)
    res = csm.match_batch(mats, csm.ScanSet(clouds), pairs)
    assert_search_ok(csm, res["status"])
    for k, (ok, score, pose) in enumerate(r[:3] for r in refs):
        assert ok, refs[k]  # every leaf sums to 0, and 0 passes min_score 0
        assert res[k]["status"] == 0
        assert np.float32(res[k]["score"]) == np.float32(score)
        got = (res[k]["x"], res[k]["y"], res[k]["theta"])
        assert got == tuple(pose), ("pose differs from the reference's pick", got, pose)
