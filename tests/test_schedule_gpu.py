"""The interleaved work queues of the v4/v5 search kernel (csm_schedule.h,
DESIGN.md §5 "Rotation chunks") leave every result what the oracle computes:
batches whose pairs fill one block, one more than a block, several queues
(3 submaps spread over 6, 9 over 8), ragged item counts from 1 to about
130, nothing above min_score, and a grid on which every leaf ties. Small
shapes: 96 x 96-cell submaps and 120-beam clouds."""
import math

import numpy as np
import pytest

from conftest import assert_search_ok
from test_fast2d_gpu import assert_fast_parity, full_submap_center

pytestmark = pytest.mark.gpu

BLOCK = 256  # csm_schedule.h CSM_SCHED_BLOCK
LIN, ANG, DEPTH = 7.0, math.radians(30.0), 5
SCALES = (1.0, 0.6, 0.35)  # a cloud's largest range sets its rotation count
# Window-mode matchers (submap indices 9 + 3 s + w, s < 3): 1 m and these
# angular windows, 3 to 21 rotations = 1 to 3 items of 8 rotations.
WINDOWS = (0.003, 0.03, 0.06)


@pytest.fixture(scope="module")
def world(csm):
    return csm.SyntheticWorld2D(num_nodes=24, num_submaps=9, submap_cells=96, beams=120,
                                seed=4242, max_range=8.0)


@pytest.fixture(scope="module")
def setup(csm, oracle, world):
    """Matchers, oracle matchers, the scan set (every node's cloud at every
    scale: scan = node * len(SCALES) + scale index) and a cache of the oracle's
    answers, shared by the cases."""
    grids = [world.grid(s) for s in range(world.num_submaps)]
    windows = [(LIN, ANG)] * len(grids)
    for s in range(3):
        grids += [grids[s]] * len(WINDOWS)
        windows += [(1.0, w) for w in WINDOWS]
    mats = [csm.FastCorrelativeScanMatcher2D(
        g, csm.FastCorrelativeScanMatcherOptions2D(lin, ang, DEPTH)) for g, (lin, ang) in zip(grids, windows)]
    oms = [oracle.fast2d((g.resolution, g.max_x, g.max_y), g.cells, lin, ang, DEPTH)
           for g, (lin, ang) in zip(grids, windows)]
    clouds = []
    for n in range(world.num_nodes):
        for f in SCALES:
            c = np.array(world.cloud(n), np.float32)
            c[:, :2] *= np.float32(f)
            clouds.append(np.ascontiguousarray(c))
    return {"mats": mats, "oms": oms, "grids": grids, "clouds": clouds,
            "scans": csm.ScanSet(clouds), "cache": {}}


def _reference(setup, s, scan, full, init, min_score):
    key = (s, scan, full, init, min_score)
    if key not in setup["cache"]:
        om, cloud = setup["oms"][s], setup["clouds"][scan]
        setup["cache"][key] = (om.match_full_submap(cloud, min_score) if full
                               else om.match(init, cloud, min_score))
    return setup["cache"][key]


def _check_batch(csm, oracle, setup, spec, min_score):
    """spec: (submap, scan, full, initial). Runs the batch twice (byte-equal
    results) and compares every pair with the oracle; returns the kinds."""
    pairs = np.zeros(len(spec), dtype=csm.make_pairs([0], [0], 0.0).dtype)
    for k, (s, scan, full, init) in enumerate(spec):
        pairs[k] = csm.make_pairs([s], [scan], min_score, full_submap=full,
                                  initial=None if full else [init])[0]
    res = csm.match_batch(setup["mats"], setup["scans"], pairs)
    assert_search_ok(csm, res["status"])
    again = csm.match_batch(setup["mats"], setup["scans"], pairs)
    assert res.tobytes() == again.tobytes()
    kinds = []
    for k, (s, scan, full, init) in enumerate(spec):
        g = setup["grids"][s]
        limits = (g.resolution, g.max_x, g.max_y)
        ref = _reference(setup, s, scan, full, init, min_score)
        gpu = (int(res[k]["status"]) == csm.CSM_OK, float(res[k]["score"]),
               (float(res[k]["x"]), float(res[k]["y"]), float(res[k]["theta"])))
        kinds.append(assert_fast_parity(
            oracle, setup["oms"][s], limits, g.cells, gpu, ref, full,
            full_submap_center(limits, g.cells) if full else init, setup["clouds"][scan]))
    return kinds


def _full(world, pairs):
    """(submap, node, scale index) -> full-submap spec rows."""
    return [(s, n * len(SCALES) + f, True, None) for s, n, f in pairs]


def test_one_pair(csm, oracle, world, setup):
    n = int(world.submap_nodes[0])
    assert _check_batch(csm, oracle, setup, _full(world, [(0, n, 2)]), 0.4) == ["exact"]


def test_block_plus_one_pairs_on_one_submap(csm, oracle, world, setup):
    """BLOCK + 1 pairs of one submap: a full block and a block of one pair.
    The 72 distinct (node, scale) clouds repeat; each repeat is a pair of its
    own to the queues."""
    count = world.num_nodes * len(SCALES)
    spec = [(0, k % count, True, None) for k in range(BLOCK + 1)]
    kinds = _check_batch(csm, oracle, setup, spec, 0.4)
    assert kinds.count("exact") >= 3


@pytest.mark.parametrize("submaps", [3, 9])
def test_several_submaps(csm, oracle, world, setup, submaps):
    """3 submaps: each on two queues; 9: queue 0 holds submaps 0 and 8."""
    pairs = [(s, int(world.submap_nodes[s]), 0) for s in range(submaps)]
    pairs += [(s, (5 * s + 3 * k) % world.num_nodes, k % len(SCALES))
              for s in range(submaps) for k in range(7)]
    kinds = _check_batch(csm, oracle, setup, _full(world, pairs), 0.4)
    assert kinds.count("exact") >= submaps // 3


def test_ragged_full_and_window_pairs(csm, oracle, world, setup):
    """Full-submap pairs of three rotation counts (about 40 to 130 items) next
    to window-mode Match pairs of one to three items (WINDOWS)."""
    rng = np.random.RandomState(11)
    spec = _full(world, [(s, (s + 4 * k) % world.num_nodes, k % len(SCALES))
                         for s in range(3) for k in range(6)])
    for s in range(3):
        n = int(world.submap_nodes[s])
        truth = world.node_poses[n]
        for k in range(6):
            init = (float(truth[0] + rng.uniform(-0.3, 0.3)), float(truth[1] + rng.uniform(-0.3, 0.3)),
                    float(truth[2] + rng.uniform(-0.02, 0.02)))
            spec.append((world.num_submaps + len(WINDOWS) * s + k % len(WINDOWS), n * len(SCALES), False, init))
    rng.shuffle(spec)
    kinds = _check_batch(csm, oracle, setup, spec, 0.3)
    for full in (True, False):
        assert sum(1 for row, kind in zip(spec, kinds) if row[2] == full and kind == "exact") >= 3


def test_all_rejected(csm, oracle, world, setup):
    pairs = [(s, (s + 2 * k) % world.num_nodes, k % len(SCALES)) for s in range(4) for k in range(5)]
    kinds = _check_batch(csm, oracle, setup, _full(world, pairs), 0.99)
    assert kinds == ["nomatch"] * len(pairs)


def test_plateau_every_leaf_ties(csm, oracle, world):
    """An all-unknown grid at min_score 0: every leaf inside the grid ties, and
    the reference's pick comes out for each of the ragged pairs."""
    cells = np.zeros((96, 96), np.uint16)
    limits = (0.05, 2.4, 2.4)
    grid = csm.ProbabilityGrid(*limits, cells)
    m = csm.FastCorrelativeScanMatcher2D(grid, csm.FastCorrelativeScanMatcherOptions2D(LIN, ANG, DEPTH))
    om = oracle.fast2d(limits, cells, LIN, ANG, DEPTH)
    rng = np.random.default_rng(5)
    clouds = [np.array([[0.1, 0.2, 0.0]], np.float32)]
    clouds += [rng.uniform(-r, r, (n, 3)).astype(np.float32) for r, n in ((0.5, 7), (1.5, 30), (3.0, 60))]
    scans = csm.ScanSet(clouds)
    pairs = csm.make_pairs(np.zeros(len(clouds), np.int32), np.arange(len(clouds), dtype=np.int32), 0.0)
    res = csm.match_batch([m], scans, pairs)
    assert_search_ok(csm, res["status"])
    assert res.tobytes() == csm.match_batch([m], scans, pairs).tobytes()
    for k, c in enumerate(clouds):
        gpu = (int(res[k]["status"]) == csm.CSM_OK, float(res[k]["score"]),
               (float(res[k]["x"]), float(res[k]["y"]), float(res[k]["theta"])))
        kind = assert_fast_parity(oracle, om, limits, cells, gpu, om.match_full_submap(c, 0.0), True,
                                  full_submap_center(limits, cells), c)
        assert kind == "exact"
        assert res[k]["tie"] != csm.TIE_NONE
