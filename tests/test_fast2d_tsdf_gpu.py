"""FastCorrelativeScanMatcher2D on a TSDF2D (csm_fast2d_create_tsdf,
csm_fast2d_create_from_tsdf_grid): the PrecomputationGridStack2D is built from
the TSD cells with Grid2D's bounds of a TSDF, -/+ truncation
(fast_correlative_scan_matcher_2d.cc:97-98, :105-160). The levels are compared
with the numpy restatement that test_ceres_tsdf_host.py proves against the
oracle; Match and MatchFullSubmap with a brute force over every level-0
candidate (ceres_tsdf_support.brute_force_match, equal to the oracle's matcher
on probability grids)."""
import math

import numpy as np
import pytest

import ceres_tsdf_support as cs
import tsdf_support as ts

pytestmark = pytest.mark.gpu

LIN, ANG, DEPTH = 0.5, 0.2, 3


@pytest.fixture(scope="module")
def room(csm):
    return cs.room_tsdf(csm)


@pytest.fixture(scope="module")
def matcher(csm, room):
    m = csm.FastCorrelativeScanMatcher2D(
        room, csm.FastCorrelativeScanMatcherOptions2D(LIN, ANG, DEPTH, 5))
    yield m
    m.close()


def _limits(room):
    return (room.resolution, room.max_x, room.max_y)


def test_every_level_equals_the_numpy_restatement(room, matcher):
    level0 = cs.quantized_level0(room.tsd_cells, -ts.TRUNCATION, ts.TRUNCATION)
    # 1 - |tsd| over [1 - trunc, 1 + trunc]: unknown (+trunc) and the surface differ.
    assert level0.min() == 0 and level0.max() > 100
    for d in range(5):
        assert np.array_equal(matcher.read_level(d), cs.sliding_max_level(level0, 1 << d)), d


@pytest.mark.parametrize("scan", [2, 5, 8])
def test_match_equals_the_brute_force(oracle, room, matcher, scan):
    cloud, origin = cs.room_cloud(scan, 60)
    init = (origin[0] + 0.1, origin[1] - 0.07, 0.03)
    score, pose, at_max = cs.brute_force_match(oracle, _limits(room), room.tsd_cells,
                                               -ts.TRUNCATION, ts.TRUNCATION, init, LIN, ANG, cloud)
    assert at_max == 1  # a unique maximum: the pose is decided
    ok, got_score, got_pose = matcher.Match(init, cloud, 0.1)
    assert ok and np.float32(got_score) == score, (got_score, score)
    assert got_pose == pose, (got_pose, pose)
    above = float(np.nextafter(score, np.float32(2.0)))
    assert matcher.Match(init, cloud, above)[0] is False  # CSM_NO_MATCH


@pytest.mark.parametrize("scan", [8, 9])
def test_match_full_submap_equals_the_brute_force(csm, oracle, room, scan):
    """The reference's 1e6 m window, clipped to the grid by ShrinkToFit."""
    full = csm.FastCorrelativeScanMatcher2D(
        room, csm.FastCorrelativeScanMatcherOptions2D(1e6, math.pi, DEPTH))
    cloud = cs.room_near_cloud(scan, 2.6, 40)
    centre = cs.full_submap_centre(_limits(room) + (room.num_x_cells, room.num_y_cells))
    score, pose, at_max = cs.brute_force_match(oracle, _limits(room), room.tsd_cells,
                                               -ts.TRUNCATION, ts.TRUNCATION, centre, 1e6, math.pi,
                                               cloud)
    assert at_max == 1
    ok, got_score, got_pose = full.MatchFullSubmap(cloud, 0.1)
    assert ok and np.float32(got_score) == score, (got_score, score)
    assert got_pose == pose, (got_pose, pose)
    above = float(np.nextafter(score, np.float32(2.0)))
    assert full.MatchFullSubmap(cloud, above)[0] is False
    full.close()


def test_match_batch_over_tsdf_and_probability_handles(csm, room, matcher):
    """Two TSDF handles (host planes, device grid) and a probability handle in
    one csm_fast2d_match_batch: every pair gets its single-call result."""
    opts = csm.FastCorrelativeScanMatcherOptions2D(LIN, ANG, DEPTH, 5)
    dev = csm.DeviceTSDF2D.from_host(room)
    from_dev = csm.FastCorrelativeScanMatcher2D(dev, opts)
    w = csm.SyntheticWorld2D(num_nodes=4, num_submaps=1, submap_cells=96, decimate_to=50, seed=3)
    prob = csm.FastCorrelativeScanMatcher2D(w.grid(0), opts)
    node = int(w.submap_nodes[0])
    t = w.node_poses[node]
    clouds = [cs.room_cloud(2, 60)[0], cs.room_cloud(5, 60)[0], w.cloud(node)]
    origins = [cs.room_cloud(2, 60)[1], cs.room_cloud(5, 60)[1]]
    init = [(origins[0][0] + 0.1, origins[0][1] - 0.07, 0.03),
            (origins[1][0] - 0.05, origins[1][1] + 0.1, -0.02),
            (t[0] + 0.1, t[1] - 0.05, t[2] + 0.02)]
    matchers = [matcher, from_dev, prob]
    scans = csm.ScanSet(clouds)
    sub, scn = [0, 1, 2, 1, 0], [0, 1, 2, 0, 1]
    pairs = csm.make_pairs(sub, scn, 0.1, full_submap=False, initial=[init[s] for s in scn])
    res = csm.match_batch(matchers, scans, pairs)
    for k in range(len(sub)):
        ok, score, pose = matchers[sub[k]].Match(init[scn[k]], clouds[scn[k]], 0.1)
        assert ok and res["status"][k] == csm.CSM_OK
        assert np.float32(res["score"][k]) == np.float32(score)
        assert (res["x"][k], res["y"][k], res["theta"][k]) == pose
    # The same grid by either route: the same answers.
    assert res["score"][0] == res["score"][3] and res["score"][1] == res["score"][4]
