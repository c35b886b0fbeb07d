"""The CPU restatement of CeresScanMatcher2D::Match on a TSDF2D
(tests/cpp/oracle_ceres_tsdf_shim.cc) that checks the device path. Ceres is
absent, so the restatement is pinned by the reference's own expectations:
tsdf_match_cost_function_2d_test.cc's four tests and both
interpolated_tsdf_2d_test.cc cases, at those files' tolerances; its Jacobian is
checked against central differences of its own residuals. The numpy restatement
of the PrecomputationGridStack2D levels that the GPU search tests use is proved
against the oracle's levels on a probability grid. The candidate-failure
configurations the GPU test runs are pinned here."""
import numpy as np
import pytest

import ceres_tsdf_support as cs


def test_restatement_passes_the_reference_cost_function_tests(csm):
    """tsdf_match_cost_function_2d_test.cc:74-161, DoubleNear 1e-3."""
    empty = cs.reference_fixture(csm, empty=True)
    valid, _, _ = cs.restated_evaluate(empty, np.zeros((1, 3), np.float32), 1.0, (0.0, 0.0, 0.0))
    assert not valid  # MatchEmptyTSDF
    grid = cs.reference_fixture(csm)
    assert (grid.weight_cells != 0).sum() > 0
    for pose, want_valid, want_r, want_j in cs.REF_CASES:
        valid, r, jac = cs.restated_evaluate(grid, cs.REF_CLOUD, 1.0, pose)
        assert valid == want_valid, pose
        if valid:
            assert abs(r[0] - want_r) <= 1e-3, (pose, r)
            assert np.all(np.abs(jac[0] - np.asarray(want_j)) <= 1e-3), (pose, jac)


def test_restatement_passes_the_reference_interpolation_tests():
    """interpolated_tsdf_2d_test.cc:48-88 (1e-4) and :90-120 (1e-3)."""
    assert cs.shim().shim_interpolated_tsdf_ref_tests() == 0


def _crosses_no_centre_line(grid, cloud, poses):
    """True when every point of `cloud` keeps its lower pixel over all `poses`:
    no stencil evaluation crosses a cell-centre line, where the interpolation
    has a kink."""
    px, py = cloud[:, 0].astype(np.float64), cloud[:, 1].astype(np.float64)
    lower = None
    for x, y, t in poses:
        c, s = np.cos(t), np.sin(t)
        u = (grid.max_x - (c * px - s * py + x)) / grid.resolution - 0.5
        v = (grid.max_y - (s * px + c * py + y)) / grid.resolution - 0.5
        for w in (u, v):
            if np.abs(w - np.round(w)).min() < 1e-4:  # float centres: keep clear of the lines
                return False
        cell = np.stack([np.floor(u), np.floor(v)])
        if lower is not None and not np.array_equal(cell, lower):
            return False
        lower = cell
    return True


def test_restated_jacobian_matches_central_differences(csm):
    """20 seeded poses on the room TSDF, 12-point clouds; a pose qualifies when
    its +-1e-6 stencil crosses no cell-centre line. 1e-5 relative to the
    Jacobian's largest entry: the differences' truncation and rounding error
    (residuals of order 1, step 1e-6), not a judgment of the code."""
    room = cs.room_tsdf(csm)
    rng = np.random.default_rng(21)
    h = 1e-6
    qualified = 0
    for k in range(20):
        cloud, origin = cs.room_cloud(2 + k % 8, 12)
        pose = np.array([origin[0] + rng.normal(0, 0.05), origin[1] + rng.normal(0, 0.05),
                         rng.normal(0, 0.03)])
        stencil = [pose] + [pose + sgn * h * np.eye(3)[a] for a in range(3) for sgn in (1, -1)]
        if not _crosses_no_centre_line(room, cloud, stencil):
            continue
        valid, _, jac = cs.restated_evaluate(room, cloud, 20.0 / np.sqrt(12), pose)
        assert valid
        fd = np.zeros_like(jac)
        for a in range(3):
            _, rp, _ = cs.restated_evaluate(room, cloud, 20.0 / np.sqrt(12), stencil[1 + 2 * a])
            _, rm, _ = cs.restated_evaluate(room, cloud, 20.0 / np.sqrt(12), stencil[2 + 2 * a])
            fd[:, a] = (rp - rm) / (2 * h)
        scale = np.abs(jac).max()
        assert scale > 0
        assert np.abs(fd - jac).max() <= 1e-5 * scale, (k, np.abs(fd - jac).max(), scale)
        qualified += 1
    assert qualified >= 10, qualified


def test_numpy_pyramid_levels_match_the_oracle_on_a_probability_grid(csm, oracle):
    """The numpy levels (quantised 1 - |cost| table, sliding 2^d x 2^d maximum
    over the widened grid) equal oracle_fast2d_level, which restates
    fast_correlative_scan_matcher_2d.cc:105-160."""
    w = csm.SyntheticWorld2D(num_nodes=4, num_submaps=1, submap_cells=96, decimate_to=50, seed=3)
    g = w.grid(0)
    om = oracle.fast2d((g.resolution, g.max_x, g.max_y), g.cells, 1.0, 0.1, 4)
    level0 = cs.quantized_level0(g.cells, g.min_correspondence_cost, g.max_correspondence_cost)
    assert len(np.unique(level0)) > 4
    for d in range(4):
        assert np.array_equal(cs.sliding_max_level(level0, 1 << d), om.level(d)), d


@pytest.mark.parametrize("opts,cloud,want_failed", cs.CANDIDATE_FAILURES)
def test_candidate_evaluations_fail_in_the_pinned_configurations(csm, opts, cloud, want_failed):
    room = cs.room_tsdf(csm)
    pose, iters, failed = cs.restated_match(room, opts, (0.0, 0.0), (0.0, 0.0, 0.0),
                                            np.asarray(cloud, np.float32))
    assert failed == want_failed and iters == opts[3], (failed, iters)
    assert np.all(np.isfinite(pose))
    # The initial-failure rule: nothing weighted under the cloud.
    pose0, it0, f0 = cs.restated_match(room, opts, (0.0, 0.0), (0.1, -0.2, 0.05),
                                       np.array([[0.0, 0.0, 0.0]], np.float32))
    assert pose0 == (0.1, -0.2, 0.05) and it0 == 0 and f0 == 0


def test_brute_force_matcher_equals_the_oracle_on_a_probability_grid(csm, oracle):
    """ceres_tsdf_support.brute_force_match (which the GPU search tests on TSDF
    submaps compare with) gives the oracle matcher's score and pose, for Match
    and for MatchFullSubmap."""
    import math
    w = csm.SyntheticWorld2D(num_nodes=4, num_submaps=1, submap_cells=96, decimate_to=50, seed=3)
    g = w.grid(0)
    node = int(w.submap_nodes[0])
    cloud, t = w.cloud(node), w.node_poses[node]
    limits = (g.resolution, g.max_x, g.max_y)
    cc = (g.min_correspondence_cost, g.max_correspondence_cost)
    init = (t[0] + 0.1, t[1] - 0.05, t[2] + 0.02)
    ok, score, pose, _ = oracle.fast2d(limits, g.cells, 0.5, 0.2, 3).match(init, cloud, 0.1)
    got = cs.brute_force_match(oracle, limits, g.cells, *cc, init, 0.5, 0.2, cloud)
    assert ok and got[2] == 1
    assert got[0] == np.float32(score) and got[1] == tuple(float(v) for v in pose)
    full = oracle.fast2d(limits, g.cells, 1e6, math.pi, 3)
    ok, score, pose, _ = full.match_full_submap(cloud, 0.1)
    centre = cs.full_submap_centre(limits + (g.num_x_cells, g.num_y_cells))
    got = cs.brute_force_match(oracle, limits, g.cells, *cc, centre, 1e6, math.pi, cloud)
    assert ok and got[2] == 1
    assert got[0] == np.float32(score) and got[1] == tuple(float(v) for v in pose)
