"""CPU: the oracle's cost rows (oracle/ceres2d.cc Evaluate, oracle/ceres3d.cc
Evaluate3, through oracle_ceres2d_evaluate / oracle_ceres3d_evaluate) against
an independent long-double restatement of the value functions and central
differences of it (tests/ceres_rows_support.py). This is the check of the
oracle's analytic Jacobians against finite differences that the device tests
rest on (test_ceres_rows_gpu.py compares the device's rows with the oracle's).

Every row of every random fixture is compared, values and Jacobian; the rows
built exactly on cell centres and boundaries are compared for value only (the
interpolants are C1 there, but their second derivatives jump, which a central
difference across the joint feels).

Bounds: 4 x the largest deviation measured on these fixtures, the named
constants of ceres_rows_support.py. Measured on this tree,
2D: values 4.4e-15, Jacobian 2.2e-11 of its largest entry; 3D: values
3.6e-15, Jacobian 3.0e-12 of its largest entry."""
import numpy as np
import pytest

import ceres_rows_support as rs


@pytest.fixture(scope="module")
def grids2d():
    return rs.grids2d()


@pytest.fixture(scope="module")
def grids3d(oracle):
    grids = rs.grids3d()
    ogrids = []
    for g in grids:
        og = oracle.hybrid_grid(float(g.resolution))
        og.set_values(g.indices, g.values)
        ogrids.append(og)
    return grids, ogrids


def test_value_tables_are_the_oracles(oracle, grids3d):
    """The restatement's cell values: the 3D table against the oracle's
    GetProbability on known, absent and outside cells."""
    grids, ogrids = grids3d
    for g, og in zip(grids, ogrids):
        lo, hi = g.indices.min(0) - 1, g.indices.max(0) + 1
        rng = np.random.default_rng(5)
        ijk = rng.integers(lo, hi + 1, (200, 3))
        want = [og.probability(int(i), int(j), int(k)) for i, j, k in ijk]
        got = g.probability(ijk[:, 0], ijk[:, 1], ijk[:, 2]).astype(np.float64)
        assert np.array_equal(got, np.asarray(want, np.float64))


def test_2d_fixtures_reach_the_borders_and_the_long_side(grids2d):
    for name, g, cloud, pose, _ in rs.cases2d():
        if len(cloud) >= 253:
            assert rs.taps_reach_the_long_side(grids2d[g], cloud, pose), name
            u, v = rs._coords2d(grids2d[g], cloud, pose)
            for c, n in ((u, grids2d[g].ny), (v, grids2d[g].nx)):
                c = c[np.abs(c) < 1000]  # without the far points
                assert c.min() < -1 and c.max() > n  # taps across both borders


def test_oracle_2d_rows_match_the_restatement(oracle, grids2d):
    worst_r, worst_j = 0.0, 0.0
    for name, g, cloud, pose, target in rs.cases2d():
        grid = grids2d[g]
        r, jac, cost = oracle.ceres2d_evaluate(grid.limits, grid.cells, rs.WEIGHTS_2D, target,
                                               pose, cloud)
        want_r = rs.residuals2d(grid, cloud, rs.WEIGHTS_2D, target, pose)
        want_j = rs.jacobian2d(grid, cloud, rs.WEIGHTS_2D, target, pose)
        dev_r = rs.deviation(r, want_r)
        dev_j = rs.deviation(jac, want_j) / np.abs(jac).max()
        worst_r, worst_j = max(worst_r, dev_r), max(worst_j, dev_j)
        assert dev_r <= rs.BOUND_VALUE_2D, (name, dev_r)
        assert dev_j <= rs.BOUND_JACOBIAN_REL_2D, (name, dev_j, np.abs(jac).max())
        assert cost == pytest.approx(0.5 * float((r * r).sum()), rel=1e-14)
        if len(cloud) >= 253:  # the far points: max cost, zero row
            scale = rs.WEIGHTS_2D[0] / np.sqrt(len(cloud))
            for i in (5, len(cloud) - 1):
                assert r[i] == pytest.approx(scale * float(rs.K_MAX_CC), rel=1e-15)
                assert not jac[i].any()
    print(f"2D oracle against the restatement: values {worst_r:.3e} (bound "
          f"{rs.BOUND_VALUE_2D:.1e}), Jacobian / max|J| {worst_j:.3e} (bound "
          f"{rs.BOUND_JACOBIAN_REL_2D:.1e})")


def test_oracle_2d_exact_rows_match_the_restatement(oracle, grids2d):
    for g, grid in enumerate(grids2d):
        name, _, cloud, pose, target, centre = rs.exact_case2d(g, grid)
        r, _, _ = oracle.ceres2d_evaluate(grid.limits, grid.cells, rs.WEIGHTS_2D, target, pose,
                                          cloud)
        want = rs.residuals2d(grid, cloud, rs.WEIGHTS_2D, target, pose)
        dev = rs.deviation(r, want)
        print(f"{name}: {len(cloud)} points, {int(centre.sum())} on centres, values {dev:.3e}")
        assert dev <= rs.BOUND_VALUE_2D, (name, dev)
        # On a centre the bicubic returns the cell's value itself.
        u, v = rs._coords2d(grid, cloud, pose)
        scale = rs.WEIGHTS_2D[0] / np.sqrt(len(cloud))
        for i in np.nonzero(centre)[0]:
            cell = float(grid.value(np.rint(u[i:i + 1]).astype(np.int64),
                                    np.rint(v[i:i + 1]).astype(np.int64))[0])
            assert r[i] == pytest.approx(scale * cell, rel=1e-14)


def test_oracle_3d_rows_match_the_restatement(oracle, grids3d):
    grids, ogrids = grids3d
    worst_r, worst_j = 0.0, 0.0
    for name, high, low, pose, target in rs.cases3d():
        r, jac, cost = oracle.ceres3d_evaluate(ogrids[0], ogrids[1], high, low, rs.WEIGHTS_3D,
                                               target, pose)
        want_r = rs.residuals3d(grids, (high, low), rs.WEIGHTS_3D, target, *pose)
        want_j = rs.jacobian3d(grids, (high, low), rs.WEIGHTS_3D, target, *pose)
        dev_r = rs.deviation(r, want_r)
        dev_j = rs.deviation(jac, want_j) / np.abs(jac).max()
        worst_r, worst_j = max(worst_r, dev_r), max(worst_j, dev_j)
        assert dev_r <= rs.BOUND_VALUE_3D, (name, dev_r)
        assert dev_j <= rs.BOUND_JACOBIAN_REL_3D, (name, dev_j, np.abs(jac).max())
        assert cost == pytest.approx(0.5 * float((r * r).sum()), rel=1e-14)
        if len(high) >= 14:  # the far points: unknown space, zero row
            for i in (12, 13):
                assert r[i] == pytest.approx(rs.WEIGHTS_3D[0] / np.sqrt(len(high)) *
                                             (1.0 - float(rs.K_MIN_PROBABILITY)), rel=1e-15)
                assert not jac[i].any()
    print(f"3D oracle against the restatement: values {worst_r:.3e} (bound "
          f"{rs.BOUND_VALUE_3D:.1e}), Jacobian / max|J| {worst_j:.3e} (bound "
          f"{rs.BOUND_JACOBIAN_REL_3D:.1e})")


def test_oracle_3d_exact_rows_match_the_restatement(oracle, grids3d):
    grids, ogrids = grids3d
    name, high, low, pose, target = rs.exact_case3d()
    assert (high < 0).any() and (high > 0).any()
    r, _, _ = oracle.ceres3d_evaluate(ogrids[0], ogrids[1], high, low, rs.WEIGHTS_3D, target, pose)
    want = rs.residuals3d(grids, (high, low), rs.WEIGHTS_3D, target, *pose)
    dev = rs.deviation(r, want)
    print(f"3D {name}: {len(high)} + {len(low)} points, values {dev:.3e}")
    assert dev <= rs.BOUND_VALUE_3D, dev


def test_an_older_oracle_library_is_named(oracle):
    """A liboracle.so without the row exports raises a message that says to
    rebuild it (conftest builds the oracle only when the file is missing)."""
    import oracle_lib

    class Old:
        lib = object()
    with pytest.raises(RuntimeError, match="rebuild the oracle"):
        oracle_lib._rows_export(Old(), "oracle_ceres2d_evaluate", [])
