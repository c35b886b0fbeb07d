"""GPU: the rows and sums of the two default cost blocks, the probability
grid's bicubic block (ceres2d.hip Row / Pass, float-plane and kU16 forms) and
the 3D occupied-space block with its delta rows (ceres3d.hip Pass3), through
csm_ceres2d_evaluate, csm_ceres2d_evaluate_grid and csm_ceres3d_evaluate: the
device functions the refinement kernels call, which here also write their
rows.

Rows: against the oracle's rows (oracle_ceres2d_evaluate /
oracle_ceres3d_evaluate, which test_ceres_rows_host.py checks against an
independent restatement and finite differences), 1e-9 absolute, the bound of
csm_ceres2d_tsdf_evaluate and csm_ceres3d_intensity_evaluate
(test_ceres_tsdf_gpu.py), on every fixture of ceres_rows_support.py: non-square
grids, taps across every border, points far outside and exactly on centres and
boundaries, clouds around the 256-thread stride.

Sums: against float64 numpy sums of the device's own rows, within the
summation error 4 * rows * 2^-52 * sum|terms| per entry, which isolates
BlockSum and the strided loop from the row arithmetic.

Refinement at those shapes: the batch entries against the oracle's solver at
the existing bound, 1e-6 and +-1 iteration."""
import math

import numpy as np
import pytest

import ceres_rows_support as rs

pytestmark = pytest.mark.gpu

ROW_BOUND = 1e-9


def _sums_within_rounding(sums, r, jac, name):
    want, magnitude = rs.packed_sums(r, jac)
    bound = 4.0 * len(r) * 2.0 ** -52 * magnitude
    err = np.abs(sums - want)
    assert np.all(err <= bound), (name, np.nonzero(err > bound)[0], err, bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))


# ------------------------------------------------------------------- 2D ----
@pytest.fixture(scope="module")
def grids2d(csm):
    """Per fixture grid: (restatement grid, matcher on a handle, device grid
    of the same cells)."""
    out = []
    for g in rs.grids2d():
        host = csm.ProbabilityGrid(g.resolution, g.max_x, g.max_y, g.cells)
        matcher = csm.FastCorrelativeScanMatcher2D(
            host, csm.FastCorrelativeScanMatcherOptions2D(0.1, 0.1, 1, 1))
        out.append((g, matcher, csm.DeviceProbabilityGrid.from_host(host)))
    return out


@pytest.fixture(scope="module")
def oracle_rows2d(oracle):
    """The oracle's rows of every 2D case, computed once."""
    grids = rs.grids2d()
    cases = rs.cases2d() + [rs.exact_case2d(g, grid)[:5] for g, grid in enumerate(grids)]
    return [(case, oracle.ceres2d_evaluate(grids[case[1]].limits, grids[case[1]].cells,
                                           rs.WEIGHTS_2D, case[4], case[3], case[2])[:2])
            for case in cases]


@pytest.mark.parametrize("entry", ["handle", "device_grid"])
def test_2d_rows_and_sums(csm, grids2d, oracle_rows2d, entry):
    opts = csm.CeresOptions2D.make(*rs.WEIGHTS_2D, 10)
    worst = 0.0
    for (name, g, cloud, pose, target), (ref_r, ref_j) in oracle_rows2d:
        on = grids2d[g][1] if entry == "handle" else grids2d[g][2]
        r, jac, sums = csm.ceres_evaluate(on, cloud, opts, target, pose)
        assert r.shape == ref_r.shape and jac.shape == ref_j.shape
        dev_r, dev_j = np.abs(r - ref_r).max(), np.abs(jac - ref_j).max()
        # S[0] is the sum of squares, not the cost 1/2 sum r^2.
        assert sums[0] == pytest.approx(float((r * r).sum()), rel=1e-12)
        part = _sums_within_rounding(sums, r, jac, name)
        print(f"2D {entry} {name}: residuals {dev_r:.3e} Jacobian {dev_j:.3e} "
              f"sums {part:.2f} of their bound")
        assert dev_r <= ROW_BOUND and dev_j <= ROW_BOUND, (name, dev_r, dev_j)
        worst = max(worst, dev_r, dev_j)
    print(f"2D {entry}: largest deviation from the oracle's rows {worst:.3e}")


def test_2d_evaluate_rejects_a_tsdf_handle_and_bad_input(csm, grids2d):
    import ceres_tsdf_support as cs
    opts = csm.CeresOptions2D.make(*rs.WEIGHTS_2D, 10)
    cloud = np.zeros((2, 3), np.float32)
    tsdf = csm.FastCorrelativeScanMatcher2D(cs.reference_fixture(csm),
                                            csm.FastCorrelativeScanMatcherOptions2D(0.1, 0.1, 1, 1))
    with pytest.raises(csm.CsmError):
        csm.ceres_evaluate(tsdf, cloud, opts, (0, 0, 0), (0, 0, 0))
    _, matcher, device = grids2d[0]
    for on in (matcher, device):
        with pytest.raises(csm.CsmError):
            csm.ceres_evaluate(on, cloud, csm.CeresOptions2D.make(0.0, 10.0, 1.0, 10), (0, 0, 0),
                               (0, 0, 0))
        with pytest.raises(csm.CsmError):
            csm.ceres_evaluate(on, cloud, opts, (0, 0, 0), (0, float("nan"), 0))
        with pytest.raises(csm.CsmError):
            csm.ceres_evaluate(on, np.zeros((0, 3), np.float32), opts, (0, 0, 0), (0, 0, 0))


def test_2d_refinement_matches_oracle_at_the_row_shapes(csm, oracle, grids2d):
    """csm_ceres2d_refine_batch and csm_ceres2d_match_grid (kU16) on the
    non-square grids, clouds of 1 to 257 points that take the strided loop
    around its second trip, starts perturbed as test_ceres2d.py's."""
    opts = (20.0, 10.0, 1.0, 10)
    rng = np.random.default_rng(9)
    clouds, sub, scn, init, tgt = [], [], [], [], []
    for g, (grid, _, _) in enumerate(grids2d):
        for k, n in enumerate((1, 2, 253, 254, 256, 257)):
            t = rs._pose2d(g, k % len(rs.THETAS_2D))
            clouds.append(rs.cloud2d(grid, t, n, 50 + 10 * g + k))
            p = (t[0] + rng.normal(0, 0.05), t[1] + rng.normal(0, 0.05),
                 t[2] + rng.normal(0, 0.03))
            sub.append(g)
            scn.append(len(clouds) - 1)
            init.append(p)
            tgt.append((p[0] + rng.normal(0, 0.01), p[1] + rng.normal(0, 0.01)))
    scans = csm.ScanSet(clouds)
    copts = csm.CeresOptions2D.make(*opts)
    poses, iters = csm.ceres_refine_batch([m for _, m, _ in grids2d], scans, sub, scn, init, tgt,
                                          copts)
    on_grid = csm.CeresScanMatcher2D(copts)
    for k in range(len(sub)):
        grid = grids2d[sub[k]][0]
        ref, ref_it = oracle.ceres2d_match(grid.limits, grid.cells, opts, tgt[k], init[k],
                                           clouds[k])
        pose16, it16 = on_grid.Match(tgt[k], init[k], clouds[k], grids2d[sub[k]][2])
        print(f"2D refine grid{sub[k]} n={len(clouds[k])}: batch {np.abs(poses[k] - ref).max():.3e} "
              f"({iters[k]} / {ref_it} iterations), device grid "
              f"{np.abs(np.asarray(pose16) - ref).max():.3e} ({it16})")
        assert np.allclose(poses[k], ref, atol=1e-6), (k, poses[k], ref)
        assert abs(int(iters[k]) - ref_it) <= 1
        assert np.allclose(pose16, ref, atol=1e-6), (k, pose16, ref)
        assert abs(it16 - ref_it) <= 1


# ------------------------------------------------------------------- 3D ----
@pytest.fixture(scope="module")
def grids3d(csm, oracle):
    grids = rs.grids3d()
    device, ogrids = [], []
    for g in grids:
        device.append(csm.HybridGrid(float(g.resolution), g.indices, g.values))
        og = oracle.hybrid_grid(float(g.resolution))
        og.set_values(g.indices, g.values)
        ogrids.append(og)
    return device, ogrids


def test_3d_rows_and_sums(csm, oracle, grids3d):
    device, ogrids = grids3d
    opts = csm.CeresOptions3D.make(*rs.WEIGHTS_3D, 10)
    worst = 0.0
    for name, high, low, pose, target in rs.cases3d() + [rs.exact_case3d()]:
        ref_r, ref_j, _ = oracle.ceres3d_evaluate(ogrids[0], ogrids[1], high, low, rs.WEIGHTS_3D,
                                                  target, pose)
        node = csm.NodeData3D(high, low, np.zeros(8, np.float32))
        r, jac, sums = csm.ceres_evaluate_3d(device[0], device[1], node, opts, target, pose)
        assert r.shape == ref_r.shape and jac.shape == ref_j.shape
        dev_r, dev_j = np.abs(r - ref_r).max(), np.abs(jac - ref_j).max()
        assert sums[0] == pytest.approx(float((r * r).sum()), rel=1e-12)
        part = _sums_within_rounding(sums, r, jac, name)
        print(f"3D {name}: residuals {dev_r:.3e} Jacobian {dev_j:.3e} "
              f"sums {part:.2f} of their bound")
        assert dev_r <= ROW_BOUND and dev_j <= ROW_BOUND, (name, dev_r, dev_j)
        worst = max(worst, dev_r, dev_j)
    print(f"3D: largest deviation from the oracle's rows {worst:.3e}")


def test_3d_evaluate_rejects_bad_input(csm, grids3d):
    device, _ = grids3d
    node = csm.NodeData3D(np.zeros((2, 3), np.float32), np.zeros((1, 3), np.float32),
                          np.zeros(8, np.float32))
    ident = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))
    with pytest.raises(csm.CsmError):
        csm.ceres_evaluate_3d(device[0], device[1], node, csm.CeresOptions3D.make(0.0), ident, ident)
    with pytest.raises(csm.CsmError):
        csm.ceres_evaluate_3d(device[0], device[1], node, csm.CeresOptions3D.make(), ident,
                              ((0.0, float("inf"), 0.0), ident[1]))
    empty = csm.NodeData3D(np.zeros((0, 3), np.float32), np.zeros((1, 3), np.float32),
                           np.zeros(8, np.float32))
    with pytest.raises(csm.CsmError):
        csm.ceres_evaluate_3d(device[0], device[1], empty, csm.CeresOptions3D.make(), ident, ident)


def _qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def test_3d_refinement_matches_oracle_from_tilted_starts(csm, oracle):
    """test_ceres3d.py's batch with the start turned about all three axes
    (roll, pitch and yaw of sigma 0.02 rad), so that the rotation columns that
    multiply q.x and q.y act from the first iteration."""
    world3 = csm.SyntheticWorld3D(num_nodes=8, num_submaps=2, seed=11)
    opts = (5.0, 30.0, 10.0, 1.0, 10)
    grids, ogrids = [], []
    for s in range(world3.num_submaps):
        grids.append(csm.HybridGrid(world3.high_resolution, *world3.high_cells[s]))
        grids.append(csm.HybridGrid(world3.low_resolution, *world3.low_cells[s]))
        hg = oracle.hybrid_grid(world3.high_resolution)
        hg.set_values(*world3.high_cells[s])
        lg = oracle.hybrid_grid(world3.low_resolution)
        lg.set_values(*world3.low_cells[s])
        ogrids.append((hg, lg))
    nodes = [world3.node(i) for i in range(world3.num_nodes)]
    rng = np.random.default_rng(4)
    items = []
    for i in range(world3.num_nodes):
        s = i % world3.num_submaps
        t, q = world3.node_in_submap(i, s)
        tt = tuple(float(v) for v in np.asarray(t) + rng.normal(0, 0.05, 3))
        qq = tuple(float(v) for v in q)
        for axis in range(3):  # roll, pitch, yaw
            a = rng.normal(0, 0.02)
            dq = [math.cos(a / 2), 0.0, 0.0, 0.0]
            dq[1 + axis] = math.sin(a / 2)
            qq = _qmul(dq, qq)
        assert qq[1] != 0.0 and qq[2] != 0.0
        items.append((2 * s, 2 * s + 1, i, (tt, qq), tt))
    poses, iters = csm.ceres_refine_batch_3d(grids, nodes, items, csm.CeresOptions3D.make(*opts))
    for k, (hgi, _, nd, (tt, qq), tgt) in enumerate(items):
        hg, lg = ogrids[hgi // 2]
        (rt, rq), rit = oracle.ceres3d_match(hg, lg, world3.high[nd], world3.low[nd], opts, tgt,
                                             tt, qq)
        print(f"3D refine item {k}: t {np.abs(np.subtract(poses[k][0], rt)).max():.3e} "
              f"q {np.abs(np.subtract(poses[k][1], rq)).max():.3e} ({iters[k]} / {rit} iterations)")
        assert np.allclose(poses[k][0], rt, atol=1e-6), (k, poses[k], rt)
        assert np.allclose(poses[k][1], rq, atol=1e-6), (k, poses[k], rq)
        assert abs(int(iters[k]) - rit) <= 1
