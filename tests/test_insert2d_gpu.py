"""GPU: range-data insertion into device-resident probability grids against the
oracle (tests/cpp/oracle_insert_shim.cc over oracle/): the pixel mask, the
inserter with growth, hit priority, batches, Finish, and the two matchers fed
from the device grid. Every comparison is exact."""
import ctypes as C
import math

import numpy as np
import pytest

import insert2d_support as sup

pytestmark = pytest.mark.gpu

HIT, MISS = 0.55, 0.49


# ---- RayToPixelMask ----------------------------------------------------------

def _assert_masks_equal(csm, rays, scale):
    rays = np.asarray(rays, np.int32).reshape(-1, 4)
    got = csm.ray_to_pixel_mask(rays, scale)
    assert len(got) == len(rays)
    for ray, g in zip(rays, got):
        want = sup.oracle_mask(ray, scale)
        assert np.array_equal(g, want), (ray.tolist(), g.tolist(), want.tolist())


def test_mask_reference_cases(csm):
    """The eight cases of ray_to_pixel_mask_test.cc at scale 1, and what the
    reference expects of each (SingleCell, AxisAligned, Diagonal, Steep, Flat,
    and reversals)."""
    x_axis = [(1, 1), (2, 1), (3, 1)]
    y_axis = [(1, 1), (1, 2), (1, 3)]
    rising = [(1, 1), (2, 2), (3, 3)]
    falling = [(1, 3), (2, 2), (3, 1)]
    cases = {
        (1, 1, 1, 1): [(1, 1)],                                      # SingleCell
        (1, 1, 3, 1): x_axis, (3, 1, 1, 1): x_axis,                  # AxisAlignedX
        (1, 1, 1, 3): y_axis, (1, 3, 1, 1): y_axis,                  # AxisAlignedY
        (1, 1, 3, 3): rising, (3, 3, 1, 1): rising,                  # Diagonal
        (1, 3, 3, 1): falling, (3, 1, 1, 3): falling,
        (1, 1, 2, 5): [(1, 1), (1, 2), (1, 3), (2, 3), (2, 4), (2, 5)],   # SteepLine
        (1, 1, 2, 4): [(1, 1), (1, 2), (2, 3), (2, 4)],
        (1, 1, 5, 2): [(1, 1), (2, 1), (3, 1), (3, 2), (4, 2), (5, 2)],   # FlatLine
        (1, 1, 4, 2): [(1, 1), (2, 1), (3, 2), (4, 2)],
    }
    rays = list(cases)
    got = csm.ray_to_pixel_mask(rays, 1)
    for ray, g in zip(rays, got):
        want = sup.oracle_mask(ray, 1)
        assert np.array_equal(g, want), (ray, g.tolist(), want.tolist())
        assert list(map(tuple, g.tolist())) == cases[ray], ray


def test_mask_random_rays_scale_1000(csm):
    """4096 seeded rays with subpixel endpoints in [0, 64000)^2: a 64 x 64 cell
    grid, the smallest with long shallow, long steep and same-column rays."""
    rng = np.random.default_rng(20240607)
    rays = rng.integers(0, 64000, (4096, 4)).astype(np.int32)
    rays[:64, 2] = rays[:64, 0] // 1000 * 1000 + rng.integers(0, 1000, 64)  # same column
    _assert_masks_equal(csm, rays, 1000)


def _corner_rays():
    rays = []
    a = b = 20
    for sx in (-1, 1):
        for sy in (-1, 1):
            for k in range(1, 9):
                for r in (0, 500, 999):
                    rays.append((1000 * a + r, 1000 * b + r, 1000 * (a + sx * k) + r,
                                 1000 * (b + sy * k) + r))
                # 1:2 and 2:1 slopes through cell centres.
                rays.append((1000 * a + 500, 1000 * b + 500, 1000 * (a + sx * k) + 500,
                             1000 * (b + 2 * sy * k) + 500))
                rays.append((1000 * a + 500, 1000 * b + 500, 1000 * (a + 2 * sx * k) + 500,
                             1000 * (b + sy * k) + 500))
    return np.asarray(rays, np.int32)


def test_mask_exact_corners(csm):
    """Rays through exact cell corners (sub_y == denominator): the walk steps
    diagonally and the two side cells stay out of the mask."""
    rays = _corner_rays()
    fired = 0
    for ray in rays:
        want = sup.oracle_mask(ray, 1000)
        four_connected = (abs(ray[2] // 1000 - ray[0] // 1000) +
                          abs(ray[3] // 1000 - ray[1] // 1000) + 1)
        fired += len(want) < four_connected
    assert fired >= 32, fired  # the oracle alone: the corner rule fired
    _assert_masks_equal(csm, rays, 1000)


# ---- insertion ---------------------------------------------------------------

def _reference_scan():
    """range_data_inserter_2d_test.cc:49-59."""
    ret = np.array([[-3.5, 0.5, 0], [-2.5, 1.5, 0], [-1.5, 2.5, 0], [-0.5, 3.5, 0]], np.float32)
    return (np.array([-0.5, 0.5, 0], np.float32), ret, np.zeros((0, 3), np.float32))


def _probability(csm, cells):
    scale = (csm.K_MAX_CORRESPONDENCE_COST - csm.K_MIN_CORRESPONDENCE_COST) / 32766.0
    cc = cells.astype(np.float64) * scale + (csm.K_MIN_CORRESPONDENCE_COST - scale)
    return 1.0 - cc


def test_reference_test_grid(csm, oracle):
    """range_data_inserter_2d_test.cc:31-133: InsertPointCloud's states, then
    ProbabilityProgression after 1001 inserts; byte-equal to the oracle at
    both points."""
    limits = (1.0, 1.0, 5.0, 5, 5)
    dev = csm.DeviceProbabilityGrid(*limits)
    ora = sup.OracleGrid(oracle, limits)
    scan = _reference_scan()
    dev.insert(*scan, hit_probability=0.7, miss_probability=0.4)
    ora.insert(scan, 0.7, 0.4, True)
    sup.assert_same_grid(dev, ora, "one insert")
    host = dev.to_host()
    assert (host.max_x, host.max_y, host.num_x_cells, host.num_y_cells) == (1.0, 5.0, 5, 5)
    U, M, H = 0, 1, 2
    expected_states = [[U, U, U, U, U], [U, H, M, M, M], [U, U, H, M, M], [U, U, U, H, M],
                       [U, U, U, U, H]]
    prob = _probability(csm, host.cells)
    for row in range(5):
        for column in range(5):
            # cell_index (row, column) is cell x = row, y = column: cells[y, x].
            v, p = host.cells[column, row], prob[column, row]
            state = expected_states[column][row]
            if state == U:
                assert v == 0
            else:
                assert v != 0 and abs(p - (0.4 if state == M else 0.7)) < 1e-4, (row, column, p)

    def cell_of(x, y):  # MapLimits::GetCellIndex
        return (round((5.0 - y) / 1.0 - 0.5), round((1.0 - x) / 1.0 - 0.5))
    for _ in range(1000):
        dev.insert(*scan, hit_probability=0.7, miss_probability=0.4)
        ora.insert(scan, 0.7, 0.4, True)
    sup.assert_same_grid(dev, ora, "1001 inserts")
    prob = _probability(csm, dev.to_host().cells)
    hx, hy = cell_of(-3.5, 0.5)
    mx, my = cell_of(-2.5, 0.5)
    assert abs(prob[hy, hx] - csm.K_MAX_PROBABILITY) < 1e-3
    assert abs(prob[my, mx] - csm.K_MIN_PROBABILITY) < 1e-3


@pytest.mark.parametrize("free_space", [True, False])
def test_growth_sequence(csm, oracle, free_space):
    """Eight scans into the kInitialSubmapSize grid, which grows 100 -> 800 a
    side over three inserts: limits and cells equal the oracle's after every
    insert."""
    dev = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
    ora = sup.OracleGrid(oracle, sup.INITIAL_LIMITS)
    sides = []
    for i, scan in enumerate(sup.growth_scans()):
        dev.insert(*scan, hit_probability=HIT, miss_probability=MISS,
                   insert_free_space=free_space)
        ora.insert(scan, HIT, MISS, free_space)
        sup.assert_same_grid(dev, ora, f"scan {i}")
        sides.append(dev.limits().num_x_cells)
    assert sides[0] == 100 and sides[-1] == 800 and len(set(sides)) == 4, sides


def test_hit_priority_and_once_per_scan(csm, oracle):
    """16 returns share one cell, and 16 further rays pass through cells that
    hold a return: a hit wins over a miss, and a cell is updated once."""
    origin = np.array([0.012, 0.013, 0], np.float32)
    shared = np.tile(np.array([[1.012, 0.013, 0]], np.float32), (16, 1))
    shared[:, 0] += np.linspace(0, 0.03, 16, dtype=np.float32)  # all in one 0.05 m cell
    near = np.zeros((16, 3), np.float32)    # returns along a line ...
    beyond = np.zeros((16, 3), np.float32)  # ... and returns behind them on the same rays
    for i in range(16):
        ang = 0.5 + 0.05 * i
        near[i, :2] = origin[:2] + 0.8 * np.array([math.cos(ang), math.sin(ang)], np.float32)
        beyond[i, :2] = origin[:2] + 1.6 * np.array([math.cos(ang), math.sin(ang)], np.float32)
    scan = (origin, np.concatenate([shared, near, beyond]), np.zeros((0, 3), np.float32))
    dev = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
    ora = sup.OracleGrid(oracle, sup.INITIAL_LIMITS)
    for i in range(2):
        dev.insert(*scan, hit_probability=HIT, miss_probability=MISS)
        ora.insert(scan, HIT, MISS, True)
        sup.assert_same_grid(dev, ora, f"insert {i}")
    cells = dev.to_host().cells
    hit2 = csm.inserter2d_lookup_table(HIT)
    twice = hit2[hit2[0] - 32768] - 32768
    assert (cells == twice).sum() >= 17  # the shared cell and the near returns: two hits each


def _batch_scans():
    scans = sup.growth_scans(seed=11, num_scans=24, num_returns=96, num_misses=24)
    # Interleaved: scan i goes into grid i % 4, so each grid takes 6.
    return scans, [i % 4 for i in range(24)]


def test_batch_equals_single_inserts_and_oracle(csm, oracle):
    scans, grid_of = _batch_scans()

    def run_batch():
        grids = [csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS) for _ in range(4)]
        csm.DeviceProbabilityGrid.insert_batch(grids, grid_of, scans, HIT, MISS, True)
        return [g.to_host() for g in grids]
    first = run_batch()
    second = run_batch()
    for g in range(4):
        single = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
        ora = sup.OracleGrid(oracle, sup.INITIAL_LIMITS)
        for scan, gi in zip(scans, grid_of):
            if gi == g:
                single.insert(*scan, hit_probability=HIT, miss_probability=MISS)
                ora.insert(scan, HIT, MISS, True)
        sup.assert_same_grid(single, ora, f"grid {g} single inserts")
        want = single.to_host()
        for got in (first[g], second[g]):
            assert sup.limits_tuple(got.limits()) == sup.limits_tuple(want.limits())
            assert np.array_equal(got.cells, want.cells)


@pytest.fixture(scope="module")
def inserted(csm, oracle):
    """The eight-scan growth sequence in a device grid and in the oracle."""
    dev = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
    ora = sup.OracleGrid(oracle, sup.INITIAL_LIMITS)
    scans = sup.growth_scans()
    for scan in scans:
        dev.insert(*scan, hit_probability=HIT, miss_probability=MISS)
        ora.insert(scan, HIT, MISS, True)
    return dev, ora, scans


def test_insert_errors(csm):
    dev = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
    before = dev.to_host()
    origin = np.zeros(3, np.float32)
    far = np.array([[1000.0, 0, 0]], np.float32)  # 20000 cells away: past 8192 a side
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        dev.insert(origin, far)
    bad = np.array([[1.0, float("nan"), 0]], np.float32)
    with pytest.raises(csm.CsmError, match=r"\(-1\)"):
        dev.insert(origin, bad)
    after = dev.to_host()
    assert sup.limits_tuple(after.limits()) == sup.limits_tuple(before.limits())
    assert np.array_equal(after.cells, before.cells)


def test_batch_erange_in_the_second_grid_leaves_both_grids(csm):
    """A batch over two grids of 8 x 8 cells: grid 0's scan is valid and would
    double it, grid 1's needs more than 8192 cells a side. CSM_ERANGE, and both
    grids keep their limits and cells: everything that can refuse a call comes
    before the first enqueue for any of its grids. (The handles' generation
    counters have no accessor; the limits stand in for them.)"""
    limits = (0.05, 0.2, 0.2, 8, 8)
    grids = [csm.DeviceProbabilityGrid(*limits) for _ in range(2)]
    origin = np.zeros(3, np.float32)
    near = np.array([[0.1, 0.0, 0], [0.0, 0.12, 0], [-0.1, -0.1, 0]], np.float32)
    for g in grids:
        g.insert(origin, near, hit_probability=HIT, miss_probability=MISS)
    before = [g.to_host() for g in grids]
    assert all((b.cells != 0).any() for b in before)
    grows = np.array([[0.3, 0.0, 0], [0.0, 0.3, 0], [-0.3, -0.3, 0]], np.float32)
    far = np.array([[0.1, 0.0, 0], [1000.0, 0.0, 0], [0.0, 0.1, 0]], np.float32)
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        csm.DeviceProbabilityGrid.insert_batch(grids, [0, 1], [(origin, grows), (origin, far)],
                                               HIT, MISS, True)
    for g, b in zip(grids, before):
        after = g.to_host()
        assert sup.limits_tuple(after.limits()) == sup.limits_tuple(b.limits())
        assert np.array_equal(after.cells, b.cells)
    # The valid scan alone does grow its grid.
    grids[0].insert(origin, grows, hit_probability=HIT, miss_probability=MISS)
    assert grids[0].limits().num_x_cells == 16


def test_finish(csm, oracle, inserted):
    """Finish crops to the oracle's ComputeCroppedGrid; a never-inserted grid
    finishes to 1 x 1; an insert after Finish is CSM_EINVAL."""
    _, _, scans = inserted
    dev = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
    ora = sup.OracleGrid(oracle, sup.INITIAL_LIMITS)
    for scan in scans:
        dev.insert(*scan, hit_probability=HIT, miss_probability=MISS)
        ora.insert(scan, HIT, MISS, True)
    dev.finish()
    ora.crop()
    sup.assert_same_grid(dev, ora, "finished")
    assert dev.limits().num_x_cells < 800
    with pytest.raises(csm.CsmError, match=r"\(-1\)"):
        dev.insert(*scans[0])
    empty = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
    empty.finish()
    ora_empty = sup.OracleGrid(oracle, sup.INITIAL_LIMITS)
    ora_empty.crop()
    sup.assert_same_grid(empty, ora_empty, "empty")
    lim = empty.limits()
    assert (lim.num_x_cells, lim.num_y_cells, lim.max_x, lim.max_y) == (1, 1, 2.5, 2.5)


def test_fast2d_create_from_grid(csm, inserted):
    """Every pyramid level equals csm_fast2d_create on the read-back cells
    (depth 4), and MatchFullSubmap agrees in status, score bits and pose."""
    dev, _, scans = inserted
    opts = csm.FastCorrelativeScanMatcherOptions2D(1.0, math.radians(10.0), 4)
    from_dev = csm.FastCorrelativeScanMatcher2D(dev, opts)
    from_host = csm.FastCorrelativeScanMatcher2D(dev.to_host(), opts)
    for level in range(4):
        a, b = from_dev.read_level(level), from_host.read_level(level)
        assert a.shape == b.shape and np.array_equal(a, b), level
    origin, ret, _ = scans[3]
    cloud = ret - origin  # the scan in its own frame; the search finds the origin again
    ra = from_dev.MatchFullSubmap(cloud, 0.3)
    rb = from_host.MatchFullSubmap(cloud, 0.3)
    assert ra[0] == rb[0]
    assert np.float32(ra[1]).tobytes() == np.float32(rb[1]).tobytes()
    assert ra[2] == rb[2]


def test_rt2d_match_grid(csm, oracle):
    """csm_rt2d_match_grid equals csm_rt2d_match on the read-back cells before
    and after a further insert: the generation counter invalidates the
    converted grid."""
    scans = sup.growth_scans()
    dev = csm.DeviceProbabilityGrid(*sup.INITIAL_LIMITS)
    for scan in scans[:4]:
        dev.insert(*scan, hit_probability=HIT, miss_probability=MISS)
    rt = csm.RealTimeCorrelativeScanMatcher2D(csm.RealTimeCorrelativeScanMatcherOptions(
        0.3, math.radians(10.0), 1e-1, 1e-1))
    host_ctx = csm.Context(0)
    rt_host = csm.RealTimeCorrelativeScanMatcher2D(rt.options, host_ctx)
    origin, ret, _ = scans[3]
    cloud = ret - origin
    initial = (float(origin[0]) + 0.07, float(origin[1]) - 0.05, 0.02)
    results = []
    for step in range(2):
        got = rt.Match(initial, cloud, dev)
        want = rt_host.Match(initial, cloud, dev.to_host())
        assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes(), step
        assert got[1] == want[1], step
        results.append(got)
        if step == 0:
            for scan in scans[4:]:
                dev.insert(*scan, hit_probability=HIT, miss_probability=MISS)
    assert results[0][0] != results[1][0]  # the further inserts changed the grid under the cloud
    host_ctx.close()
