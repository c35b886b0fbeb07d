"""GPU: device-resident IntensityHybridGrids and
RangeDataInserter3D::Insert(range_data, grid, intensity_grid)
(csm_intensity_grid_*, csm_hybrid_grid_insert_intensities[_batch],
csrc/insert3d.hip) against the CPU restatement
(tests/cpp/oracle_intensity3d_shim.cc).

"Same intensity grid" means: csm_intensity_grid_info equals (the box of the
restatement's cells with count > 0, its DynamicGrid size), csm_intensity_grid_read
equals its sums and counts bit for bit, and csm_intensity_grid_get_intensity
equals its GetIntensity bit for bit over the box, one cell around it and far
away. No comparison here has a tolerance, except the reference test's own
EXPECT_NEAR, kept next to the exact comparison."""
import math

import numpy as np
import pytest

import insert3d_support as sup
import intensity3d_support as isup

pytestmark = pytest.mark.gpu

RES = 0.1
OPTS = (0.55, 0.49, 2)


def empty_grid(csm, resolution):
    return csm.HybridGrid(resolution, np.zeros((0, 3), np.int32), np.zeros(0, np.uint16))


def fresh(csm, resolution=RES):
    """(device HybridGrid, device intensity grid, restated intensity grid)."""
    return (empty_grid(csm, resolution), csm.IntensityHybridGrid(resolution),
            isup.OracleIntensityGrid(resolution))


def insert_both(hg, dev, ora, origin, returns, intensities, threshold, opts=OPTS):
    hg.insert(origin, returns, *opts, intensity_grid=dev, intensities=intensities,
              intensity_threshold=threshold)
    ora.insert(returns, intensities, threshold)


FIXTURE_ORIGIN = np.array([0, 0, -4], np.float32)
FIXTURE_RETURNS = np.array([[-3, -1, 4], [-2, 0, 4], [-1, 1, 4], [0, 2, 4]], np.float32)
FIXTURE_INTENSITIES = np.array([7, 8, 9, 10], np.float32)


def test_empty_grid(csm):
    dev = csm.IntensityHybridGrid(0.25)
    assert dev.info() == ((0, 0, 0), (0, 0, 0), 128)
    isup.assert_same_intensity_grid(dev, isup.OracleIntensityGrid(0.25), "empty")
    s, c = dev.read()
    assert s.size == 0 and c.size == 0


def test_reference_fixture(csm, oracle):
    """range_data_inserter_3d_test.cc:56-67, :113-133, and the HybridGrid next
    to it against the oracle's."""
    hg, dev, ora = fresh(csm, 1.0)
    ohg = oracle.hybrid_grid(1.0)
    insert_both(hg, dev, ora, FIXTURE_ORIGIN, FIXTURE_RETURNS, FIXTURE_INTENSITIES, 100.0,
                (0.7, 0.4, 1000))
    ohg.insert(FIXTURE_ORIGIN, FIXTURE_RETURNS, 0.7, 0.4, 1000)
    isup.assert_same_intensity_grid(dev, ora, "fixture")
    sup.assert_same_grid(hg, ohg, "fixture")
    assert dev.info() == ((-3, -1, 4), (4, 4, 1), 128)
    plane = [(x, y, 4) for x in range(-4, 5) for y in range(-4, 5)]
    got = dev.get_intensity(plane)
    for (x, y, _), v in zip(plane, got):
        want = 0.0 if (x < -3 or x > 0 or y != x + 2) else 10 + x
        assert abs(v - want) <= 1e-6, (x, y, v)


def test_threshold_edges(csm):
    hg, dev, ora = fresh(csm)
    pts = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [-0.3, 0.2, 0.1]], np.float32)
    above = np.nextafter(np.float32(100.0), np.float32(200.0))
    # Everything above the threshold: the grid stays empty, dims 0.
    insert_both(hg, dev, ora, (0, 0, 0), pts, [above, 150.0, 1e30], 100.0)
    assert dev.info() == ((0, 0, 0), (0, 0, 0), 128) and dev.device_bytes() == 0
    isup.assert_same_intensity_grid(dev, ora, "all above")
    # Equal to the threshold is inserted, the next float above it is not.
    insert_both(hg, dev, ora, (0, 0, 0), pts, [100.0, above, above], 100.0)
    isup.assert_same_intensity_grid(dev, ora, "edges")
    assert dev.info()[:2] == ((5, 5, 5), (1, 1, 1))
    s, c = dev.read()
    assert s.ravel().tolist() == [100.0] and c.ravel().tolist() == [1]
    # A cloud without intensities, and no returns at all.
    before = (dev.info(), dev.read()[0].tobytes(), dev.read()[1].tobytes())
    insert_both(hg, dev, ora, (0, 0, 0), pts, None, 100.0)
    hg.insert((0, 0, 0), np.zeros((0, 3), np.float32), *OPTS, intensity_grid=dev,
              intensities=np.zeros(0, np.float32), intensity_threshold=100.0)
    assert (dev.info(), dev.read()[0].tobytes(), dev.read()[1].tobytes()) == before
    # A negative and a zero intensity: count 1 with sum 0 is a known cell.
    insert_both(hg, dev, ora, (0, 0, 0), pts, [-3.5, 0.0, 0.0], 100.0)
    isup.assert_same_intensity_grid(dev, ora, "zero and negative")
    assert dev.info()[1] == (9, 4, 5)


def order_sensitive_scan():
    """64 returns into 3 cells, intensities from {2^24, 1, 3, 0.1}: the float
    sum of a cell depends on the order (test_intensity3d_host.py)."""
    rng = np.random.default_rng(41)
    cells = np.array([[2, -1, 3], [2, 0, 3], [-4, 5, 1]], np.int32)
    which = rng.integers(0, 3, 64)
    pts = (cells[which] * np.float32(RES)).astype(np.float32)
    pts += rng.uniform(-0.03, 0.03, (64, 3)).astype(np.float32)
    vals = rng.choice(np.array([16777216.0, 1.0, 3.0, 0.1], np.float32), 64)
    return pts, vals


def test_sum_is_in_returns_order_and_reproducible(csm):
    pts, vals = order_sensitive_scan()
    # The case can tell a wrong order: reversed returns give other bits.
    fwd, rev = isup.OracleIntensityGrid(RES), isup.OracleIntensityGrid(RES)
    fwd.insert(pts, vals, 1e9)
    rev.insert(pts[::-1], vals[::-1], 1e9)
    assert fwd.cells()[1].tobytes() != rev.cells()[1].tobytes()
    seen = set()
    for _ in range(3):
        hg, dev, ora = fresh(csm)
        insert_both(hg, dev, ora, (0.01, 0.02, 0.03), pts, vals, 1e9)
        isup.assert_same_intensity_grid(dev, ora, "order")
        s, c = dev.read()
        assert c.sum() == 64 and len(ora.cells()[0]) == 3
        seen.add((dev.info(), s.tobytes(), c.tobytes()))
    assert len(seen) == 1


def test_same_cell_in_two_consecutive_calls(csm):
    """The second call's sum continues from the first's: (old + a) + b."""
    hg, dev, ora = fresh(csm)
    p = np.repeat(np.array([[0.7, -0.2, 0.4]], np.float32), 3, 0)
    insert_both(hg, dev, ora, (0, 0, 0), p, [0.1, 16777216.0, 1.0], 1e9)
    isup.assert_same_intensity_grid(dev, ora, "first")
    insert_both(hg, dev, ora, (0, 0, 0), p[:2], [1.0, 3.0], 1e9)
    isup.assert_same_intensity_grid(dev, ora, "second")
    s, c = dev.read()
    assert c.ravel().tolist() == [5]
    want = np.float32(0.0)
    for v in [0.1, 16777216.0, 1.0, 1.0, 3.0]:
        want = np.float32(want + np.float32(v))
    assert s.ravel()[0] == want


def test_a_run_longer_than_a_workgroup(csm):
    """300 returns in one cell between two smaller runs. Sorted by cell (z,
    then y, then x) the run of 255 comes first, so the run of 300 starts at a
    256-thread block's last key and its thread walks through the whole next
    block into a third."""
    rng = np.random.default_rng(43)
    cells = np.concatenate([np.tile([[3, -2, 0]], (255, 1)), np.tile([[1, 1, 1]], (300, 1)),
                            np.tile([[-5, 4, 2]], (90, 1))]).astype(np.int32)
    order = rng.permutation(len(cells))
    pts = (cells[order] * np.float32(RES)).astype(np.float32)
    vals = rng.choice(np.array([16777216.0, 1.0, 3.0, 0.1], np.float32), len(cells))
    hg, dev, ora = fresh(csm)
    insert_both(hg, dev, ora, (0, 0, 0), pts, vals, 1e9)
    isup.assert_same_intensity_grid(dev, ora, "long run")
    assert sorted(dev.read()[1][dev.read()[1] > 0].tolist()) == [90, 255, 300]


@pytest.fixture(scope="module")
def scans():
    return sup.growth_scans()


def test_growth(csm, scans):
    """insert3d_support.growth_scans() (8 x 256 returns) with seeded
    intensities in [0, 255] and a threshold of 200: the brick grows in every
    direction. After every scan the intensity grid equals the restatement's and
    the HybridGrid's bytes equal those the entry point without intensities
    leaves (test_insert3d_gpu.py compares that one with the oracle)."""
    hg, dev, ora = fresh(csm)
    plain = empty_grid(csm, RES)
    kept = 0
    for k, (origin, returns) in enumerate(scans):
        vals = isup.seeded_intensities(len(returns), 100 + k)
        kept += int((vals <= 200).sum())
        insert_both(hg, dev, ora, origin, returns, vals, 200.0)
        plain.insert(origin, returns, *OPTS)
        isup.assert_same_intensity_grid(dev, ora, f"scan {k}")
        assert hg.info() == plain.info()
        assert hg.values().tobytes() == plain.values().tobytes()
    assert dev.read()[1].sum() == kept and 0.6 * 8 * 256 < kept < 8 * 256
    assert max(dev.info()[1]) > 250  # 16 m at 0.1 m both ways
    assert dev.device_bytes() >= 8 * int(np.prod(dev.info()[1]))


def test_grid_size_follows_the_inserted_returns_only(csm):
    """DynamicGrid grows for the cells that get an intensity, not for returns
    above the threshold."""
    hg, dev, ora = fresh(csm, 1.0)
    pts = np.array([[63, 0, 0], [0, 64, 0]], np.float32)
    insert_both(hg, dev, ora, (0, 0, 0), pts, [1.0, 500.0], 100.0)
    isup.assert_same_intensity_grid(dev, ora, "inside")
    assert dev.info()[2] == 128 and hg.info()[2] == 256
    insert_both(hg, dev, ora, (0, 0, 0), pts, [1.0, 50.0], 100.0)
    isup.assert_same_intensity_grid(dev, ora, "grown")
    assert dev.info()[2] == 256
    insert_both(hg, dev, ora, (0, 0, 0), np.array([[0, 0, -129]], np.float32), [2.0], 100.0)
    isup.assert_same_intensity_grid(dev, ora, "grown twice")
    assert dev.info()[2] == 512


def test_resolutions_may_differ(csm):
    """The intensity grid uses its own GetCellIndex, as in the reference."""
    hg = empty_grid(csm, 0.1)
    dev, ora = csm.IntensityHybridGrid(0.3), isup.OracleIntensityGrid(0.3)
    rng = np.random.default_rng(5)
    origin, returns = sup.sphere_scan(rng, (0.1, 0.1, 0.1), 200, 0.5, 2.0)
    insert_both(hg, dev, ora, origin, returns, isup.seeded_intensities(200, 6), 128.0)
    isup.assert_same_intensity_grid(dev, ora, "0.3 in 0.1")


def test_errors_leave_both_grids_untouched(csm):
    hg = empty_grid(csm, 1.0)
    dev, ora = csm.IntensityHybridGrid(0.01), isup.OracleIntensityGrid(0.01)
    rng = np.random.default_rng(4)
    origin, returns = sup.sphere_scan(rng, (0.0, 0.0, 0.0), 64, 0.05, 0.3)
    insert_both(hg, dev, ora, origin, returns, isup.seeded_intensities(64, 7), 300.0)

    def state():
        return (hg.info(), hg.values().tobytes(), dev.info(), dev.read()[0].tobytes(),
                dev.read()[1].tobytes())

    before = state()
    # 80^3 cells for the HybridGrid, 8000^3 > 2^31 for the intensity grid.
    far = np.array([[40.0, 40.0, 40.0], [-40.0, -40.0, -40.0]], np.float32)
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        hg.insert((0, 0, 0), far, *OPTS, intensity_grid=dev, intensities=[1.0, 2.0],
                  intensity_threshold=100.0)
    assert state() == before
    with pytest.raises(csm.CsmError, match=r"\(-1\)"):
        hg.insert((0, 0, 0), far, *OPTS, intensity_grid=dev, intensities=[1.0, float("nan")],
                  intensity_threshold=100.0)
    assert state() == before
    # Above the threshold the far returns reach the HybridGrid only.
    hg.insert((0, 0, 0), far, *OPTS, intensity_grid=dev, intensities=[101.0, 102.0],
              intensity_threshold=100.0)
    assert hg.info()[1] == (81, 81, 81)
    assert (dev.info(), dev.read()[0].tobytes(), dev.read()[1].tobytes()) == before[2:]
    isup.assert_same_intensity_grid(dev, ora, "after errors")


def _quat(roll, pitch, yaw):
    cr, sr = math.cos(roll / 2), math.sin(roll / 2)
    cp, sp = math.cos(pitch / 2), math.sin(pitch / 2)
    cy, sy = math.cos(yaw / 2), math.sin(yaw / 2)
    q = np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                  cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], np.float32)
    return [float(v) for v in q]


def oracle_job_with_intensities(origin, returns, intensities, pose7, max_range):
    """insert3d_support.oracle_job and the intensities of the returns it keeps
    (PointCloud::copy_if, point_cloud.h:60-84): oracle_job's own mask, found
    by running it on single returns."""
    org, kept = sup.oracle_job(origin, returns, pose7, max_range)
    mask = np.array([len(sup.oracle_job(origin, returns[i:i + 1], pose7, max_range)[1]) == 1
                     for i in range(len(returns))], bool)
    assert mask.sum() == len(kept)
    return org, kept, None if intensities is None else np.asarray(intensities, np.float32)[mask]


def test_batch(csm, oracle):
    """Two submaps x (high + low) grids, intensity grids on the high ones only,
    per-job transforms and max_range; scan 1 has no intensities."""
    rng = np.random.default_rng(21)
    scans = []
    for s in range(3):
        origin, returns = sup.sphere_scan(rng, (0.25 * s, -0.5 * s, 0.125 * s), 300, 0.5, 6.0)
        scans.append((origin, returns,
                      None if s == 1 else isup.seeded_intensities(300, 50 + s)))
    max_range = 3.0
    tf_a = ([0.5, -1.25, 0.75], _quat(0.0, 0.0, 0.6))
    tf_b = ([-2.0, 0.5, 0.25], _quat(0.2, -0.15, -1.1))
    resolutions = [0.1, 0.45, 0.1, 0.45]
    jobs = []
    for s in range(3):
        jobs += [(0, s, tf_a, max_range, 0), (1, s, tf_a, None, None),
                 (2, s, tf_b, max_range, 1), (3, s, tf_b, None, -1)]
    devs = [empty_grid(csm, r) for r in resolutions]
    plain = [empty_grid(csm, r) for r in resolutions]
    idevs = [csm.IntensityHybridGrid(0.1) for _ in range(2)]
    ioras = [isup.OracleIntensityGrid(0.1) for _ in range(2)]
    csm.HybridGrid.insert_batch(devs, scans, jobs, *OPTS, intensity_grids=idevs,
                                intensity_threshold=180.0)
    csm.HybridGrid.insert_batch(plain, [s[:2] for s in scans], [j[:4] for j in jobs], *OPTS)
    dropped = 0
    for g, s, tf, mr, ig in jobs:
        if ig is None or ig < 0:
            continue
        _, kept, vals = oracle_job_with_intensities(*scans[s], sup.pose7f(*tf), mr)
        dropped += 300 - len(kept)
        ioras[ig].insert(kept, vals, 180.0)
    assert dropped > 100
    for g in range(4):
        assert devs[g].info() == plain[g].info(), g
        assert devs[g].values().tobytes() == plain[g].values().tobytes(), g
    for ig in range(2):
        isup.assert_same_intensity_grid(idevs[ig], ioras[ig], f"intensity grid {ig}")
        assert idevs[ig].read()[1].sum() > 100


def test_two_jobs_on_one_grid_in_one_call(csm):
    """Jobs on one grid apply in array order: scan a, scan b, scan a again,
    with cells shared between them; equal to three single calls."""
    rng = np.random.default_rng(22)
    a = sup.sphere_scan(rng, (0.0, 0.0, 0.0), 256, 0.2, 0.6)
    b = sup.sphere_scan(rng, (0.05, 0.05, -0.05), 256, 0.2, 0.8)
    va = rng.choice(np.array([16777216.0, 1.0, 3.0, 0.1], np.float32), 256)
    vb = rng.choice(np.array([16777216.0, 1.0, 3.0, 0.1], np.float32), 256)
    one, ione = empty_grid(csm, RES), csm.IntensityHybridGrid(RES)
    csm.HybridGrid.insert_batch([one], [a + (va,), b + (vb,)],
                                [(0, 0, None, None, 0), (0, 1, None, None, 0),
                                 (0, 0, None, None, 0)], *OPTS, intensity_grids=[ione],
                                intensity_threshold=1e9)
    two, itwo, ora = fresh(csm)
    for scan, vals in ((a, va), (b, vb), (a, va)):
        insert_both(two, itwo, ora, scan[0], scan[1], vals, 1e9)
    isup.assert_same_intensity_grid(ione, ora, "batch")
    isup.assert_same_intensity_grid(itwo, ora, "singles")
    assert one.values().tobytes() == two.values().tobytes()
    counts = ione.read()[1]
    assert counts.max() >= 3 and counts.sum() == 3 * 256
