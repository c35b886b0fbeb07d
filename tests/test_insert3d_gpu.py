"""GPU: RangeDataInserter3D::Insert on device-resident HybridGrids
(csm_hybrid_grid_insert / _insert_batch, csrc/insert3d.hip) against the
oracle's line-by-line restatement (oracle/grid3d.cc).

"Same grid" everywhere means: csm_hybrid_grid_info equals (the box of the
oracle grid's cells, its DynamicGrid size) and csm_hybrid_grid_read equals the
oracle's cells scattered into that box, byte for byte. No comparison here has a
tolerance, except the reference test's own EXPECT_NEAR on the fixture's stated
probabilities, which is kept next to the exact comparison."""
import math

import numpy as np
import pytest

import insert3d_support as sup

pytestmark = pytest.mark.gpu

RES = 0.1


def empty_grid(csm, resolution):
    return csm.HybridGrid(resolution, np.zeros((0, 3), np.int32), np.zeros(0, np.uint16))


def gpu_grid(csm, og):
    ijk, v = og.cells()
    return csm.HybridGrid(og.resolution, ijk, v, grid_size=og.grid_size)


def fresh(csm, oracle, resolution=RES):
    return empty_grid(csm, resolution), oracle.hybrid_grid(resolution)


def insert_both(dev, ora, origin, returns, hit=0.55, miss=0.49, free=2):
    dev.insert(origin, returns, hit, miss, free)
    ora.insert(origin, returns, hit, miss, free)


def cell_points(cells, resolution=RES):
    """A point well inside each cell (its centre in float)."""
    return (np.asarray(cells, np.float32) * np.float32(resolution)).astype(np.float32)


# ---- 1. the reference's own fixture ---------------------------------------
FIXTURE_ORIGIN = np.array([0, 0, -4], np.float32)
FIXTURE_RETURNS = np.array([[-3, -1, 4], [-2, 0, 4], [-1, 1, 4], [0, 2, 4]], np.float32)


def test_reference_fixture(csm, oracle):
    """range_data_inserter_3d_test.cc:29-111: resolution 1, 0.7 / 0.4 / 1000."""
    dev, ora = fresh(csm, oracle, 1.0)
    insert_both(dev, ora, FIXTURE_ORIGIN, FIXTURE_RETURNS, 0.7, 0.4, 1000)
    sup.assert_same_grid(dev, ora, "fixture")
    misses = np.array([[0, 0, -4], [0, 0, -3], [0, 0, -2]], np.int32)
    hits = FIXTURE_RETURNS.astype(np.int32)
    pm, ph = dev.get_probability(misses), dev.get_probability(hits)
    for c, p in zip(misses, pm):
        assert p == np.float32(ora.probability(*[int(v) for v in c]))
        assert abs(p - 0.4) < 1e-4
    for c, p in zip(hits, ph):
        assert p == np.float32(ora.probability(*[int(v) for v in c]))
        assert abs(p - 0.7) < 1e-4
    # Every other cell of the z = 4 plane is unknown (:103-110).
    o, d, _ = dev.info()
    plane = dev.values()[4 - o[2]]
    known = {(x + o[0], y + o[1]) for y, x in zip(*np.nonzero(plane))}
    assert known == {(int(h[0]), int(h[1])) for h in hits}


def test_reference_fixture_repeated_to_saturation(csm, oracle):
    """ProbabilityProgression-style: the same cloud 20 times, compared after
    every insert, walks both tables up to their clamps."""
    dev, ora = fresh(csm, oracle, 1.0)
    for k in range(20):
        insert_both(dev, ora, FIXTURE_ORIGIN, FIXTURE_RETURNS, 0.7, 0.4, 1000)
        sup.assert_same_grid(dev, ora, f"repeat {k}")
    v = dev.values()
    assert v.max() == 32767 and v[v > 0].min() == 1  # both clamps were reached


# ---- 2. edge rays ----------------------------------------------------------
def tie_coordinate(k, resolution=RES):
    """A float p with p / resolution == k + 0.5 (k >= 0) exactly in float, so
    GetCellIndex's lround sees a tie; mirrored for the negative side."""
    res = np.float32(resolution)
    want = np.float32(k + 0.5)
    p = np.float32(want * res)
    for cand in (p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(1e9))):
        if np.float32(cand / res) == want:
            return np.float32(cand)
    raise AssertionError("no float lands on the tie")


def edge_cases():
    org = np.array([0.12, 0.11, 0.09], np.float32)  # cell (1, 1, 1)
    cases = {
        "same_cell": (org, np.array([[0.13, 0.08, 0.12]], np.float32)),
        "one_sample": (org, cell_points([[2, 1, 1]])),
        "two_samples": (org, cell_points([[3, 0, 2]])),
        "negative_one_axis": (org, cell_points([[-7, 3, 2]])),
        "negative_two_axes": (org, cell_points([[-5, -6, 9]])),
        "negative_three_axes": (org, cell_points([[-4, -7, -9]])),
        "many_in_one_cell": (org, np.repeat(cell_points([[6, -3, 4]]), 64, 0) +
                             np.linspace(-0.03, 0.03, 64, dtype=np.float32)[:, None]),
        "empty": (org, np.zeros((0, 3), np.float32)),
    }
    t = tie_coordinate(4)
    ties = []
    for axis in range(3):
        for sign in (1, -1):
            p = np.array([0.31, -0.22, 0.13], np.float32)
            p[axis] = sign * t
            ties.append(p)
    cases["ties"] = (org, np.array(ties, np.float32))
    # One ray's miss cell is the other's hit cell: hit (6, 1, 1) has misses at
    # (5, 1, 1), (4, 1, 1), ...; the other ray hits (5, 1, 1).
    a, b = cell_points([[6, 1, 1]])[0], cell_points([[5, 1, 1]])[0]
    cases["hit_wins_ab"] = (org, np.array([a, b], np.float32))
    cases["hit_wins_ba"] = (org, np.array([b, a], np.float32))
    return cases


@pytest.mark.parametrize("free", [2, 5])
def test_edge_rays(csm, oracle, free):
    cases = edge_cases()
    # The tie case is what it claims: lround rounds the half away from zero.
    probe = oracle.hybrid_grid(RES)
    ties = cases["ties"][1]
    idx = probe.cell_index(ties)
    for k, p in enumerate(ties):
        axis, sign = k // 2, (1 if k % 2 == 0 else -1)
        assert np.float32(abs(p[axis]) / np.float32(RES)) == np.float32(4.5)
        assert idx[k, axis] == sign * 5
    results = {}
    for name, (origin, returns) in cases.items():
        dev, ora = fresh(csm, oracle)
        info0 = dev.info()
        insert_both(dev, ora, origin, returns, 0.55, 0.49, free)
        sup.assert_same_grid(dev, ora, name)
        if name == "empty":
            assert dev.info() == info0
        results[name] = (dev.info(), dev.values().tobytes())
        # A second insert of the same rays on the now non-empty grid.
        insert_both(dev, ora, origin, returns, 0.55, 0.49, free)
        sup.assert_same_grid(dev, ora, name + " twice")
    assert results["hit_wins_ab"] == results["hit_wins_ba"]
    # 64 returns in one cell are one update: the same grid as one return.
    dev, ora = fresh(csm, oracle)
    insert_both(dev, ora, cases["many_in_one_cell"][0], cases["many_in_one_cell"][1][:1], 0.55,
                0.49, free)
    assert results["many_in_one_cell"] == (dev.info(), dev.values().tobytes())
    # same_cell: num_samples 0, the hit alone.
    assert np.count_nonzero(np.frombuffer(results["same_cell"][1], np.uint16)) == 1


def test_empty_insert_leaves_a_filled_grid_unchanged(csm, oracle):
    dev, ora = fresh(csm, oracle)
    rng = np.random.default_rng(3)
    insert_both(dev, ora, *sup.sphere_scan(rng, (0.1, 0.2, 0.3), 64, 0.5, 2.0))
    before = (dev.info(), dev.values().tobytes())
    dev.insert((5.0, 5.0, 5.0), np.zeros((0, 3), np.float32))
    assert (dev.info(), dev.values().tobytes()) == before
    sup.assert_same_grid(dev, ora)


# ---- 3. grid_size boundaries ------------------------------------------------
@pytest.mark.parametrize("cell,free,want", [
    ((63, 0, 0), 2, 128), ((0, -64, 0), 2, 128), ((0, 0, 64), 2, 256), ((-65, 0, 0), 2, 256),
    ((0, 64, 0), 0, 256), ((128, 0, 0), 2, 512), ((0, 0, -129), 1, 512), ((66, 0, 0), 1, 256),
])
def test_grid_size_boundaries(csm, oracle, cell, free, want):
    """DynamicGrid doubles while a touched index lies outside
    [-grid_size / 2, grid_size / 2), from 128; 128 on a 128 grid doubles twice.
    (66, 0, 0) with one free-space voxel: the miss cell (65, 0, 0) is outside
    too, the origin inside."""
    dev, ora = fresh(csm, oracle, 1.0)
    insert_both(dev, ora, (0.0, 0.0, 0.0), np.array([cell], np.float32), 0.55, 0.49, free)
    sup.assert_same_grid(dev, ora, str(cell))
    assert dev.info()[2] == want == ora.grid_size


def test_grid_size_grows_step_by_step(csm, oracle):
    dev, ora = fresh(csm, oracle, 1.0)
    for cell, want in [((63, 0, 0), 128), ((-64, 5, 0), 128), ((0, 64, 0), 256), ((0, 0, -65), 256),
                       ((100, 100, 100), 256), ((-129, 0, 0), 512)]:
        insert_both(dev, ora, (1.0, -1.0, 0.0), np.array([cell], np.float32), 0.55, 0.49, 3)
        sup.assert_same_grid(dev, ora, str(cell))
        assert dev.info()[2] == want


# ---- 4. brick growth in every direction ------------------------------------
@pytest.fixture(scope="module")
def scans():
    return sup.growth_scans()


def test_growth_from_empty(csm, oracle, scans):
    dev, ora = fresh(csm, oracle)
    dims = []
    for k, (origin, returns) in enumerate(scans):
        insert_both(dev, ora, origin, returns)
        sup.assert_same_grid(dev, ora, f"scan {k}")
        dims.append(dev.info()[1])
    assert all(b >= a for a, b in zip(np.prod(dims, 1)[:-1], np.prod(dims, 1)[1:]))
    assert max(dims[-1]) > 250  # 16 m at 0.1 m both ways


def test_growth_from_a_created_grid(csm, oracle, scans):
    ora = oracle.hybrid_grid(RES)
    rng = np.random.default_rng(2)
    ora.insert(*sup.sphere_scan(rng, (-1.0, 2.0, 0.5), 200, 0.5, 3.0), 0.7, 0.4, 5)
    dev = gpu_grid(csm, ora)
    sup.assert_same_grid(dev, ora, "created")
    for k, (origin, returns) in enumerate(scans):
        insert_both(dev, ora, origin, returns)
        sup.assert_same_grid(dev, ora, f"scan {k}")


# ---- 5. order independence ---------------------------------------------------
def test_order_independence(csm, oracle):
    """512 returns within 1.5 m at 0.1 m with five free-space voxels: most
    cells are touched by several rays, as hit and as miss."""
    rng = np.random.default_rng(17)
    origin, returns = sup.sphere_scan(rng, (0.03, -0.04, 0.02), 512, 0.2, 1.5)
    ora = oracle.hybrid_grid(RES)
    ora.insert(origin, returns, 0.55, 0.49, 5)
    ijk, _ = ora.cells()
    assert len(ijk) < 0.6 * 512 * 6  # the rays do overlap
    seen = set()
    for seed in (0, 1, 2):
        order = np.random.default_rng(seed).permutation(len(returns))
        dev = empty_grid(csm, RES)
        dev.insert(origin, returns[order], 0.55, 0.49, 5)
        sup.assert_same_grid(dev, ora, f"order {seed}")
        seen.add(dev.values().tobytes())
    assert len(seen) == 1


# ---- 6. errors leave the grid untouched ------------------------------------
def test_errors_leave_the_grid_untouched(csm, oracle):
    dev, ora = fresh(csm, oracle, 0.01)
    rng = np.random.default_rng(4)
    insert_both(dev, ora, *sup.sphere_scan(rng, (0.0, 0.0, 0.0), 64, 0.05, 0.3))
    before = (dev.info(), dev.values().tobytes())
    good = np.array([[0.1, 0.0, 0.0]], np.float32)
    # num_samples = 40000 >= 2^15: the reference's CHECK_LT.
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        dev.insert((0.0, 0.0, 0.0), np.concatenate([good, [[400.0, 0.0, 0.0]]]).astype(np.float32))
    assert (dev.info(), dev.values().tobytes()) == before
    # Rays of 16000 cells each whose box has 32000^3 > 2^31 cells.
    far = np.array([[160.0, 160.0, 160.0], [-160.0, -160.0, -160.0]], np.float32)
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        dev.insert((0.0, 0.0, 0.0), far)
    assert (dev.info(), dev.values().tobytes()) == before
    # Still usable.
    insert_both(dev, ora, (0.0, 0.0, 0.0), good)
    sup.assert_same_grid(dev, ora)


def test_batch_erange_in_the_second_grid_leaves_both_grids(csm):
    """A batch over two grids of a few cells: grid 0's job is valid and would
    grow its brick, grid 1's has a coordinate past 1e9 cells. CSM_ERANGE, and
    both grids keep their bricks: everything that can refuse a call comes
    before the first enqueue for any of its grids. (The handles' generation
    counters have no accessor; the brick and DynamicGrid size stand in.)"""
    grids = [empty_grid(csm, RES) for _ in range(2)]
    origin = np.zeros(3, np.float32)
    near = np.array([[0.3, 0.0, 0.0], [0.0, 0.3, 0.1], [-0.2, -0.2, 0.0]], np.float32)
    for g in grids:
        g.insert(origin, near)
    before = [(g.info(), g.values().tobytes()) for g in grids]
    grows = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.5], [-1.0, -1.0, 0.0]], np.float32)
    far = np.array([[0.3, 0.0, 0.0], [2.0e8, 0.0, 0.0], [0.0, 0.3, 0.0]], np.float32)
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        csm.HybridGrid.insert_batch(grids, [(origin, grows), (origin, far)], [(0, 0), (1, 1)])
    assert [(g.info(), g.values().tobytes()) for g in grids] == before
    # The valid job alone does grow its grid.
    grids[0].insert(origin, grows)
    assert grids[0].info()[1] != before[0][0][1]


# ---- 7. touched-cell scaling --------------------------------------------------
def test_apply_pass_visits_touched_cells_only(csm, oracle):
    """64 short rays into a brick of 200^3 cells: the FinishUpdate pass looks at
    one cell per return and per miss position (3 per ray here) and at nothing
    else, far below 1% of the brick volume."""
    free = 2
    rng = np.random.default_rng(9)
    origin, returns = sup.sphere_scan(rng, (0.5, -0.3, 0.2), 64, 0.4, 1.0)
    probe = oracle.hybrid_grid(RES)
    probe.insert(origin, returns, 0.55, 0.49, free)
    touched = len(probe.cells()[1])
    assert touched < 400
    corners = np.array([[-100, -100, -100], [99, 99, 99]], np.int32)
    dev = csm.HybridGrid(RES, corners, np.array([16000, 17000], np.uint16))
    ora = oracle.hybrid_grid(RES)
    ora.set_values(corners, np.array([16000, 17000], np.uint16))
    assert dev.info()[1] == (200, 200, 200)
    v0, u0 = dev.insert_stats()
    insert_both(dev, ora, origin, returns, 0.55, 0.49, free)
    v1, u1 = dev.insert_stats()
    sup.assert_same_grid(dev, ora)
    assert dev.info()[1] == (200, 200, 200)
    assert u1 - u0 == touched
    assert touched <= v1 - v0 <= 64 * (1 + free)
    assert v1 - v0 < 0.01 * 200 ** 3


# ---- 8. batch ---------------------------------------------------------------
def _quat(roll, pitch, yaw):
    cr, sr = math.cos(roll / 2), math.sin(roll / 2)
    cp, sp = math.cos(pitch / 2), math.sin(pitch / 2)
    cy, sy = math.cos(yaw / 2), math.sin(yaw / 2)
    q = np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                  cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], np.float32)
    return [float(v) for v in q]


def test_batch(csm, oracle):
    rng = np.random.default_rng(21)
    scans = [sup.sphere_scan(rng, (0.25 * s, -0.5 * s, 0.125 * s), 300, 0.5, 6.0) for s in range(3)]
    # Scan 2 carries a return at exactly max_range from its (dyadic) origin on
    # the y axis, and one just past it.
    max_range = 3.0
    o2, r2 = scans[2]
    r2[0] = o2 + np.array([0, max_range, 0], np.float32)
    r2[1] = o2 + np.array([0, np.nextafter(np.float32(max_range), np.float32(10)), 0], np.float32)
    assert sup.oracle_norm(r2[0] - o2) == max_range
    assert sup.oracle_norm(r2[1] - o2) > max_range
    tf_a = ([0.5, -1.25, 0.75], _quat(0.0, 0.0, 0.6))
    tf_b = ([-2.0, 0.5, 0.25], _quat(0.2, -0.15, -1.1))
    resolutions = [0.1, 0.45, 0.1, 0.45]
    jobs = []
    for s in range(3):
        jobs += [(0, s, tf_a, max_range), (1, s, tf_a, None), (2, s, tf_b, max_range),
                 (3, s, tf_b, None)]
    jobs.append((0, 2, None, max_range))  # the exact-range case, no transform
    devs = [empty_grid(csm, r) for r in resolutions]
    csm.HybridGrid.insert_batch(devs, scans, jobs, 0.55, 0.49, 2)
    oras = [oracle.hybrid_grid(r) for r in resolutions]
    singles = [empty_grid(csm, r) for r in resolutions]
    dropped = 0
    for g, s, tf, mr in jobs:
        pose = None if tf is None else sup.pose7f(*tf)
        origin, returns = sup.oracle_job(scans[s][0], scans[s][1], pose, mr)
        if tf is None:
            assert len(returns) < 300 and np.array_equal(returns[0], r2[0])  # kept: `<=`
            assert not any(np.array_equal(p, r2[1]) for p in returns)
        dropped += 300 - len(returns)
        oras[g].insert(origin, returns, 0.55, 0.49, 2)
        singles[g].insert(origin, returns, 0.55, 0.49, 2)  # host-side transform and filter
    for g in range(4):
        sup.assert_same_grid(devs[g], oras[g], f"batch grid {g}")
        sup.assert_same_grid(singles[g], oras[g], f"single grid {g}")
        assert devs[g].info() == singles[g].info()
        assert devs[g].values().tobytes() == singles[g].values().tobytes()
    assert dropped > 100  # max_range did filter the high-resolution jobs


def test_two_jobs_on_one_grid_equal_two_inserts(csm, oracle):
    rng = np.random.default_rng(22)
    a = sup.sphere_scan(rng, (0.0, 0.0, 0.0), 256, 0.3, 2.0)
    b = sup.sphere_scan(rng, (0.2, 0.1, -0.1), 256, 0.3, 2.5)
    one = empty_grid(csm, RES)
    csm.HybridGrid.insert_batch([one], [a, b], [(0, 0), (0, 1), (0, 0)], 0.55, 0.49, 3)
    two, ora = fresh(csm, oracle)
    for scan in (a, b, a):
        insert_both(two, ora, scan[0], scan[1], 0.55, 0.49, 3)
    sup.assert_same_grid(one, ora)
    assert one.values().tobytes() == two.values().tobytes()


# ---- 9. consumers see inserts --------------------------------------------------
def test_consumers_see_inserts(csm, oracle):
    """The stale-cache test: the matcher runs between the inserts, so its
    padded copies of the probability brick must follow every insert."""
    rng = np.random.default_rng(31)
    high, ohigh = fresh(csm, oracle, 0.1)
    low, olow = fresh(csm, oracle, 0.45)
    m = csm.RealTimeCorrelativeScanMatcher3D(
        csm.RealTimeCorrelativeScanMatcherOptions(0.1, math.radians(1.0), 0.1, 0.1))
    for k in range(3):
        origin, returns = sup.sphere_scan(rng, (0.2 * k, -0.1 * k, 0.05 * k), 300, 1.0, 2.0 + k)
        for dev, ora in ((high, ohigh), (low, olow)):
            insert_both(dev, ora, origin, returns, 0.55, 0.49, 2)
        ref = gpu_grid(csm, ohigh)
        assert high.info() == ref.info()
        cloud = returns[:30] - origin
        initial = ((float(origin[0]) + 0.03, float(origin[1]) - 0.02, float(origin[2]) + 0.01),
                   (math.cos(0.002), 0.0, 0.0, math.sin(0.002)))
        got = m.Match(initial, cloud, high)
        want = m.Match(initial, cloud, ref)
        assert np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes(), (k, got, want)
        assert got[1] == want[1], (k, got, want)
        o, d, _ = high.info()
        idx = (rng.integers(-2, np.array(d) + 2, (64, 3)) + np.array(o)).astype(np.int32)
        idx[:32] = ohigh.cells()[0][rng.integers(0, len(ohigh.cells()[0]), 32)]
        assert high.get_probability(idx).tobytes() == ref.get_probability(idx).tobytes()
        pts = (idx + rng.uniform(-0.5, 0.5, (64, 3))) * 0.1
        assert high.interpolate(pts).tobytes() == ref.interpolate(pts).tobytes()
    opts = csm.FastCorrelativeScanMatcherOptions3D(5, 3, 0.1, 0.15, 0.8, 0.8, 0.3)
    hist = np.zeros(10, np.float32)
    got = csm.FastCorrelativeScanMatcher3D(high, low, hist, opts)
    want = csm.FastCorrelativeScanMatcher3D(gpu_grid(csm, ohigh), gpu_grid(csm, olow), hist, opts)
    for level in range(5):
        (go, gb), (wo, wb) = got.read_level(level), want.read_level(level)
        assert tuple(go) == tuple(wo) and gb.shape == wb.shape, level
        assert gb.tobytes() == wb.tobytes(), level
