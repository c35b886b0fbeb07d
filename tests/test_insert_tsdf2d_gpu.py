"""GPU: TSDFRangeDataInserter2D on device-resident TSDF2D grids
(csm_tsdf_grid_*) against the oracle's restated inserter: limits equal and
both planes byte for byte after every insert, over inputs where the
first-writer rule and the sort's tie permutation decide thousands of cells;
batches, Finish, errors and the real-time matcher on the device planes."""
import ctypes as C

import numpy as np
import pytest

import tsdf_support as sup

pytestmark = pytest.mark.gpu

_INPUT_CACHE = {}


def _scans(name, shuffle=False):
    key = (name, shuffle)
    if key not in _INPUT_CACHE:
        s = sup.INPUTS[name]()
        _INPUT_CACHE[key] = sup.shuffled(s) if shuffle else s
    return _INPUT_CACHE[key]


def _insert_and_compare(csm, oracle, scans, options, what):
    dev = sup.new_device_grid(csm)
    ora = sup.OracleTSDF(oracle)
    for i, scan in enumerate(scans):
        dev.insert(scan[0], scan[1], options)
        ora.insert(scan, options)
        sup.assert_same_tsdf(dev, ora, (what, i))
    return dev, ora


@pytest.mark.parametrize("opt", sorted(sup.OPTION_SETS))
@pytest.mark.parametrize("name", sorted(sup.INPUTS))
def test_every_insert_equals_oracle(csm, oracle, name, opt):
    dev, ora = _insert_and_compare(csm, oracle, _scans(name), sup.OPTION_SETS[opt], (name, opt))
    _, tsd, _ = ora.get()
    assert (tsd != 0).sum() > 100  # the input does write cells under these options
    dev.close()


@pytest.mark.parametrize("name,opt", [("room", "C"), ("dup", "A")])
def test_shuffled_returns_equal_oracle_on_the_same_order(csm, oracle, name, opt):
    """The input order of the returns is observable (the first writer without
    a sort, the permutation among equivalent returns with it): the oracle's own
    cells differ between the two orders, and the device follows each."""
    options = sup.OPTION_SETS[opt]
    dev, ora = _insert_and_compare(csm, oracle, _scans(name, True), options, (name, opt, "shuf"))
    plain = sup.OracleTSDF(oracle)
    for scan in _scans(name):
        plain.insert(scan, options)
    (_, tsd_s, wgt_s), (_, tsd_p, wgt_p) = ora.get(), plain.get()
    assert ((tsd_s != tsd_p) | (wgt_s != wgt_p)).sum() > 100
    dev.close()


# tsdf_range_data_inserter_2d_test.cc:28-62: MapLimits(1., (1, 7), 8 x 1),
# truncation 2, max weight 10, and the fixture's options.
REF_LIMITS = (1.0, 1.0, 7.0, 8, 1)
REF_OPTIONS = (2.0, 10.0, 0, 2, 10.0, 0, 0, 0.0, 0.0)
REF_ORIGIN = np.array([-0.5, -0.5, 0.0], np.float32)
REF_POINT = np.array([[-0.5, 3.5, 0.0]], np.float32)
REF_TWO = np.array([[-0.5, 3.5, 0.0], [5.5, 3.5, 0.0]], np.float32)
REF_THREE = np.array([[-0.5, 3.5, 0.0], [5.5, 3.5, 0.0], [10.5, 3.5, 0.0]], np.float32)


def _ref_opts(**kw):
    names = ["truncation_distance", "maximum_weight", "update_free_space", "num_normal_samples",
             "sample_radius", "project", "exponent", "angle_bw", "distance_bw"]
    v = list(REF_OPTIONS)
    for k, x in kw.items():
        v[names.index(k)] = x
    return tuple(v)


REF_CASES = {
    "InsertPoint": (_ref_opts(), REF_POINT, 12),
    "InsertPointWithFreeSpaceUpdate": (_ref_opts(update_free_space=1), REF_POINT, 12),
    "InsertPointLinearWeight": (_ref_opts(exponent=1), REF_POINT, 1),
    "InsertPointQuadraticWeight": (_ref_opts(exponent=2), REF_POINT, 1),
    "InsertSmallAnglePointWithoutNormalProjection": (_ref_opts(), REF_THREE, 1),
    "InsertSmallAnglePointWitNormalProjection": (_ref_opts(project=1), REF_TWO, 1),
    "InsertPointsWithAngleScanNormalToRayWeight": (_ref_opts(angle_bw=10.0), REF_TWO, 1),
    "InsertPointsWithDistanceCellToHit": (_ref_opts(distance_bw=10.0), REF_POINT, 1),
}


@pytest.mark.parametrize("case", sorted(REF_CASES))
def test_reference_inserter_test_scans(csm, oracle, case):
    """The scans of the reference's own inserter tests, repeated inserts
    included (the weight saturates at the maximum)."""
    options, returns, repeats = REF_CASES[case]
    dev = sup.new_device_grid(csm, REF_LIMITS, 2.0, 10.0)
    ora = sup.OracleTSDF(oracle, REF_LIMITS, 2.0, 10.0)
    for i in range(repeats):
        dev.insert(REF_ORIGIN, returns, options)
        ora.insert((REF_ORIGIN, returns), options)
        sup.assert_same_tsdf(dev, ora, (case, i))
    _, tsd, _ = ora.get()
    assert (tsd != 0).any()
    dev.close()


def test_same_sequence_twice_gives_equal_bytes(csm):
    """Run to run determinism, and a clean rank plane: every insert after the
    first runs on the plane the one before left (test_every_insert_equals_oracle
    compares each of them)."""
    out = []
    for _ in range(2):
        dev = sup.new_device_grid(csm)
        for origin, ret in _scans("room"):
            dev.insert(origin, ret, sup.OPTION_SETS["F"])
        h = dev.to_host()
        out.append((h.tsd_cells.copy(), h.weight_cells.copy()))
        dev.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_insert_batch_equals_single_inserts_and_oracle(csm, oracle):
    """4 grids x 6 room scans through one insert_batch, scans interleaved over
    the grids (grid g gets the scans in its own rotation of the order)."""
    options = sup.OPTION_SETS["B"]
    room = _scans("room")[:6]
    per_grid = [room[g:] + room[:g] for g in range(4)]
    grids = [sup.new_device_grid(csm) for _ in range(4)]
    scans, gos = [], []
    for i in range(6):
        for g in range(4):
            scans.append(per_grid[g][i])
            gos.append(g)
    csm.DeviceTSDF2D.insert_batch(grids, gos, scans, options)
    for g in range(4):
        single = sup.new_device_grid(csm)
        ora = sup.OracleTSDF(oracle)
        for scan in per_grid[g]:
            single.insert(scan[0], scan[1], options)
            ora.insert(scan, options)
        sup.assert_same_tsdf(grids[g], ora, ("batch", g))
        sup.assert_same_tsdf(single, ora, ("single", g))
        single.close()
    for g in grids:
        g.close()


def _assert_cropped(dev, want):
    (res, max_x, max_y, nx, ny), tsd, wgt = want
    host = dev.to_host()
    got = (host.resolution, host.max_x, host.max_y, host.num_x_cells, host.num_y_cells)
    assert got == (res, max_x, max_y, nx, ny)
    assert np.array_equal(host.tsd_cells, tsd) and np.array_equal(host.weight_cells, wgt)


def test_finish_equals_compute_cropped_grid(csm, oracle):
    options = sup.OPTION_SETS["A"]
    dev, ora = _insert_and_compare(csm, oracle, _scans("room")[:4], options, "finish")
    limits, tsd, wgt = ora.get()
    dev.finish()
    _assert_cropped(dev, sup.oracle_crop(limits, tsd, wgt, sup.TRUNCATION, sup.MAX_WEIGHT))
    assert dev.limits().num_x_cells < 200
    # Later inserts fail and change nothing; a second finish changes nothing.
    lib = csm.load_library()
    o = csm.TSDFInserterOptions.make(options)
    origin, ret = _scans("room")[4]
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(  # noqa: E731
        C.POINTER(C.c_float))
    before = dev.to_host()
    assert lib.csm_tsdf_grid_insert(dev.handle, C.byref(o), fp(origin), fp(ret), len(ret)) == \
        csm.CSM_EINVAL
    dev.finish()
    after = dev.to_host()
    assert np.array_equal(before.tsd_cells, after.tsd_cells)
    assert np.array_equal(before.weight_cells, after.weight_cells)
    dev.close()


def test_finish_all_unknown_grid(csm):
    dev = sup.new_device_grid(csm)
    dev.finish()
    lim = dev.limits()
    want = sup.oracle_crop(sup.INITIAL_LIMITS[:3], np.zeros((100, 100), np.uint16),
                           np.zeros((100, 100), np.uint16), sup.TRUNCATION, sup.MAX_WEIGHT)
    assert (lim.num_x_cells, lim.num_y_cells) == (1, 1)
    assert (lim.max_x, lim.max_y) == (sup.INITIAL_LIMITS[1], sup.INITIAL_LIMITS[2])
    _assert_cropped(dev, want)
    dev.close()


def test_finish_created_grid_with_known_cell_of_weight_zero(csm):
    """A created grid whose known cells carry the weight value 0: the crop
    sends them through WeightToValue(ValueToWeight(0)) = 1."""
    tsd = np.zeros((40, 60), np.uint16)
    wgt = np.zeros_like(tsd)
    tsd[7, 9] = 12345
    tsd[30, 50] = 1
    wgt[30, 50] = 32767
    tsd[12, 20] = 32767
    wgt[12, 20] = 777
    limits = (0.05, 1.5, 1.0)
    dev = csm.DeviceTSDF2D(*limits, 60, 40, 0.3, 10.0, tsd, wgt)
    dev.finish()
    want = sup.oracle_crop(limits, tsd, wgt, 0.3, 10.0)
    _assert_cropped(dev, want)
    assert want[2][0, 0] == 1 and want[0][3:] == (42, 24)
    dev.close()


def test_growth_past_8192_is_erange_and_leaves_the_grid(csm, oracle):
    options = sup.OPTION_SETS["A"]
    dev, ora = _insert_and_compare(csm, oracle, _scans("room")[:1], options, "erange")
    lib = csm.load_library()
    o = csm.TSDFInserterOptions.make(options)
    origin = np.zeros(3, np.float32)
    far = np.array([[1.0, 0.0, 0.0], [300.0, 0.0, 0.0]], np.float32)  # 8192 * 0.05 = 409.6 m
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert lib.csm_tsdf_grid_insert(dev.handle, C.byref(o), fp(origin), fp(far), 2) == \
        csm.CSM_ERANGE
    sup.assert_same_tsdf(dev, ora, "after ERANGE")
    # The grid still takes inserts.
    scan = _scans("room")[1]
    dev.insert(scan[0], scan[1], options)
    ora.insert(scan, options)
    sup.assert_same_tsdf(dev, ora, "insert after ERANGE")
    dev.close()


def test_batch_erange_in_the_second_grid_leaves_both_grids(csm):
    """A batch over two small grids: grid 0's scan is valid and would grow it,
    grid 1's needs more than 8192 cells a side. CSM_ERANGE, and both grids keep
    their limits and planes: everything that can refuse a call comes before the
    first enqueue for any of its grids. (The handles' generation counters have
    no accessor; the limits stand in for them.)"""
    options = sup.OPTION_SETS["A"]
    grids = [sup.new_device_grid(csm, (0.05, 0.2, 0.2, 8, 8)) for _ in range(2)]
    origin = np.zeros(3, np.float32)
    # Past the truncation distance (0.3 m): nearer returns cast no ray.
    near = np.array([[0.5, 0.0, 0], [0.0, 0.45, 0], [-0.4, -0.4, 0]], np.float32)
    for g in grids:
        g.insert(origin, near, options)
    before = [g.to_host() for g in grids]
    side = before[0].num_x_cells
    assert side <= 64 and all((b.weight_cells != 0).any() for b in before)
    grows = np.array([[2.0, 0.0, 0], [0.0, 2.0, 0], [-2.0, -2.0, 0]], np.float32)
    far = np.array([[0.1, 0.0, 0], [300.0, 0.0, 0], [0.0, 0.1, 0]], np.float32)
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        csm.DeviceTSDF2D.insert_batch(grids, [0, 1], [(origin, grows), (origin, far)], options)
    for g, b in zip(grids, before):
        after = g.to_host()
        assert (after.resolution, after.max_x, after.max_y) == (b.resolution, b.max_x, b.max_y)
        assert np.array_equal(after.tsd_cells, b.tsd_cells)
        assert np.array_equal(after.weight_cells, b.weight_cells)
    # The valid scan alone does grow its grid.
    grids[0].insert(origin, grows, options)
    assert grids[0].limits().num_x_cells > side
    for g in grids:
        g.close()


def test_match_on_device_planes(csm, oracle):
    """csm_rt2d_match_tsdf_grid after each of room's inserts: the score and
    pose of csm_rt2d_match_tsdf on the read-back planes, and the oracle's
    within the real-time matcher's 1e-6 relative bar. Each match sees the
    newest grid (generation)."""
    options = sup.OPTION_SETS["A"]
    rt = (0.1, 0.05, 0.1, 0.1)
    m = csm.RealTimeCorrelativeScanMatcher2D(csm.RealTimeCorrelativeScanMatcherOptions(*rt))
    dev = sup.new_device_grid(csm)
    scores = []
    for origin, ret in _scans("room")[:6]:
        dev.insert(origin, ret, options)
        # The scan in the sensor frame, matched from a slightly wrong pose.
        cloud = np.ascontiguousarray(ret - origin)[::3]
        init = (float(origin[0]) + 0.03, float(origin[1]) - 0.02, 0.01)
        score, pose = m.Match(init, cloud, dev)
        host = dev.to_host()
        host_score, host_pose = m.Match(init, cloud, host)
        assert (score, pose) == (host_score, host_pose)
        ref_score, ref_pose, _ = oracle.rt2d_match_tsdf(
            (host.resolution, host.max_x, host.max_y), host.tsd_cells, host.weight_cells,
            sup.TRUNCATION, sup.MAX_WEIGHT, rt, init, cloud)
        assert abs(score - ref_score) <= 1e-6 * abs(ref_score)
        assert pose == ref_pose
        # Again on the cached converted grid.
        assert m.Match(init, cloud, dev) == (score, pose)
        scores.append(score)
    assert min(scores) > 0.0
    dev.close()
