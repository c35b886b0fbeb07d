"""CeresScanMatcher2D on TSDF submaps and on device-resident grids, on the GPU:
TSDFMatchCostFunction2D through csm_ceres2d_tsdf_evaluate, the batch refinement
of TSDF handles against the CPU restatement (ceres_tsdf_support), mixed
batches, the two failure rules, and the single-call entry points that read a
device grid's uint16 cells directly.

Bounds: cost evaluation 1e-9 absolute (both sides do double arithmetic on the
same float inputs; only the summation order of W differs); poses 1e-6 m /
1e-6 rad and iterations +-1, the project's bound for this solver
(test_ceres2d.py:11-12)."""
import numpy as np
import pytest

import ceres_tsdf_support as cs
import tsdf_support as ts

pytestmark = pytest.mark.gpu

FOPTS = (0.5, 0.2, 3)


def _matcher(csm, grid):
    return csm.FastCorrelativeScanMatcher2D(grid, csm.FastCorrelativeScanMatcherOptions2D(*FOPTS))


@pytest.fixture(scope="module")
def room(csm):
    return cs.room_tsdf(csm)


@pytest.fixture(scope="module")
def room_matcher(csm, room):
    m = _matcher(csm, room)
    yield m
    m.close()


def test_evaluate_reference_cases(csm):
    """tsdf_match_cost_function_2d_test.cc's four tests through the device cost,
    to the file's 1e-3 and to 1e-9 of the restatement."""
    empty = _matcher(csm, cs.reference_fixture(csm, empty=True))
    valid, _, _ = csm.ceres_tsdf_evaluate(empty, np.zeros((1, 3), np.float32), 1.0, (0, 0, 0))
    assert not valid
    grid = cs.reference_fixture(csm)
    m = _matcher(csm, grid)
    for pose, want_valid, want_r, want_j in cs.REF_CASES:
        valid, r, jac = csm.ceres_tsdf_evaluate(m, cs.REF_CLOUD, 1.0, pose)
        ok, rr, rj = cs.restated_evaluate(grid, cs.REF_CLOUD, 1.0, pose)
        assert valid == want_valid == ok, pose
        if not valid:
            continue
        assert abs(r[0] - want_r) <= 1e-3 and np.all(np.abs(jac[0] - want_j) <= 1e-3), (pose, r, jac)
        dev = max(np.abs(r - rr).max(), np.abs(jac - rj).max())
        print(f"evaluate {pose}: max |gpu - restatement| = {dev:.3e}")
        assert dev <= 1e-9, (pose, dev)


@pytest.mark.parametrize("n", [1, 2, 253, 257])
def test_evaluate_matches_restatement_on_room(csm, room, room_matcher, n):
    cloud, origin = cs.room_cloud(8, n)
    for pose in [origin, (origin[0] + 0.04, origin[1] - 0.03, 0.02)]:
        valid, r, jac = csm.ceres_tsdf_evaluate(room_matcher, cloud, 20.0 / np.sqrt(n), pose)
        ok, rr, rj = cs.restated_evaluate(room, cloud, 20.0 / np.sqrt(n), pose)
        assert valid and ok
        dr, dj = np.abs(r - rr), np.abs(jac - rj)
        print(f"n={n}: max residual dev {dr.max():.3e} (row {dr.argmax()}), "
              f"Jacobian dev {dj.max():.3e} (row {dj.argmax() // 3})")
        assert dr.max() <= 1e-9 and dj.max() <= 1e-9


def _room_items(rng):
    """24 items: n in (1, 2, 253, 254, 256, 257), starts perturbed by about
    5 cm / 0.03 rad as in test_gpu_refinement_matches_oracle."""
    clouds, init, tgt = [], [], []
    for k in range(24):
        n = (1, 2, 253, 254, 256, 257)[k % 6]
        cloud, origin = cs.room_cloud(2 + k % 8, n)
        p = (origin[0] + rng.normal(0, 0.05), origin[1] + rng.normal(0, 0.05), rng.normal(0, 0.03))
        clouds.append(cloud)
        init.append(p)
        tgt.append((p[0] + rng.normal(0, 0.01), p[1] + rng.normal(0, 0.01)))
    return clouds, init, tgt


def test_batch_refinement_matches_restatement(csm, room, room_matcher):
    clouds, init, tgt = _room_items(np.random.default_rng(9))
    scans = csm.ScanSet(clouds)
    n = len(clouds)
    worst = [0.0, 0.0]
    for opts in cs.OPTION_SETS:
        poses, iters = csm.ceres_refine_batch([room_matcher], scans, [0] * n, list(range(n)), init,
                                              tgt, cs.make_options(csm, opts))
        for k in range(n):
            ref, ref_it, _ = cs.restated_match(room, opts, tgt[k], init[k], clouds[k])
            d = np.abs(np.asarray(poses[k]) - ref)
            worst = [max(worst[0], d[:2].max()), max(worst[1], d[2])]
            assert np.allclose(poses[k], ref, rtol=0, atol=1e-6), (opts, k, poses[k], ref)
            assert abs(int(iters[k]) - ref_it) <= 1, (opts, k, iters[k], ref_it)
    print(f"largest deviation: {worst[0]:.3e} m, {worst[1]:.3e} rad")


def test_mixed_batch_equals_batches_of_one_kind(csm, room_matcher):
    w = csm.SyntheticWorld2D(num_nodes=6, num_submaps=2, submap_cells=200, decimate_to=200, seed=5)
    prob = [csm.FastCorrelativeScanMatcher2D(w.grid(s), csm.FastCorrelativeScanMatcherOptions2D())
            for s in range(2)]
    rng = np.random.default_rng(4)
    clouds, init = [], []
    for i in range(6):  # probability items: scans 0..5
        t = w.node_poses[i]
        clouds.append(w.cloud(i))
        init.append((t[0] + rng.normal(0, 0.05), t[1] + rng.normal(0, 0.05),
                     t[2] + rng.normal(0, 0.03)))
    for i in range(5):  # TSDF items: scans 6..10
        cloud, origin = cs.room_cloud(3 + i, 120)
        clouds.append(cloud)
        init.append((origin[0] + rng.normal(0, 0.05), origin[1] + rng.normal(0, 0.05),
                     rng.normal(0, 0.03)))
    scans = csm.ScanSet(clouds)
    matchers = prob + [room_matcher]
    sub = [0, 1, 0, 1, 0, 1] + [2] * 5
    order = [0, 6, 1, 7, 8, 2, 3, 9, 4, 10, 5]  # interleaved
    mixed, mixed_it = csm.ceres_refine_batch(matchers, scans, [sub[i] for i in order], order,
                                             [init[i] for i in order])
    p_idx, t_idx = list(range(6)), list(range(6, 11))
    own_p, own_p_it = csm.ceres_refine_batch(matchers, scans, [sub[i] for i in p_idx], p_idx,
                                             [init[i] for i in p_idx])
    own_t, own_t_it = csm.ceres_refine_batch(matchers, scans, [sub[i] for i in t_idx], t_idx,
                                             [init[i] for i in t_idx])
    own = {i: (own_p[k], own_p_it[k]) for k, i in enumerate(p_idx)}
    own.update({i: (own_t[k], own_t_it[k]) for k, i in enumerate(t_idx)})
    for k, i in enumerate(order):
        assert np.array_equal(mixed[k], own[i][0]) and mixed_it[k] == own[i][1], (k, i)
    assert (own_t_it >= 1).all() and own_p_it.max() >= 1  # both kernels did work


def test_failed_initial_evaluation_returns_the_initial_pose(csm, room, room_matcher):
    off_grid = np.array([[500.0, 500.0, 0.0], [501.0, 499.0, 0.0]], np.float32)
    never_seen = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, 0.0]], np.float32)  # mid-room: no weight
    scans = csm.ScanSet([off_grid, never_seen])
    init = [(1.0, 2.0, 0.3), (0.1, -0.2, 0.05)]
    poses, iters = csm.ceres_refine_batch([room_matcher], scans, [0, 0], [0, 1], init,
                                          [(1.2, 2.1), (0.0, 0.0)])
    for k in range(2):
        assert tuple(poses[k]) == init[k], (k, poses[k])  # bit for bit
        assert iters[k] == 0
        assert cs.restated_match(room, (20.0, 10.0, 1.0, 10), (0.0, 0.0), init[k],
                                 [off_grid, never_seen][k])[1:] == (0, 0)


@pytest.mark.parametrize("opts,cloud,want_failed", cs.CANDIDATE_FAILURES)
def test_failed_candidate_evaluation_matches_restatement(csm, room, room_matcher, opts, cloud,
                                                         want_failed):
    cloud = np.asarray(cloud, np.float32)
    ref, ref_it, failed = cs.restated_match(room, opts, (0.0, 0.0), (0.0, 0.0, 0.0), cloud)
    assert failed == want_failed > 0
    scans = csm.ScanSet([cloud])
    poses, iters = csm.ceres_refine_batch([room_matcher], scans, [0], [0], [(0.0, 0.0, 0.0)],
                                          [(0.0, 0.0)], cs.make_options(csm, opts))
    print(f"candidate failures {failed}: |gpu - restatement| = {np.abs(poses[0] - ref).max():.3e}")
    assert np.allclose(poses[0], ref, rtol=0, atol=1e-6), (poses[0], ref)
    assert abs(int(iters[0]) - ref_it) <= 1


def _device_room(csm, scans):
    dev = ts.new_device_grid(csm)
    for scan in scans:
        dev.insert(scan[0], scan[1], ts.OPTION_SETS["A"])
    return dev


def test_same_results_however_the_grid_arrives(csm, room, room_matcher):
    """A handle from the device grid after device insertion and one from the
    oracle's byte-equal host planes: identical levels, identical refinement.
    The handle outlives its grid. csm_ceres2d_match_tsdf_grid, which reads the
    uint16 cells through the tables, gives the batch result bitwise: the
    accessor yields the same floats and the arithmetic after it is shared."""
    dev = _device_room(csm, ts.room())
    host = dev.to_host()
    assert np.array_equal(host.tsd_cells, room.tsd_cells)
    assert np.array_equal(host.weight_cells, room.weight_cells)
    from_dev = _matcher(csm, dev)
    # csm_fast2d_device_bytes counts the pyramid and both float planes.
    levels = sum(from_dev.read_level(d).size for d in range(FOPTS[2]))
    assert from_dev.device_bytes() >= levels + 2 * 4 * room.tsd_cells.size
    clouds, init, tgt = _room_items(np.random.default_rng(2))
    clouds, init, tgt = clouds[:8], init[:8], tgt[:8]
    single = [csm.CeresScanMatcher2D().Match(tgt[k], init[k], clouds[k], dev) for k in range(8)]
    dev.close()  # the handle keeps its own planes
    for d in range(FOPTS[2]):
        assert np.array_equal(from_dev.read_level(d), room_matcher.read_level(d)), d
    scans = csm.ScanSet(clouds)
    a, a_it = csm.ceres_refine_batch([from_dev], scans, [0] * 8, list(range(8)), init, tgt)
    b, b_it = csm.ceres_refine_batch([room_matcher], scans, [0] * 8, list(range(8)), init, tgt)
    assert np.array_equal(a, b) and np.array_equal(a_it, b_it)
    for k in range(8):
        assert single[k][0] == tuple(b[k]) and single[k][1] == b_it[k], (k, single[k], b[k])
    # The host-grid overload goes through a one-level handle: the same again.
    pose, it = csm.CeresScanMatcher2D().Match(tgt[0], init[0], clouds[0], room)
    assert pose == tuple(b[0]) and it == b_it[0]


def test_match_grid_reads_the_live_probability_grid(csm, oracle):
    """csm_ceres2d_match_grid equals the oracle after an insert and again after
    a further insert: no stale copy is read."""
    from insert2d_support import INITIAL_LIMITS
    scans = ts.room()
    dev = csm.DeviceProbabilityGrid(*INITIAL_LIMITS)
    matcher = csm.CeresScanMatcher2D()
    cloud, origin = cs.room_cloud(1, 150)
    init = (origin[0] + 0.04, origin[1] - 0.03, 0.02)
    seen = []
    for upto in (0, 1):
        dev.insert(scans[upto][0], scans[upto][1], None)
        pose, it = matcher.Match(init[:2], init, cloud, dev)
        g = dev.to_host()
        ref, ref_it = oracle.ceres2d_match((g.resolution, g.max_x, g.max_y), g.cells,
                                           (20.0, 10.0, 1.0, 10), init[:2], init, cloud)
        assert np.allclose(pose, ref, rtol=0, atol=1e-6), (upto, pose, ref)
        assert abs(it - ref_it) <= 1
        seen.append(pose)
    assert seen[0] != seen[1]
    # The host ProbabilityGrid overload: the same solve through a handle.
    pose_h, _ = matcher.Match(init[:2], init, cloud, dev.to_host())
    assert np.allclose(pose_h, seen[1], rtol=0, atol=1e-12)


def test_error_paths(csm, room, room_matcher):
    lib = csm.load_library()
    ctx = csm.default_context()
    other = csm.Context(0)
    import ctypes as C
    lim = room.limits()
    opts = csm.Fast2DOptions(0.5, 0.2, 3, 0)
    tsd = np.ascontiguousarray(room.tsd_cells)
    wgt = np.ascontiguousarray(room.weight_cells)
    u16 = C.POINTER(C.c_uint16)
    h = C.c_void_p()

    def create(t, w, trunc, mw):
        return lib.csm_fast2d_create_tsdf(ctx.handle, C.byref(lim),
                                          t.ctypes.data_as(u16) if t is not None else None,
                                          w.ctypes.data_as(u16) if w is not None else None,
                                          trunc, mw, C.byref(opts), C.byref(h))
    assert create(tsd, None, 0.3, 10.0) == csm.CSM_EINVAL
    assert create(None, wgt, 0.3, 10.0) == csm.CSM_EINVAL
    assert create(tsd, wgt, 0.0, 10.0) == csm.CSM_EINVAL
    assert create(tsd, wgt, 0.3, -1.0) == csm.CSM_EINVAL
    # A probability handle has no TSDF cost.
    w = csm.SyntheticWorld2D(num_nodes=2, num_submaps=1, submap_cells=64, decimate_to=50, seed=1)
    prob = csm.FastCorrelativeScanMatcher2D(w.grid(0), csm.FastCorrelativeScanMatcherOptions2D())
    with pytest.raises(csm.CsmError):
        csm.ceres_tsdf_evaluate(prob, cs.REF_CLOUD, 1.0, (0, 0, 0))
    # A handle or grid of another context.
    with pytest.raises(csm.CsmError):
        csm.ceres_tsdf_evaluate(room_matcher, cs.REF_CLOUD, 1.0, (0, 0, 0), context=other)
    dev = csm.DeviceTSDF2D.from_host(room)
    with pytest.raises(csm.CsmError):
        csm.CeresScanMatcher2D(context=other).Match((0, 0), (0, 0, 0), cs.REF_CLOUD, dev)
    with pytest.raises(csm.CsmError):  # n >= 1
        csm.CeresScanMatcher2D().Match((0, 0), (0, 0, 0), np.zeros((0, 3), np.float32), dev)
    with pytest.raises(csm.CsmError):  # finite points
        csm.CeresScanMatcher2D().Match((0, 0), (0, 0, 0),
                                       np.array([[np.nan, 0, 0]], np.float32), dev)
    other.close()
