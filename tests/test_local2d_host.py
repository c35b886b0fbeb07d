"""CPU: the host side of LocalTrajectoryBuilder2D. The reference's
motion_filter_test.cc cases through the Python MotionFilter and the shim's
(tests/cpp/oracle_local2d_shim.cc), which must agree; the shim's front end on
inputs whose outputs can be worked out by hand; the Python mirror's rigid
transforms against the shim's; and DESIGN.md's scope."""
import math
import os

import numpy as np
import pytest

from conftest import ROOT

import local2d_support as sup

IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))


@pytest.fixture(scope="module")
def ltb(csm):
    import importlib
    return importlib.import_module("cartographer_amd.local_trajectory_builder_2d")


def _translation(x, y, z):
    return ((x, y, z), (1.0, 0.0, 0.0, 0.0))


def _rotation_y(angle):
    """Rigid3d::Rotation(AngleAxisd(angle, UnitY))."""
    return ((0.0, 0.0, 0.0), (math.cos(angle / 2), 0.0, math.sin(angle / 2), 0.0))


# motion_filter_test.cc:40-113: (test, [(seconds, pose, expected IsSimilar)]), with
# max_time_seconds = 0.5, max_distance_meters = 0.2, max_angle_radians = 2.
MOTION_FILTER_CASES = {
    "NotInitialized": [(0, IDENTITY, False)],
    "NoChange": [(42, IDENTITY, False), (42, IDENTITY, True)],
    "TimeElapsed": [(42, IDENTITY, False), (43, IDENTITY, False), (43, IDENTITY, True)],
    "LinearMotion": [(42, IDENTITY, False), (42, _translation(0.3, 0, 0), False),
                     (42, _translation(0.45, 0, 0), True), (42, _translation(0.6, 0, 0), False),
                     (42, _translation(0.6, 0.15, 0), True)],
    "RotationalMotion": [(42, IDENTITY, False), (42, _rotation_y(1.9), True),
                         (42, _rotation_y(2.1), False), (42, _rotation_y(4.0), True),
                         (42, _rotation_y(5.9), False), (42, IDENTITY, True)],
}


@pytest.mark.parametrize("name", sorted(MOTION_FILTER_CASES))
def test_motion_filter_reference_cases(ltb, name):
    py = ltb.MotionFilter(ltb.MotionFilterOptions(0.5, 0.2, 2.0))
    ref = sup.ShimMotionFilter(0.5, 0.2, 2.0)
    for seconds, pose, expected in MOTION_FILTER_CASES[name]:
        got_py = py.IsSimilar(float(seconds), pose)
        got_ref = ref.IsSimilar(float(seconds), pose)
        assert got_py == got_ref == expected, (name, seconds, pose, got_py, got_ref)


def test_motion_filter_python_equals_shim_on_a_random_walk(ltb):
    rng = np.random.default_rng(5)
    py = ltb.MotionFilter(ltb.MotionFilterOptions(0.5, 0.2, 0.1))
    ref = sup.ShimMotionFilter(0.5, 0.2, 0.1)
    t, xyz, rpy = 0.0, np.zeros(3), np.zeros(3)
    decisions = []
    for _ in range(300):
        t += rng.uniform(0.0, 0.2)
        xyz = xyz + rng.uniform(-0.05, 0.05, 3)
        rpy = rpy + rng.uniform(-0.02, 0.02, 3)
        pose = (tuple(xyz), sup.quat_from_rpy(*rpy))
        decisions.append(py.IsSimilar(t, pose))
        assert decisions[-1] == ref.IsSimilar(t, pose)
    assert 20 < sum(decisions) < 280  # both outcomes occur


def test_default_options_are_the_lua_defaults(csm, ltb):
    o = ltb.LocalTrajectoryBuilderOptions2D()
    assert (o.min_range, o.max_range, o.min_z, o.max_z) == (0.0, 30.0, -0.8, 2.0)
    assert (o.missing_data_ray_length, o.num_accumulated_range_data) == (5.0, 1)
    assert o.voxel_filter_size == 0.025 and not o.use_online_correlative_scan_matching
    a = o.adaptive_voxel_filter_options
    assert (a.max_length, a.min_num_points, a.max_range) == (0.5, 200.0, 50.0)
    c = o.ceres_scan_matcher_options
    assert (c.occupied_space_weight, c.translation_weight, c.rotation_weight) == (1.0, 10.0, 40.0)
    assert (c.max_num_iterations, c.use_nonmonotonic_steps) == (20, False)
    m = o.motion_filter_options
    assert (m.max_time_seconds, m.max_distance_meters) == (5.0, 0.2)
    assert m.max_angle_radians == math.radians(1.0)
    assert o.submaps_options.num_range_data == 90
    r = o.range_data_options()
    assert isinstance(r, csm.RangeData2DOptions)
    assert r.voxel_filter_size == np.float32(0.025) and r.max_z == 2.0


def test_python_transforms_equal_the_shims(ltb):
    """The three rigid transforms the builder computes on the host, bit for bit."""
    rng = np.random.default_rng(11)
    for _ in range(50):
        gq = sup.quat_from_rpy(*rng.uniform(-0.1, 0.1, 2), 0.0)
        pose = (tuple(rng.uniform(-20, 20, 3)), sup.quat_from_rpy(*rng.uniform(-3, 3, 3)))
        last = np.array(list(pose[0]) + list(pose[1]), np.float32)
        want = sup.gravity_from_local(gq, last)
        got = ltb._tq(ltb._mul(ltb._cast_f(((0.0, 0.0, 0.0), gq)),
                               ltb._inverse((tuple(last[:3]), tuple(last[3:]))), np.sqrt))
        assert got.tobytes() == want.tobytes()
        pred = ltb.Project2D(ltb._mul(pose, ltb._inverse(((0.0, 0.0, 0.0), gq)), math.sqrt))
        assert pred == sup.pose_prediction(pose, gq)
        pose2d = tuple(rng.uniform(-4, 4, 3))
        assert ltb._mul(ltb.Embed3D(pose2d), ((0.0, 0.0, 0.0), gq), math.sqrt) == \
            sup.pose_estimate(pose2d, gq)
        assert ltb._tq(ltb.Embed3DF(pose2d)).tobytes() == sup.embed3d_f(pose2d).tobytes()


# ---- the shim's front end on inputs worked out by hand -----------------------------

def _options(csm, **kw):
    base = dict(min_range=1.0, max_range=5.0, missing_data_ray_length=2.0, min_z=-0.5, max_z=0.5,
                voxel_filter_size=0.025,
                adaptive_voxel_filter=csm.AdaptiveVoxelFilterOptions.make(0.5, 200, 50.0))
    base.update(kw)
    return csm.RangeData2DOptions.make(**base)


def _shim_prepare(csm, hits, **kw):
    hits = np.asarray(hits, np.float32).reshape(-1, 3)
    n = len(hits)
    return sup.prepare(_options(csm, **kw), hits, np.zeros(n, np.int32), sup.identity_poses(n),
                       np.zeros((1, 3), np.float32), sup.IDENTITY_TQ, np.zeros(3, np.float32))


def test_shim_range_bounds_are_inclusive(csm):
    origin, returns, misses, filtered = _shim_prepare(csm, [[3, 4, 0], [6, 8, 0]])
    assert origin.tolist() == [0, 0, 0]
    assert returns.tolist() == [[3, 4, 0]]  # range exactly max_range = 5: a return
    s = np.float32(2.0) / np.float32(10.0)  # missing_data_ray_length / range
    assert misses.tobytes() == np.array([[s * np.float32(6), s * np.float32(8), 0]],
                                        np.float32).tobytes()
    assert filtered.tolist() == [[3, 4, 0]]


def test_shim_min_range_is_inclusive(csm):
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    _, returns, misses, _ = _shim_prepare(csm, [[1, 0, 0], [below, 0, 0], [0, below, 0],
                                                [0, 1, 0]])
    assert returns.tolist() == [[1, 0, 0], [0, 1, 0]] and len(misses) == 0


def test_shim_drops_a_nan_hit(csm):
    _, returns, misses, _ = _shim_prepare(csm, [[2, 0, 0], [np.nan, 0, 0], [0, np.nan, 0],
                                                [0, 2, 0], [0, 0, np.nan]])
    assert returns.tolist() == [[2, 0, 0], [0, 2, 0]] and len(misses) == 0


def test_shim_z_bounds_are_inclusive(csm):
    above = np.nextafter(np.float32(0.5), np.float32(1.0))
    below = np.nextafter(np.float32(-0.5), np.float32(-1.0))
    _, returns, _, _ = _shim_prepare(csm, [[2, 0, -0.5], [0, 2, 0.5], [-2, 0, above],
                                           [0, -2, below]])
    assert returns.tolist() == [[2, 0, -0.5], [0, 2, 0.5]]


def test_shim_moves_each_point_by_its_own_pose(csm):
    """A quarter turn about z and a shift: hit (2, 0, 0) from origin (1, 0, 0)
    lands at (10, 2 + 20, 0) and its origin at (10, 1 + 20, 0): range 1."""
    h = math.sqrt(0.5)
    poses = np.array([[10, 20, 0, h, 0, 0, h]], np.float32)
    o = _options(csm, min_range=0.5)
    _, returns, _, _ = sup.prepare(o, [[2, 0, 0]], [0], poses, [[1, 0, 0]], sup.IDENTITY_TQ,
                                   np.zeros(3, np.float32))
    assert np.allclose(returns, [[10, 22, 0]], atol=1e-5)
    o = _options(csm, min_range=1.5)
    assert len(sup.prepare(o, [[2, 0, 0]], [0], poses, [[1, 0, 0]], sup.IDENTITY_TQ,
                           np.zeros(3, np.float32))[1]) == 0


def test_design_scope():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    scope = text[text.index("## 9"):]
    scope = scope[:scope.index("\n## ", 4)] if "\n## " in scope[4:] else scope
    assert "TransformRangeData" not in scope
    assert "csm_range_data2d_prepare" in text and "LocalTrajectoryBuilder2D" in text
