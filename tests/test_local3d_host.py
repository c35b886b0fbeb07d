"""CPU: the host side of the 3D local SLAM front end: csm_compute_histogram
against the oracle's ComputeHistogram bit for bit, the argument checks of the
large voxel filters and of csm_range_data3d_prepare that return before any
handle is read, the minstd_rand0 walk that pins the input of the GPU
rejection test, the option structs against the header and
trajectory_builder_3d.lua, and the adaptive-search restatement's pass counts
for the clouds the GPU test relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import local3d_support as sup

NEW_ENTRIES = ["csm_voxel_filter_large", "csm_adaptive_voxel_filter_large",
               "csm_range_data3d_prepare", "csm_compute_histogram"]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _room_cloud(n, seed):
    rng = np.random.RandomState(seed)
    return sup.room_sweep(rng, n) + rng.normal(0, 0.01, (n, 3)).astype(np.float32)


HISTOGRAM_CLOUDS = {
    "room": lambda: _room_cloud(3000, 11),
    "one_slice": lambda: np.concatenate(
        [_room_cloud(800, 12)[:, :2], np.full((800, 1), 0.31, np.float32)], 1),
    "empty": lambda: np.zeros((0, 3), np.float32),
    "identical": lambda: np.tile(np.array([[1.5, -2.0, 0.7]], np.float32), (200, 1)),
}


@pytest.mark.parametrize("size", [120, 7])
@pytest.mark.parametrize("name", sorted(HISTOGRAM_CLOUDS))
def test_compute_histogram_equals_oracle(csm, oracle, name, size):
    cloud = HISTOGRAM_CLOUDS[name]()
    got = csm.compute_histogram(cloud, size)
    want = oracle.histogram(cloud, size)
    assert got.dtype == np.float32 and got.shape == (size,)
    sup.assert_same_bits(got, want, name)
    if name == "room":
        assert got.sum() > 0  # the comparison is not of two empty histograms


def test_compute_histogram_argument_checks(csm):
    lib = csm.load_library()
    pts = np.zeros((4, 3), np.float32)
    out = np.zeros(8, np.float32)
    assert lib.csm_compute_histogram(_fp(pts), -1, 8, _fp(out)) == csm.CSM_EINVAL
    assert lib.csm_compute_histogram(_fp(pts), 4, 0, _fp(out)) == csm.CSM_EINVAL
    assert lib.csm_compute_histogram(None, 4, 8, _fp(out)) == csm.CSM_EINVAL
    assert lib.csm_compute_histogram(_fp(pts), 4, 8, None) == csm.CSM_EINVAL
    assert lib.csm_compute_histogram(None, 0, 8, _fp(out)) == csm.CSM_OK


def test_header_declares_and_library_exports_new_entries(csm):
    text = open(os.path.join(ROOT, "include", "csm_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(csm_[a-z0-9_]+)\s*\(", text))
    lib = csm.load_library()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in csm._SIGNATURES, name
    assert "csm_range_data3d_options" in text


def _fake_handle():
    """A handle-sized block of zeros: an argument check must not read it."""
    fake = (C.c_uint8 * 4096)()
    return fake, C.cast(fake, C.c_void_p)


def test_large_filters_check_arguments_without_a_device(csm):
    lib = csm.load_library()
    _keepalive, handle = _fake_handle()
    pts = np.zeros((4, 3), np.float32)
    keep = np.zeros(4, np.uint8)
    kp = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    count = C.c_int64(-1)
    opts = csm.AdaptiveVoxelFilterOptions.make(2.0, 150, 15.0)
    too_many = 2**20 + 1
    assert lib.csm_voxel_filter_large(handle, _fp(pts), too_many, 0.1, kp,
                                      C.byref(count)) == csm.CSM_ERANGE
    assert lib.csm_adaptive_voxel_filter_large(handle, _fp(pts), too_many, C.byref(opts), kp,
                                               C.byref(count)) == csm.CSM_ERANGE
    for bad in (0.0, -1.0, float("nan")):
        assert lib.csm_voxel_filter_large(handle, _fp(pts), 4, bad, kp,
                                          C.byref(count)) == csm.CSM_EINVAL
        bad_opts = csm.AdaptiveVoxelFilterOptions.make(bad, 150, 15.0)
        assert lib.csm_adaptive_voxel_filter_large(handle, _fp(pts), 4, C.byref(bad_opts), kp,
                                                   C.byref(count)) == csm.CSM_EINVAL
    assert lib.csm_voxel_filter_large(handle, None, 4, 0.1, kp, C.byref(count)) == csm.CSM_EINVAL
    assert lib.csm_voxel_filter_large(handle, _fp(pts), 4, 0.1, None,
                                      C.byref(count)) == csm.CSM_EINVAL
    assert lib.csm_voxel_filter_large(handle, _fp(pts), 4, 0.1, kp, None) == csm.CSM_EINVAL
    assert lib.csm_voxel_filter_large(handle, _fp(pts), -1, 0.1, kp,
                                      C.byref(count)) == csm.CSM_EINVAL
    assert lib.csm_voxel_filter_large(None, _fp(pts), 4, 0.1, kp, C.byref(count)) == csm.CSM_EINVAL
    assert lib.csm_adaptive_voxel_filter_large(handle, _fp(pts), 4, None, kp,
                                               C.byref(count)) == csm.CSM_EINVAL
    # An empty cloud is fine and touches nothing.
    assert lib.csm_voxel_filter_large(handle, None, 0, 0.1, None, C.byref(count)) == csm.CSM_OK
    assert count.value == 0
    count.value = -1
    assert lib.csm_adaptive_voxel_filter_large(handle, None, 0, C.byref(opts), None,
                                               C.byref(count)) == csm.CSM_OK
    assert count.value == 0


def _prepare_args(csm, n, num_origins=3):
    hits = np.ones((max(n, 1), 3), np.float32)
    idx = np.zeros(max(n, 1), np.int32)
    poses = np.zeros((max(n, 1), 7), np.float32)
    poses[:, 3] = 1
    origins = np.zeros((num_origins, 3), np.float32)
    tfl = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    lo = np.zeros(3, np.float32)
    outs = {k: np.zeros((max(n, 1), 3), np.float32) for k in ("returns", "misses", "high", "low")}
    return dict(hits=hits, idx=idx, poses=poses, origins=origins, tfl=tfl, lo=lo, outs=outs,
                origin=np.zeros(3, np.float32), counts=[C.c_int32(-1) for _ in range(4)])


def _call_prepare(lib, handle, options, a, n, num_origins=3, **override):
    v = dict(hits=_fp(a["hits"]), idx=a["idx"].ctypes.data_as(C.POINTER(C.c_int32)),
             poses=_fp(a["poses"]), origins=_fp(a["origins"]), tfl=_fp(a["tfl"]), lo=_fp(a["lo"]),
             origin=_fp(a["origin"]), returns=_fp(a["outs"]["returns"]),
             misses=_fp(a["outs"]["misses"]), high=_fp(a["outs"]["high"]),
             low=_fp(a["outs"]["low"]), intensities=None)
    v.update(override)
    c = a["counts"]
    return lib.csm_range_data3d_prepare(
        handle, C.byref(options) if options is not None else None, v["hits"], v["intensities"],
        v["idx"], v["poses"], n, v["origins"], num_origins, v["tfl"], v["lo"], v["origin"],
        v["returns"], None, C.byref(c[0]), v["misses"], C.byref(c[1]), v["high"], None,
        C.byref(c[2]), v["low"], None, C.byref(c[3]))


def test_range_data3d_prepare_checks_arguments_without_a_device(csm):
    lib = csm.load_library()
    _keepalive, handle = _fake_handle()
    opts = csm.RangeData3DOptions.make()
    a = _prepare_args(csm, 4)
    assert _call_prepare(lib, handle, opts, a, 2**20 + 1) == csm.CSM_ERANGE
    assert _call_prepare(lib, None, opts, a, 4) == csm.CSM_EINVAL
    assert _call_prepare(lib, handle, None, a, 4) == csm.CSM_EINVAL
    assert _call_prepare(lib, handle, opts, a, -1) == csm.CSM_EINVAL
    for missing in ("hits", "idx", "poses", "origins", "returns", "misses", "high", "low", "tfl",
                    "lo", "origin"):
        assert _call_prepare(lib, handle, opts, a, 4, **{missing: None}) == csm.CSM_EINVAL, missing
    # Intensities in, but nowhere to put them.
    inten = np.zeros(4, np.float32)
    assert _call_prepare(lib, handle, opts, a, 4, intensities=_fp(inten)) == csm.CSM_EINVAL
    bad = _prepare_args(csm, 4)
    bad["idx"][2] = 3
    assert _call_prepare(lib, handle, opts, bad, 4) == csm.CSM_EINVAL
    bad["idx"][2] = -1
    assert _call_prepare(lib, handle, opts, bad, 4) == csm.CSM_EINVAL
    for field in ("voxel_filter_size",):
        o = csm.RangeData3DOptions.make(**{field: 0.0})
        assert _call_prepare(lib, handle, o, a, 4) == csm.CSM_EINVAL
    o = csm.RangeData3DOptions.make(
        high_resolution_adaptive_voxel_filter=csm.AdaptiveVoxelFilterOptions.make(0.0, 150, 15.0))
    assert _call_prepare(lib, handle, o, a, 4) == csm.CSM_EINVAL
    o = csm.RangeData3DOptions.make(
        low_resolution_adaptive_voxel_filter=csm.AdaptiveVoxelFilterOptions.make(-4.0, 200, 60.0))
    assert _call_prepare(lib, handle, o, a, 4) == csm.CSM_EINVAL
    # n == 0: zero counts and the moved origin, without a device.
    a["lo"][:] = (1.0, 2.0, 3.0)
    a["tfl"][:3] = (0.5, 0.0, -1.0)
    assert _call_prepare(lib, handle, opts, a, 0) == csm.CSM_OK
    assert [c.value for c in a["counts"]] == [0, 0, 0, 0]
    assert a["origin"].tolist() == [1.5, 2.0, 2.0]


def test_rejections_of_a_single_voxel_of_140000_points():
    """What test_voxel_filter_large_gpu.py's single-voxel case relies on: four
    rejected draws, so five draw passes, the last three at ranks a uint16
    cannot hold."""
    assert sup.rejected_points(140000) == [1311, 122567, 124405, 134497]
    assert sup.rejected_points(2000) == [1311]


def test_option_structs_match_the_header_and_the_lua_defaults(csm):
    text = open(os.path.join(ROOT, "include", "csm_amd.h")).read()
    body = re.search(r"typedef struct csm_range_data3d_options \{(.*?)\} csm_range_data3d_options;",
                     text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+);", body)
    assert [f for _, f in fields] == [f for f, _ in csm.RangeData3DOptions._fields_]
    assert C.sizeof(csm.RangeData3DOptions) == 4 * 3 + 2 * C.sizeof(csm.AdaptiveVoxelFilterOptions)
    assert C.sizeof(csm.AdaptiveVoxelFilterOptions) == 12
    o = csm.RangeData3DOptions.make()
    assert (o.min_range, o.max_range) == (1.0, 60.0)
    assert o.voxel_filter_size == np.float32(0.15)
    h, l = o.high_resolution_adaptive_voxel_filter, o.low_resolution_adaptive_voxel_filter
    assert (h.max_length, h.min_num_points, h.max_range) == sup.HIGH_OPTIONS
    assert (l.max_length, l.min_num_points, l.max_range) == sup.LOW_OPTIONS


def test_adaptive_cases_take_every_branch_of_the_search():
    """The clouds of the GPU adaptive test, through the counted restatement:
    no pass (the range filter leaves at most min_num_points), one pass
    (max_length suffices), more than two (halving, then bisection), and the
    halving running out (no length reaches min_num_points)."""
    import test_voxel_filter_large_gpu as gpu_cases
    seen = set()
    for name, cloud, options in gpu_cases.adaptive_cases():
        keep, passes = sup.adaptive(cloud, options)
        branch = gpu_cases.branch_of(passes, int(keep.sum()), options[1])
        seen.add(branch)
        assert gpu_cases.ADAPTIVE_BRANCH[name] == branch, (name, passes, int(keep.sum()))
    assert seen == {"none", "one", "bisect", "exhausted"}


# ---- the 3D builder's host side --------------------------------------------------

@pytest.fixture(scope="module")
def ltb(csm):
    import importlib
    return importlib.import_module("cartographer_amd.local_trajectory_builder_3d")


def test_builder_options_are_the_lua_defaults(csm, ltb):
    """trajectory_builder_3d.lua:18-112."""
    o = ltb.LocalTrajectoryBuilderOptions3D()
    assert (o.min_range, o.max_range, o.num_accumulated_range_data) == (1.0, 60.0, 1)
    assert o.voxel_filter_size == 0.15 and o.rotational_histogram_size == 120
    assert not o.use_online_correlative_scan_matching and not o.use_intensities
    rt = o.real_time_correlative_scan_matcher_options
    assert (rt.linear_search_window, rt.angular_search_window) == (0.15, np.radians(1.0))
    assert (rt.translation_delta_cost_weight, rt.rotation_delta_cost_weight) == (1e-1, 1e-1)
    c = o.ceres_scan_matcher_options
    assert (c.occupied_space_weight_0, c.occupied_space_weight_1) == (1.0, 6.0)
    assert (c.translation_weight, c.rotation_weight, c.max_num_iterations) == (5.0, 4e2, 12)
    i = c.intensity_cost_function_options_0
    assert (i.weight, i.huber_scale, i.intensity_threshold) == (0.5, 0.3, 40.0)
    m = o.motion_filter_options
    assert (m.max_time_seconds, m.max_distance_meters, m.max_angle_radians) == (0.5, 0.1, 0.004)
    s = o.submaps_options
    assert (s.high_resolution, s.high_resolution_max_range, s.low_resolution,
            s.num_range_data) == (0.10, 20.0, 0.45, 160)
    r = s.range_data_inserter_options
    assert (r.hit_probability, r.miss_probability, r.num_free_space_voxels,
            r.intensity_threshold) == (0.55, 0.49, 2, 40.0)
    rd = o.range_data_options()
    assert bytes(rd) == bytes(csm.RangeData3DOptions.make())
    # The header's defaults are the same numbers.
    text = open(os.path.join(ROOT, "include", "cartographer_amd",
                             "local_trajectory_builder_3d.h")).read()
    for needle in ("min_range = 1.f", "max_range = 60.f", "voxel_filter_size = 0.15f",
                   "{2.f, 150.f,", "{4.f, 200.f,", "rotational_histogram_size = 120",
                   "max_distance_meters = 0.1", "max_angle_radians = 0.004",
                   "linear_search_window = 0.15"):
        assert needle in text, needle
    for left_out in ("scanmatch_mode", "VoxelFilterEdge", "IMU-acceleration gate", "PCD",
                     "metrics gauges"):
        assert left_out in text, left_out


def test_motion_filter_reference_cases_through_the_3d_options(ltb):
    """motion_filter_test.cc:40-113 with the filter the 3D builder makes from
    its options."""
    import local2d_support as sup2
    from test_local2d_host import MOTION_FILTER_CASES

    class NoDevice:
        """Stands in for the context: the builder's constructor touches none."""
        _lib = None

    for name, steps in sorted(MOTION_FILTER_CASES.items()):
        options = ltb.LocalTrajectoryBuilderOptions3D(
            motion_filter_options=ltb.MotionFilterOptions(0.5, 0.2, 2.0))
        builder = ltb.LocalTrajectoryBuilder3D(options, None, NoDevice())
        ref = sup2.ShimMotionFilter(0.5, 0.2, 2.0)
        for seconds, pose, expected in steps:
            got = builder.motion_filter.IsSimilar(float(seconds), pose)
            assert got == ref.IsSimilar(float(seconds), pose) == expected, (name, seconds)


def test_python_host_arithmetic_equals_the_shims(ltb):
    """tracking_from_local, the local origin and local_from_gravity_aligned, in bits."""
    rng = np.random.default_rng(13)
    for _ in range(50):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        pose = (tuple(rng.uniform(-20, 20, 3).tolist()), tuple(q.tolist()))
        tfl, lo = sup.tracking_from_local(pose)
        mine = ltb._tq(ltb._cast_f(ltb._inverse(ltb._rigid3d(pose))))
        sup.assert_same_bits(mine, tfl, "tracking_from_local")
        sup.assert_same_bits(np.array([np.float32(v) for v in pose[0]]), lo, "local origin")
        g = rng.normal(size=4)
        g /= np.linalg.norm(g) * rng.uniform(0.999, 1.001)
        assert ltb.local_from_gravity_aligned(pose[1], g) == \
            sup.local_from_gravity_aligned(pose[1], g)


def test_default_extrapolate_poses_with_gravity(ltb):
    """PoseExtrapolator::ExtrapolatePosesWithGravity's body over the 2D interface."""
    ex = sup.ScriptedExtrapolator3D(10.0, (1, 2, 3), (0.5, -0.25, 0.125), 0.2,
                                    sup.quat_from_rpy(0.01, 0.02, 0.0), use_default_body=True)
    times = [10.1, 10.2, 10.25]
    result = ltb.extrapolate_poses_with_gravity(ex, times)
    assert result.previous_poses.shape == (2, 7) and result.previous_poses.dtype == np.float32
    for row, t in zip(result.previous_poses, times[:-1]):
        p = ex._poses([t])[0]
        sup.assert_same_bits(row, p.astype(np.float32), "previous pose")
    p = ex._poses([times[-1]])[0]
    assert result.current_pose == (tuple(p[:3].tolist()), tuple(p[3:].tolist()))
    assert tuple(result.gravity_from_tracking) == ex.gravity_q
    assert ex.last_extrapolated_time == times[-1]


def test_design_and_integration_describe_the_3d_loop():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for needle in ("csm_voxel_filter_large", "csm_range_data3d_prepare", "csm_compute_histogram",
                   "LocalTrajectoryBuilder3D", "passes = rejections + 1"):
        assert needle in design, needle
    scope = design[design.index("## 9"):]
    assert "csm_compute_histogram" in scope[:scope.index("\n## ", 4)]
    assert "LocalTrajectoryBuilder3D" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "local_trajectory_builder_3d.h" in open(os.path.join(ROOT, "README.md")).read()
