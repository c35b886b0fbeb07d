"""Shared by the LocalTrajectoryBuilder3D tests: the CPU restatement
(tests/cpp/oracle_local3d_shim.cc, built against oracle/_build/liboracle.so the
way local2d_support.py builds its shim), wrappers over it, and the seeded
inputs: voxel-filter clouds, 3D room sweeps with a pose per point and three
origins."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, ensure_built
from local2d_support import quat_from_rpy, random_poses  # noqa: F401

SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "oracle_local3d_shim.cc")
SHIM_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "liboracle_local3d_shim.so")

F, D, I32, U8 = C.c_float, C.c_double, C.c_int32, C.c_uint8
P = C.POINTER

MINSTD_M = 2147483647
URNG_RANGE = 2147483645

# trajectory_builder_3d.lua:24-34.
HIGH_OPTIONS = (2.0, 150.0, 15.0)
LOW_OPTIONS = (4.0, 200.0, 60.0)

_shim = None


def _p(a, t):
    return a.ctypes.data_as(P(t)) if a is not None else None


def shim():
    """The compiled shim (once per process)."""
    global _shim
    if _shim is not None:
        return _shim
    ensure_built()
    os.makedirs(os.path.dirname(SHIM_LIB), exist_ok=True)
    odir = os.path.join(ROOT, "oracle", "_build")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle"), SHIM_SRC,
                           "-o", SHIM_LIB, "-L", odir, "-loracle", "-Wl,-rpath," + odir])
    lib = C.CDLL(SHIM_LIB)
    lib.shim3_adaptive.restype = I32
    lib.shim3_adaptive.argtypes = [P(F), I32, P(F), P(U8), P(I32)]
    lib.shim3_prepare.restype = None
    lib.shim3_prepare.argtypes = [P(F), P(F), P(F), P(I32), P(F), I32, P(F), P(F), P(F), P(F),
                                  P(F), P(F), P(I32), P(F), P(I32), P(F), P(F), P(I32), P(F),
                                  P(F), P(I32), P(I32)]
    lib.shim3_tracking_from_local.restype = None
    lib.shim3_tracking_from_local.argtypes = [P(D), P(F), P(F)]
    lib.shim3_histogram.restype = None
    lib.shim3_histogram.argtypes = [P(F), I32, P(D), I32, P(F)]
    lib.shim3_local_from_gravity_aligned.restype = None
    lib.shim3_local_from_gravity_aligned.argtypes = [P(D), P(D), P(D)]
    _shim = lib
    return lib


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def adaptive(cloud, options3):
    """(keep mask, VoxelFilter passes) of the restated AdaptiveVoxelFilter; the
    mask is checked against the oracle's AdaptiveVoxelFilterIndices."""
    pts = _f32(cloud, (-1, 3))
    opts = np.asarray(options3, np.float32)
    keep = np.zeros(max(len(pts), 1), np.uint8)
    passes = I32(0)
    agree = shim().shim3_adaptive(_p(pts, F), len(pts), _p(opts, F), _p(keep, U8),
                                  C.byref(passes))
    assert agree == 1, "the counted restatement differs from the oracle's adaptive filter"
    return keep[:len(pts)].astype(bool), passes.value


def options_array(o):
    """A RangeData3DOptions as the shim's nine floats."""
    h, l = o.high_resolution_adaptive_voxel_filter, o.low_resolution_adaptive_voxel_filter
    return np.array([o.min_range, o.max_range, o.voxel_filter_size, h.max_length,
                     h.min_num_points, h.max_range, l.max_length, l.min_num_points, l.max_range],
                    np.float32)


def prepare(options, hits, origin_index, poses, origins, tracking_from_local, local_origin,
            intensities=None):
    """The restated front end: the dict range_data3d_prepare returns, plus
    ``passes`` (the VoxelFilter passes of the high and the low adaptive filter)."""
    opts = options_array(options)
    h = _f32(hits, (-1, 3))
    n = len(h)
    idx = np.ascontiguousarray(np.asarray(origin_index, np.int32).reshape(-1))
    p = _f32(poses, (-1, 7))
    o = _f32(origins, (-1, 3))
    g = _f32(tracking_from_local, 7)
    lo = _f32(local_origin, 3)
    inten = None if intensities is None else _f32(intensities, -1)
    origin = np.zeros(3, np.float32)
    clouds = [np.zeros((max(n, 1), 3), np.float32) for _ in range(4)]
    ints = [np.zeros(max(n, 1), np.float32) for _ in range(3)]
    counts = [I32(0) for _ in range(4)]
    passes = np.zeros(2, np.int32)
    shim().shim3_prepare(_p(opts, F), _p(h, F), _p(inten, F), _p(idx, I32), _p(p, F), n, _p(o, F),
                         _p(g, F), _p(lo, F), _p(origin, F),
                         _p(clouds[0], F), _p(ints[0], F), C.byref(counts[0]),
                         _p(clouds[1], F), C.byref(counts[1]),
                         _p(clouds[2], F), _p(ints[1], F), C.byref(counts[2]),
                         _p(clouds[3], F), _p(ints[2], F), C.byref(counts[3]), _p(passes, I32))
    nr, nm, nh, nl = (c.value for c in counts)
    with_i = inten is not None
    return {"origin": origin, "returns": clouds[0][:nr].copy(), "misses": clouds[1][:nm].copy(),
            "high": clouds[2][:nh].copy(), "low": clouds[3][:nl].copy(),
            "returns_intensities": ints[0][:nr].copy() if with_i else None,
            "high_intensities": ints[1][:nh].copy() if with_i else None,
            "low_intensities": ints[2][:nl].copy() if with_i else None,
            "passes": tuple(int(v) for v in passes)}


def _pose7(pose):
    return np.asarray(list(pose[0]) + list(pose[1]), np.float64)


def tracking_from_local(pose):
    """(current_pose.inverse().cast<float>() as 7 floats, translation.cast<float>())."""
    p = _pose7(pose)
    tfl, lo = np.zeros(7, np.float32), np.zeros(3, np.float32)
    shim().shim3_tracking_from_local(_p(p, D), _p(tfl, F), _p(lo, F))
    return tfl, lo


def histogram(returns, gravity_q, size):
    r = _f32(returns, (-1, 3))
    q = np.asarray(gravity_q, np.float64)
    out = np.zeros(size, np.float32)
    shim().shim3_histogram(_p(r, F), len(r), _p(q, D), size, _p(out, F))
    return out


def local_from_gravity_aligned(pose_q, gravity_q):
    a, b, out = np.asarray(pose_q, np.float64), np.asarray(gravity_q, np.float64), np.zeros(4)
    shim().shim3_local_from_gravity_aligned(_p(a, D), _p(b, D), _p(out, D))
    return tuple(out.tolist())


def assert_same_bits(got, want, what):
    """Equal as bit patterns (so NaN equals NaN and -0 differs from 0)."""
    g = np.ascontiguousarray(np.asarray(got, np.float32))
    w = np.ascontiguousarray(np.asarray(want, np.float32))
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), what


def assert_prepared_equal(got, want):
    for key in ("origin", "returns", "misses", "high", "low"):
        assert_same_bits(got[key], want[key], key)
    for key in ("returns_intensities", "high_intensities", "low_intensities"):
        assert (got[key] is None) == (want[key] is None), key
        if want[key] is not None:
            assert_same_bits(got[key], want[key], key)


# ---- inputs ----------------------------------------------------------------

def cloud3d(n, seed, scale=20.0):
    """test_voxel_filter.py's cloud3d."""
    rng = np.random.RandomState(seed)
    pts = rng.randn(n, 3) * np.array([scale, scale, scale / 6])
    return pts.astype(np.float32)


def single_voxel_cloud(n, seed=7):
    """n points in one voxel at any resolution of 0.3 or more: the point of
    rank r draws with k = r + 1 at stream position r - 1 (plus rejections)."""
    rng = np.random.RandomState(seed)
    return (0.2 + 0.05 * rng.rand(n, 3)).astype(np.float32)


def rejected_points(n):
    """The points of a single voxel of n points whose draw meets a rejected
    minstd_rand0 output (libstdc++'s downscaling), walking the stream."""
    state, out = 1, []
    for point in range(1, n):
        k = point + 1
        past = k * (URNG_RANGE // k)
        while True:
            state = state * 16807 % MINSTD_M
            if state - 1 < past:
                break
            out.append(point)
    return out


def room_sweep(rng, n, half=(6.0, 4.5, 2.5), far_fraction=0.0, far=80.0):
    """n rays from near the centre of a (2 half) box, evenly spread over the
    sphere and jittered: the hits on the walls, (n, 3) float32. A fraction of
    the rays is pushed out to ``far`` metres (beyond any max_range)."""
    z = rng.uniform(-1.0, 1.0, n)
    az = rng.uniform(-np.pi, np.pi, n)
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(az), s * np.sin(az), z], 1)
    with np.errstate(divide="ignore"):
        t = np.min(np.asarray(half)[None, :] / np.abs(d), axis=1)
    if far_fraction > 0:
        t = np.where(rng.rand(n) < far_fraction, far, t)
    return (d * t[:, None]).astype(np.float32)


ORIGINS = np.array([[0.0, 0.0, 0.0], [0.1, -0.05, 0.2], [-0.15, 0.1, 0.05]], np.float32)


def sweep_inputs(n, seed, with_intensities=True, far_fraction=0.02):
    """hits, origin indices (three origins), a pose per point, intensities."""
    rng = np.random.RandomState(seed)
    hits = room_sweep(rng, n, far_fraction=far_fraction) if n else np.zeros((0, 3), np.float32)
    idx = rng.randint(0, len(ORIGINS), n).astype(np.int32)
    poses = pose_table(rng, n)
    inten = rng.uniform(0.0, 100.0, n).astype(np.float32) if with_intensities else None
    return hits, idx, poses, inten


def pose_table(rng, n, distinct=257):
    """A pose per point drawn from a table of `distinct` small motions (quick
    to make for large n; every point still goes through its own row)."""
    table = random_poses(rng, min(max(n, 1), distinct))
    return np.ascontiguousarray(table[rng.randint(0, len(table), n)]) if n else \
        np.zeros((0, 7), np.float32)


# ---- the builder's world -------------------------------------------------------

def quat_rotate(q, v):
    """Rotates the rows of v (n, 3) by q = (w, x, y, z), in double."""
    w, u = q[0], np.asarray(q[1:], np.float64)
    v = np.asarray(v, np.float64)
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def quat_conjugate(q):
    return (q[0], -q[1], -q[2], -q[3])


def quat_from_angle_axis(angle, axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    s = np.sin(0.5 * angle)
    return (float(np.cos(0.5 * angle)), float(s * a[0]), float(s * a[1]), float(s * a[2]))


def box_returns(directions, pose, half, bubbles=None, bubble_radius=0.5):
    """What a rangefinder at ``pose`` (inside the axis-aligned box of half edge
    ``half`` about the origin) sees along ``directions`` (n, 3, tracking frame):
    the hits on the box, or on the nearest of the ``bubbles`` (m, 3) before it,
    as (n, 3) float32 in the tracking frame."""
    t, q = np.asarray(pose[0], np.float64), pose[1]
    d = quat_rotate(q, directions)
    with np.errstate(divide="ignore", invalid="ignore"):
        lim = np.where(d > 0, (half - t) / d, np.where(d < 0, (-half - t) / d, np.inf))
    reach = lim.min(axis=1)
    if bubbles is not None:
        for c in np.asarray(bubbles, np.float64):
            oc = t - c
            b = d @ oc
            disc = b * b - (oc @ oc - bubble_radius * bubble_radius)
            hit = disc >= 0
            s = -b - np.sqrt(np.where(hit, disc, 0.0))
            reach = np.where(hit & (s >= 0) & (s < reach), s, reach)
    return (np.asarray(directions, np.float64) * reach[:, None]).astype(np.float32)


def sphere_directions(rng, n):
    z = rng.uniform(-1.0, 1.0, n)
    az = rng.uniform(-np.pi, np.pi, n)
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(az), s * np.sin(az), z], 1)


class ScriptedExtrapolator3D:
    """Constant linear and yaw velocity from a start pose, a fixed gravity
    estimate and a record of AddPose. ExtrapolatePosesWithGravity is the
    interface's default body, vectorised; ``use_default_body`` leaves it to
    the builder's default instead."""

    def __init__(self, start_time, start_xyz, velocity_xyz, yaw_rate=0.0,
                 gravity_q=(1.0, 0.0, 0.0, 0.0), use_default_body=False):
        self.start_time = float(start_time)
        self.start = np.asarray(start_xyz, np.float64)
        self.velocity = np.asarray(velocity_xyz, np.float64)
        self.yaw_rate = float(yaw_rate)
        self.gravity_q = tuple(float(v) for v in gravity_q)
        self.last_pose_time = self.start_time
        self.last_extrapolated_time = self.start_time
        self.added = []
        self.answers = []  # what ExtrapolatePosesWithGravity returned, in order
        if use_default_body:
            self.ExtrapolatePosesWithGravity = None

    def GetLastPoseTime(self):
        return self.last_pose_time

    def GetLastExtrapolatedTime(self):
        return self.last_extrapolated_time

    def _poses(self, times):
        dt = np.asarray(times, np.float64) - self.start_time
        t = self.start[None, :] + self.velocity[None, :] * dt[:, None]
        half = 0.5 * self.yaw_rate * dt
        q = np.stack([np.cos(half), 0.0 * half, 0.0 * half, np.sin(half)], 1)
        return np.concatenate([t, q], 1)

    def ExtrapolatePose(self, time):
        self.last_extrapolated_time = time
        p = self._poses([time])[0]
        return (tuple(p[:3].tolist()), tuple(p[3:].tolist()))

    def EstimateGravityOrientation(self, time):
        return self.gravity_q

    def ExtrapolatePosesWithGravity(self, times):
        from cartographer_amd.local_trajectory_builder_3d import ExtrapolationResult
        p = self._poses(times)
        self.last_extrapolated_time = float(times[-1])
        current = (tuple(p[-1, :3].tolist()), tuple(p[-1, 3:].tolist()))
        self.answers.append(ExtrapolationResult(p[:-1].astype(np.float32), current, self.gravity_q))
        return self.answers[-1]

    def AddPose(self, time, pose):
        self.added.append((time, pose))
        self.last_pose_time = time
