"""Shared by the LocalTrajectoryBuilder2D tests: the CPU restatement
(tests/cpp/oracle_local2d_shim.cc, built against oracle/_build/liboracle.so the
way intensity3d_support.py builds its shim), wrappers over it, the seeded room
sweeps with per-point poses the front-end tests feed, and the scripted
constant-velocity extrapolator of the builder tests."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import ROOT, ensure_built

SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "oracle_local2d_shim.cc")
SHIM_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "liboracle_local2d_shim.so")

F, D, I32, VP = C.c_float, C.c_double, C.c_int32, C.c_void_p
P = C.POINTER

_shim = None


def _p(a, t):
    return a.ctypes.data_as(P(t))


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
    lib.shiml_prepare.restype = None
    lib.shiml_prepare.argtypes = [P(F), P(F), P(I32), P(F), I32, P(F), P(F), P(F), P(F), P(F),
                                  P(I32), P(F), P(I32), P(F), P(I32)]
    lib.shiml_transform.restype = None
    lib.shiml_transform.argtypes = [P(F), P(F), P(F), I32, P(F), I32, P(F), P(F), P(F)]
    lib.shiml_gravity_from_local.restype = None
    lib.shiml_gravity_from_local.argtypes = [P(D), P(F), P(F)]
    lib.shiml_pose_prediction.restype = None
    lib.shiml_pose_prediction.argtypes = [P(D), P(D), P(D)]
    lib.shiml_pose_estimate.restype = None
    lib.shiml_pose_estimate.argtypes = [P(D), P(D), P(D)]
    lib.shiml_embed3d_f.restype = None
    lib.shiml_embed3d_f.argtypes = [P(D), P(F)]
    lib.shiml_motion_filter_create.restype = VP
    lib.shiml_motion_filter_create.argtypes = [D, D, D]
    lib.shiml_motion_filter_destroy.restype = None
    lib.shiml_motion_filter_destroy.argtypes = [VP]
    lib.shiml_motion_filter_is_similar.restype = I32
    lib.shiml_motion_filter_is_similar.argtypes = [VP, D, P(D)]
    _shim = lib
    return lib


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def options_array(o):
    """A RangeData2DOptions as the shim's nine floats."""
    a = o.adaptive_voxel_filter
    return np.array([o.min_range, o.max_range, o.missing_data_ray_length, o.min_z, o.max_z,
                     o.voxel_filter_size, a.max_length, a.min_num_points, a.max_range], np.float32)


def prepare(options, hits, origin_index, poses, origins, gravity_from_local, local_origin):
    """The restated front end: (origin, returns, misses, filtered)."""
    opts = options_array(options)
    h = _f32(hits, (-1, 3))
    n = len(h)
    idx = np.ascontiguousarray(np.asarray(origin_index, np.int32).reshape(-1))
    p = _f32(poses, (-1, 7))
    o = _f32(origins, (-1, 3))
    g = _f32(gravity_from_local, 7)
    lo = _f32(local_origin, 3)
    origin = np.zeros(3, np.float32)
    outs = [np.zeros((max(n, 1), 3), np.float32) for _ in range(3)]
    counts = [I32(0) for _ in range(3)]
    shim().shiml_prepare(_p(opts, F), _p(h, F), _p(idx, I32), _p(p, F), n, _p(o, F), _p(g, F),
                         _p(lo, F), _p(origin, F), _p(outs[0], F), C.byref(counts[0]),
                         _p(outs[1], F), C.byref(counts[1]), _p(outs[2], F), C.byref(counts[2]))
    return (origin,) + tuple(a[:c.value].copy() for a, c in zip(outs, counts))


def transform(tq, origin, returns, misses):
    """sensor::TransformRangeData restated: (origin, returns, misses)."""
    t = _f32(tq, 7)
    o = _f32(origin, 3)
    r = _f32(returns, (-1, 3))
    m = _f32(misses, (-1, 3))
    oo, ro, mo = np.zeros(3, np.float32), np.zeros_like(r), np.zeros_like(m)
    shim().shiml_transform(_p(t, F), _p(o, F), _p(r, F), len(r), _p(m, F), len(m), _p(oo, F),
                           _p(ro, F), _p(mo, F))
    return oo, ro, mo


def gravity_from_local(gravity_q, last_pose_tq):
    q = np.asarray(gravity_q, np.float64)
    p = _f32(last_pose_tq, 7)
    out = np.zeros(7, np.float32)
    shim().shiml_gravity_from_local(_p(q, D), _p(p, F), _p(out, F))
    return out


def _pose7(pose):
    return np.asarray(list(pose[0]) + list(pose[1]), np.float64)


def pose_prediction(pose, gravity_q):
    """Project2D(pose * gravity_alignment.inverse()) -> (x, y, angle)."""
    p, q, out = _pose7(pose), np.asarray(gravity_q, np.float64), np.zeros(3)
    shim().shiml_pose_prediction(_p(p, D), _p(q, D), _p(out, D))
    return tuple(out.tolist())


def pose_estimate(pose2d, gravity_q):
    """Embed3D(pose2d) * gravity_alignment -> (t, q)."""
    p, q, out = np.asarray(pose2d, np.float64), np.asarray(gravity_q, np.float64), np.zeros(7)
    shim().shiml_pose_estimate(_p(p, D), _p(q, D), _p(out, D))
    return tuple(out[:3].tolist()), tuple(out[3:].tolist())


def embed3d_f(pose2d):
    p, out = np.asarray(pose2d, np.float64), np.zeros(7, np.float32)
    shim().shiml_embed3d_f(_p(p, D), _p(out, F))
    return out


class ShimMotionFilter:
    """MotionFilter as the shim restates it."""

    def __init__(self, max_time_seconds, max_distance_meters, max_angle_radians):
        self._lib = shim()
        self.h = VP(self._lib.shiml_motion_filter_create(max_time_seconds, max_distance_meters,
                                                         max_angle_radians))

    def IsSimilar(self, time, pose):
        p = _pose7(pose)
        return bool(self._lib.shiml_motion_filter_is_similar(self.h, float(time), _p(p, D)))

    def __del__(self):
        if getattr(self, "h", None):
            self._lib.shiml_motion_filter_destroy(self.h)
            self.h = None


# ---- geometry for the inputs (double; the inputs only have to be plausible) ----

def quat_from_rpy(roll, pitch, yaw):
    """(w, x, y, z) of Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr = math.cos(roll / 2), math.sin(roll / 2)
    cp, sp = math.cos(pitch / 2), math.sin(pitch / 2)
    cy, sy = math.cos(yaw / 2), math.sin(yaw / 2)
    return (cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
            cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy)


def rotate(q, v):
    w, x, y, z = q
    v = np.asarray(v, np.float64)
    u = np.array([x, y, z])
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def room_hits(rng, n, half_x=4.0, half_y=3.0, z_jitter=0.05):
    """A 2D sweep of a (2 half_x) x (2 half_y) room seen from its centre: n
    points on the walls at evenly spread bearings, jittered in z."""
    ang = np.linspace(-np.pi, np.pi, n, endpoint=False) + rng.uniform(0, 1e-3, n)
    c, s = np.cos(ang), np.sin(ang)
    with np.errstate(divide="ignore"):
        r = np.minimum(half_x / np.abs(c), half_y / np.abs(s))
    pts = np.stack([r * c, r * s, rng.uniform(-z_jitter, z_jitter, n)], 1)
    return pts.astype(np.float32)


def random_poses(rng, n, angle=0.03, shift=0.1):
    """A different Rigid3f per point: small rotations about all three axes and
    small translations, (n, 7) as (t, q)."""
    out = np.zeros((n, 7), np.float32)
    for i in range(n):
        out[i, :3] = rng.uniform(-shift, shift, 3)
        out[i, 3:] = quat_from_rpy(*rng.uniform(-angle, angle, 3))
    return out


def identity_poses(n):
    out = np.zeros((n, 7), np.float32)
    out[:, 3] = 1.0
    return out


IDENTITY_TQ = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


class ScriptedExtrapolator:
    """Constant velocity from a start pose, a fixed small gravity tilt, and a
    record of AddPose: the five methods of PoseExtrapolatorInterface."""

    def __init__(self, start_time, start_xy_yaw, velocity_xy_yaw, tilt=(0.01, -0.015)):
        self.start_time = float(start_time)
        self.start = tuple(float(v) for v in start_xy_yaw)
        self.velocity = tuple(float(v) for v in velocity_xy_yaw)
        self.tilt = tilt
        self.gravity_q = quat_from_rpy(tilt[0], tilt[1], 0.0)
        self.last_pose_time = self.start_time
        self.last_extrapolated_time = self.start_time
        self.added = []

    def GetLastPoseTime(self):
        return self.last_pose_time

    def GetLastExtrapolatedTime(self):
        return self.last_extrapolated_time

    def ExtrapolatePose(self, time):
        dt = time - self.start_time
        x, y, yaw = (self.start[a] + self.velocity[a] * dt for a in range(3))
        self.last_extrapolated_time = time
        # The tracking frame is tilted against gravity by the inverse of the
        # alignment, so that aligned sweeps are level.
        q = quat_from_rpy(-self.tilt[0], -self.tilt[1], yaw)
        return ((x, y, 0.0), q)

    def EstimateGravityOrientation(self, time):
        return self.gravity_q

    def AddPose(self, time, pose):
        self.added.append((time, pose))
        self.last_pose_time = time
