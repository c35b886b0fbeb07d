"""Shared by the 3D range-data insertion tests: the oracle shim
(tests/cpp/oracle_insert3d_shim.cc, built against oracle/_build/liboracle.so
exactly as insert2d_support.py builds its shim), the "same grid" comparison of
a device HybridGrid with an OracleHybridGrid, and the seeded scans."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, ensure_built

SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "oracle_insert3d_shim.cc")
SHIM_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "liboracle_insert3d_shim.so")

F, D, I32, I64 = C.c_float, C.c_double, C.c_int32, C.c_int64
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
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle"), SHIM_SRC,
                           "-o", SHIM_LIB, "-L", odir, "-loracle", "-Wl,-rpath," + odir])
    lib = C.CDLL(SHIM_LIB)
    lib.shim3_lookup_table.restype = None
    lib.shim3_lookup_table.argtypes = [F, P(C.c_uint16)]
    lib.shim3_rotate_histogram.restype = None
    lib.shim3_rotate_histogram.argtypes = [P(F), I32, F, P(F)]
    lib.shim3_apply.restype = None
    lib.shim3_apply.argtypes = [P(F), P(F), I64, P(F)]
    lib.shim3_inverse.restype = None
    lib.shim3_inverse.argtypes = [P(F), P(F)]
    lib.shim3_cast_inverse.restype = None
    lib.shim3_cast_inverse.argtypes = [P(D), P(F)]
    lib.shim3_norm.restype = F
    lib.shim3_norm.argtypes = [P(F)]
    lib.shim3_yaw_in_submap.restype = F
    lib.shim3_yaw_in_submap.argtypes = [P(D), P(D)]
    _shim = lib
    return lib


def oracle_table(p):
    out = np.zeros(32768, np.uint16)
    shim().shim3_lookup_table(p, _p(out, C.c_uint16))
    return out


def oracle_rotate_histogram(h, angle):
    h = np.ascontiguousarray(h, np.float32)
    out = np.zeros_like(h)
    shim().shim3_rotate_histogram(_p(h, F), len(h), float(np.float32(angle)), _p(out, F))
    return out


def pose7f(t, q):
    return np.array(list(t) + list(q), np.float32)


def oracle_apply(pose7, points):
    """oracle::Apply3 of a float pose (t, then q as w, x, y, z) on (n, 3) points."""
    pose7 = np.ascontiguousarray(pose7, np.float32)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    out = np.zeros_like(pts)
    shim().shim3_apply(_p(pose7, F), _p(pts, F), len(pts), _p(out, F))
    return out


def oracle_cast_inverse(t, q):
    """CastF(Inverse(Rigid3d(t, q))): float pose7."""
    p = np.array(list(t) + list(q), np.float64)
    out = np.zeros(7, np.float32)
    shim().shim3_cast_inverse(_p(p, D), _p(out, F))
    return out


def oracle_norm(v):
    v = np.ascontiguousarray(v, np.float32)
    return float(shim().shim3_norm(_p(v, F)))


def oracle_yaw_in_submap(local_q, gravity_q):
    a = np.array(local_q, np.float64)
    b = np.array(gravity_q, np.float64)
    return float(shim().shim3_yaw_in_submap(_p(a, D), _p(b, D)))


def oracle_job(origin, returns, pose7=None, max_range=None):
    """The (origin, returns) one batch job inserts: transformed by Apply3, then
    filtered by NormF(p - origin) <= max_range (submap_3d.cc:91-99)."""
    org = np.asarray(origin, np.float32).reshape(1, 3)
    ret = np.ascontiguousarray(returns, np.float32).reshape(-1, 3)
    if pose7 is not None:
        org = oracle_apply(pose7, org)
        ret = oracle_apply(pose7, ret)
    if max_range is not None and max_range > 0:
        mr = np.float32(max_range)
        keep = [np.float32(oracle_norm(p - org[0])) <= mr for p in ret]
        ret = ret[np.array(keep, bool)] if len(ret) else ret
    return org[0], ret


def oracle_box(ora):
    """((origin3, dims3, grid_size), brick[z, y, x]) of an OracleHybridGrid: the
    box of its cells() and the cells scattered into it."""
    ijk, v = ora.cells()
    if len(v) == 0:
        return ((0, 0, 0), (0, 0, 0), ora.grid_size), np.zeros((0, 0, 0), np.uint16)
    lo, hi = ijk.min(0), ijk.max(0)
    d = hi - lo + 1
    brick = np.zeros((d[2], d[1], d[0]), np.uint16)
    brick[ijk[:, 2] - lo[2], ijk[:, 1] - lo[1], ijk[:, 0] - lo[0]] = v
    return (tuple(int(x) for x in lo), tuple(int(x) for x in d), ora.grid_size), brick


def assert_same_grid(dev, ora, what=""):
    """csm_hybrid_grid_info == (box of the oracle's cells, its grid_size) and
    csm_hybrid_grid_read == the oracle's cells scattered into that box, byte
    for byte."""
    want_info, want = oracle_box(ora)
    got_info = dev.info()
    if want.size == 0:  # nothing known: the device grid has no box either
        assert got_info[1] == (0, 0, 0) and got_info[2] == want_info[2], (what, got_info, want_info)
        return
    assert got_info == want_info, (what, got_info, want_info)
    got = dev.values()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()))


def sphere_scan(rng, origin, n, near, far):
    """n returns all round the origin at ranges in [near, far]."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = rng.uniform(near, far, (n, 1))
    return (np.asarray(origin, np.float32),
            (np.asarray(origin, np.float64) + d * r).astype(np.float32))


def growth_scans(seed=11, num_scans=8, num_returns=256):
    """The growth sequence: the sensor moves 0.5 m per scan along (+x, -y, +z)
    and the longest range doubles per scan from 1 m, capped at 16 m, so the
    brick grows in every direction."""
    rng = np.random.default_rng(seed)
    scans = []
    for s in range(num_scans):
        origin = np.array([0.5 * s, -0.5 * s, 0.5 * s], np.float32)
        far = min(16.0, 2.0 ** s)
        scans.append(sphere_scan(rng, origin, num_returns, 0.3 * far, far))
    return scans


def yaw_quat(yaw):
    return (float(np.cos(0.5 * yaw)), 0.0, 0.0, float(np.sin(0.5 * yaw)))
