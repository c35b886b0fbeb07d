"""Shared by the range-data insertion tests: the oracle shim
(tests/cpp/oracle_insert_shim.cc, built against oracle/_build/liboracle.so the
way test_builder_metrics.py builds its C++), an oracle grid wrapper with
misses, and the seeded scans the tests insert."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, ensure_built

SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "oracle_insert_shim.cc")
SHIM_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "liboracle_insert_shim.so")

F, I32, I64, VP = C.c_float, C.c_int32, C.c_int64, C.c_void_p
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
                           "-I", os.path.join(ROOT, "oracle"), SHIM_SRC, "-o", SHIM_LIB,
                           "-L", odir, "-loracle", "-Wl,-rpath," + odir])
    lib = C.CDLL(SHIM_LIB)
    lib.shim_ray_to_pixel_mask.restype = I64
    lib.shim_ray_to_pixel_mask.argtypes = [I32, I32, I32, I32, I32, P(I32), I64]
    lib.shim_lookup_table.restype = None
    lib.shim_lookup_table.argtypes = [F, P(C.c_uint16)]
    lib.shim_grid_insert.restype = None
    lib.shim_grid_insert.argtypes = [VP, F, F, I32, P(F), P(F), I32, P(F), I32]
    _shim = lib
    return lib


def oracle_mask(ray, scale):
    """oracle::RayToPixelMask of (bx, by, ex, ey): (k, 2) int32 cells."""
    lib = shim()
    out = np.zeros((4, 2), np.int32)
    n = lib.shim_ray_to_pixel_mask(*[int(v) for v in ray], scale, _p(out, I32), len(out))
    if n > len(out):
        out = np.zeros((n, 2), np.int32)
        lib.shim_ray_to_pixel_mask(*[int(v) for v in ray], scale, _p(out, I32), len(out))
    return out[:n]


def oracle_table(p):
    out = np.zeros(32768, np.uint16)
    shim().shim_lookup_table(p, _p(out, C.c_uint16))
    return out


class OracleGrid:
    """A ProbabilityGrid of the oracle (oracle_grid_create), inserted into
    through the shim."""

    def __init__(self, oracle, limits):
        self.o = oracle
        res, max_x, max_y, nx, ny = limits
        self.h = oracle.lib.oracle_grid_create(res, max_x, max_y, nx, ny)

    def insert(self, scan, hit, miss, free):
        origin, ret, mis = scan
        o = np.ascontiguousarray(origin, np.float32)
        r = np.ascontiguousarray(ret, np.float32).reshape(-1, 3)
        m = np.ascontiguousarray(mis, np.float32).reshape(-1, 3)
        shim().shim_grid_insert(self.h, hit, miss, int(free), _p(o, F), _p(r, F), len(r),
                                _p(m, F), len(m))

    def crop(self):
        self.o.lib.oracle_grid_crop(self.h)

    def get(self):
        """((resolution, max_x, max_y), cells[y, x])."""
        return self.o._grid_out(self.h)

    def close(self):
        if self.h:
            self.o.lib.oracle_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def limits_tuple(lim):
    return (lim.resolution, lim.max_x, lim.max_y, lim.num_x_cells, lim.num_y_cells)


def assert_same_grid(dev, ora, what=""):
    """Limits == and cells byte-equal between a DeviceProbabilityGrid and an
    OracleGrid."""
    host = dev.to_host()
    (res, max_x, max_y), cells = ora.get()
    got = (host.resolution, host.max_x, host.max_y, host.num_x_cells, host.num_y_cells)
    want = (res, max_x, max_y, cells.shape[1], cells.shape[0])
    assert got == want, (what, got, want)
    assert np.array_equal(host.cells, cells), (what, int((host.cells != cells).sum()))


def growth_scans(seed=7, num_scans=8, num_returns=256, num_misses=64):
    """The growth sequence: ranges 0.3-12 m all round, the sensor moving 0.4 m
    per scan. The longest range doubles per scan (1.5, 3, 6, 12 m), so from a
    100 x 100 grid at 0.05 m the grid grows in three separate inserts, to 800
    a side."""
    rng = np.random.default_rng(seed)
    scans = []
    for s in range(num_scans):
        origin = np.array([0.4 * s, 0.1 * s, 0.0], np.float32)
        far = min(12.0, 1.5 * 2 ** s)

        def ring(n):
            ang = rng.uniform(0, 2 * np.pi, n)
            rad = rng.uniform(0.3, far, n)
            pts = np.zeros((n, 3), np.float32)
            pts[:, 0] = origin[0] + rad * np.cos(ang)
            pts[:, 1] = origin[1] + rad * np.sin(ang)
            return pts
        ret = ring(num_returns)
        ret[0, :2] = origin[:2] + np.float32(far) * np.array([1.0, 0.0], np.float32)
        ret[1, :2] = origin[:2] - np.float32(far) * np.array([0.0, 1.0], np.float32)
        scans.append((origin, ret, ring(num_misses)))
    return scans


# kInitialSubmapSize grid at 0.05 m centred on the origin (submap_2d.cc:196-207).
INITIAL_LIMITS = (0.05, 2.5, 2.5, 100, 100)
