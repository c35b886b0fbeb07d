"""Shared by the TSDF range-data insertion tests: the oracle shim
(tests/cpp/oracle_tsdf_shim.cc, built against oracle/_build/liboracle.so the
way insert2d_support.py builds its shim), an oracle TSDF2D wrapper, the inputs
(`growth`, `room`, `dup`) and the option sets A-F."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, ensure_built
from insert2d_support import INITIAL_LIMITS, growth_scans  # noqa: F401
from oracle_lib import Oracle

SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "oracle_tsdf_shim.cc")
SHIM_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "liboracle_tsdf_shim.so")

F, D, I32, I64, U16 = C.c_float, C.c_double, C.c_int32, C.c_int64, C.c_uint16
P = C.POINTER

TRUNCATION, MAX_WEIGHT = 0.3, 10.0

# Options in proto order: truncation_distance, maximum_weight,
# update_free_space, num_normal_samples, sample_radius,
# project_sdf_distance_to_scan_normal, update_weight_range_exponent, angle
# bandwidth, distance bandwidth.
_A = tuple(Oracle.TSDF_TEST_OPTIONS)
OPTION_SETS = {
    "A": _A,
    "B": _A[:2] + (1,) + _A[3:],
    "C": _A[:5] + (0,) + _A[6:7] + (0.0,) + _A[8:],   # no sort, no normals
    "D": (0.3, 10.0, 1, 8, 0.3, 0, 2, 0.5, 0.5),
    "E": _A[:7] + (0.02,) + _A[8:],                   # most rays weigh exactly 0
    "F": _A[:2] + (1,) + _A[3:7] + (0.02,) + _A[8:],
}

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
    lib.shim_tsdf_out_of_order.restype = I32
    lib.shim_tsdf_out_of_order.argtypes = [P(F), P(F), I32, P(I32)]
    lib.shim_tsdf_normals.restype = None
    lib.shim_tsdf_normals.argtypes = [P(F), P(F), I32, I32, F, P(F)]
    lib.shim_tsdf_round_trip.restype = None
    lib.shim_tsdf_round_trip.argtypes = [F, F, P(U16), P(U16)]
    lib.shim_tsdf_crop.restype = I64
    lib.shim_tsdf_crop.argtypes = [D, D, D, I32, I32, F, F, P(U16), P(U16), P(D), P(I32), P(U16),
                                   P(U16), I64]
    _shim = lib
    return lib


def out_of_order(origin, returns, order):
    o = np.ascontiguousarray(origin, np.float32)
    r = np.ascontiguousarray(returns, np.float32)
    k = np.ascontiguousarray(order, np.int32)
    return int(shim().shim_tsdf_out_of_order(_p(o, F), _p(r, F), len(r), _p(k, I32)))


def oracle_normals(origin, returns, num_samples, radius):
    o = np.ascontiguousarray(origin, np.float32)
    r = np.ascontiguousarray(returns, np.float32)
    out = np.zeros(len(r), np.float32)
    shim().shim_tsdf_normals(_p(o, F), _p(r, F), len(r), num_samples, radius, _p(out, F))
    return out


def oracle_round_trip(truncation, max_weight):
    t = np.zeros(32768, np.uint16)
    w = np.zeros(32768, np.uint16)
    shim().shim_tsdf_round_trip(truncation, max_weight, _p(t, U16), _p(w, U16))
    return t, w


def oracle_crop(limits, tsd, wgt, truncation, max_weight):
    """ComputeCroppedGrid: ((res, max_x, max_y, nx, ny), tsd[y, x], weight[y, x])."""
    res, max_x, max_y = limits
    tsd = np.ascontiguousarray(tsd, np.uint16)
    wgt = np.ascontiguousarray(wgt, np.uint16)
    ny, nx = tsd.shape
    lim = np.zeros(3)
    cells = np.zeros(2, np.int32)
    t = np.zeros(tsd.size, np.uint16)
    w = np.zeros(tsd.size, np.uint16)
    n = shim().shim_tsdf_crop(res, max_x, max_y, nx, ny, truncation, max_weight, _p(tsd, U16),
                              _p(wgt, U16), _p(lim, D), _p(cells, I32), _p(t, U16), _p(w, U16),
                              t.size)
    shape = (int(cells[1]), int(cells[0]))
    return ((float(lim[0]), float(lim[1]), float(lim[2]), int(cells[0]), int(cells[1])),
            t[:n].reshape(shape), w[:n].reshape(shape))


class OracleTSDF:
    """A TSDF2D of the oracle (oracle_tsdf_create) and its restated inserter."""

    def __init__(self, oracle, limits=INITIAL_LIMITS, truncation=TRUNCATION,
                 max_weight=MAX_WEIGHT):
        self.lib = oracle.lib
        res, max_x, max_y, nx, ny = limits
        self.h = self.lib.oracle_tsdf_create(res, max_x, max_y, nx, ny, truncation, max_weight)

    def insert(self, scan, options):
        o = np.ascontiguousarray(scan[0], np.float32)
        r = np.ascontiguousarray(scan[1], np.float32).reshape(-1, 3)
        opts = np.asarray(options, np.float64)
        self.lib.oracle_tsdf_insert(self.h, _p(opts, D), _p(o, F), _p(r, F), len(r))

    def get(self):
        """((resolution, max_x, max_y), tsd[y, x], weight[y, x])."""
        info = np.zeros(3)
        cells = np.zeros(2, np.int32)
        self.lib.oracle_tsdf_info(self.h, _p(info, D), _p(cells, I32))
        tsd = np.zeros((cells[1], cells[0]), np.uint16)
        wgt = np.zeros_like(tsd)
        self.lib.oracle_tsdf_cells(self.h, _p(tsd, U16), _p(wgt, U16))
        return (float(info[0]), float(info[1]), float(info[2])), tsd, wgt

    def close(self):
        if self.h:
            self.lib.oracle_tsdf_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def new_device_grid(csm, limits=INITIAL_LIMITS, truncation=TRUNCATION, max_weight=MAX_WEIGHT):
    return csm.DeviceTSDF2D(*limits, truncation, max_weight)


def assert_same_tsdf(dev, ora, what=""):
    """Limits == and both planes byte-equal between a DeviceTSDF2D and an
    OracleTSDF."""
    host = dev.to_host()
    (res, max_x, max_y), tsd, wgt = ora.get()
    got = (host.resolution, host.max_x, host.max_y, host.num_x_cells, host.num_y_cells)
    want = (res, max_x, max_y, tsd.shape[1], tsd.shape[0])
    assert got == want, (what, got, want)
    assert np.array_equal(host.tsd_cells, tsd), (what, "tsd", int((host.tsd_cells != tsd).sum()))
    assert np.array_equal(host.weight_cells, wgt), (what, "weight",
                                                    int((host.weight_cells != wgt).sum()))


# ---- inputs ----------------------------------------------------------------

def growth():
    """insert2d_support.growth_scans(seed=7), returns only: 8 x 256, the grid
    grows in three inserts to 800 x 800."""
    return [(o, r) for o, r, _ in growth_scans(seed=7)]


def _room_scan(rng, origin, beams):
    """One scan of the inside of the rectangle |x| <= 4, |y| <= 3 from
    `origin`, 1 cm Gaussian range noise."""
    ang = np.linspace(0.0, 2.0 * np.pi, beams, endpoint=False) + 0.003
    dx, dy = np.cos(ang), np.sin(ang)
    with np.errstate(divide="ignore"):
        tx = np.where(dx > 0, (4.0 - origin[0]) / dx, (-4.0 - origin[0]) / dx)
        ty = np.where(dy > 0, (3.0 - origin[1]) / dy, (-3.0 - origin[1]) / dy)
    rng_m = np.minimum(tx, ty) + rng.normal(0.0, 0.01, beams)
    pts = np.zeros((beams, 3), np.float32)
    pts[:, 0] = origin[0] + rng_m * dx
    pts[:, 1] = origin[1] + rng_m * dy
    return np.asarray(origin, np.float32), pts


def room(seed=11):
    """A sensor stepping through an 8 x 6 m rectangle: 6 scans of 360 beams,
    then 4 of 1080. Neighbouring beams share cells, so the first-writer rule
    decides thousands of cells; the grid reaches 200 x 200."""
    rng = np.random.default_rng(seed)
    scans = []
    for s in range(10):
        origin = np.array([-2.0 + 0.45 * s, -1.0 + 0.2 * s, 0.0])
        scans.append(_room_scan(rng, origin, 360 if s < 6 else 1080))
    return scans


def dup():
    """Origin (0, 0, 0), 128 bearings, each with a return at (x, y) and one at
    exactly (2x, 2y) in float: the two normalize to identical floats, so the
    sort's permutation among equivalent returns decides the result."""
    ang = np.linspace(0.0, 2.0 * np.pi, 128, endpoint=False) + 0.01
    near = np.zeros((128, 3), np.float32)
    near[:, 0] = (0.9 * np.cos(ang)).astype(np.float32)
    near[:, 1] = (0.9 * np.sin(ang)).astype(np.float32)
    far = near * np.float32(2.0)
    pts = np.empty((256, 3), np.float32)
    pts[0::2] = near
    pts[1::2] = far
    return [(np.zeros(3, np.float32), pts)]


def shuffled(scans, seed=5):
    rng = np.random.default_rng(seed)
    return [(o, np.ascontiguousarray(r[rng.permutation(len(r))])) for o, r in scans]


INPUTS = {"growth": growth, "room": room, "dup": dup}
