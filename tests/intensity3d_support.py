"""Shared by the IntensityHybridGrid tests: the CPU restatement
(tests/cpp/oracle_intensity3d_shim.cc, built against oracle/_build/liboracle.so
the way insert3d_support.py builds its shim), the "same intensity grid"
comparison of a device grid with it, and seeded intensities."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT, ensure_built

SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "oracle_intensity3d_shim.cc")
SHIM_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "liboracle_intensity3d_shim.so")

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
    lib.shimi_create.restype = C.c_void_p
    lib.shimi_create.argtypes = [F]
    lib.shimi_destroy.restype = None
    lib.shimi_destroy.argtypes = [C.c_void_p]
    lib.shimi_grid_size.restype = I32
    lib.shimi_grid_size.argtypes = [C.c_void_p]
    lib.shimi_add_intensity.restype = None
    lib.shimi_add_intensity.argtypes = [C.c_void_p, I32, I32, I32, F]
    lib.shimi_get_intensity.restype = None
    lib.shimi_get_intensity.argtypes = [C.c_void_p, P(I32), I64, P(F)]
    lib.shimi_insert.restype = None
    lib.shimi_insert.argtypes = [C.c_void_p, P(F), P(F), I64, F]
    lib.shimi_cells.restype = I64
    lib.shimi_cells.argtypes = [C.c_void_p, P(I32), P(F), P(I32)]
    lib.shimi_cost_block.restype = None
    lib.shimi_cost_block.argtypes = [C.c_void_p, P(F), P(F), I32, P(D), D, F, P(D), P(D)]
    lib.shimi_huber.restype = None
    lib.shimi_huber.argtypes = [D, D, P(D)]
    lib.shimi_ceres3d_match.restype = I32
    lib.shimi_ceres3d_match.argtypes = [C.c_void_p, C.c_void_p, P(F), I32, P(F), I32, P(D), P(D),
                                        P(D), C.c_void_p, P(F), P(D), P(D), P(D)]
    _shim = lib
    return lib


class OracleIntensityGrid:
    """IntensityHybridGrid as the shim restates it."""

    def __init__(self, resolution):
        self._lib = shim()
        self.resolution = float(resolution)
        self.handle = C.c_void_p(self._lib.shimi_create(self.resolution))

    def __del__(self):
        if getattr(self, "handle", None):
            self._lib.shimi_destroy(self.handle)
            self.handle = None

    @property
    def grid_size(self):
        return int(self._lib.shimi_grid_size(self.handle))

    def add_intensity(self, index, intensity):
        x, y, z = (int(v) for v in index)
        self._lib.shimi_add_intensity(self.handle, x, y, z, float(np.float32(intensity)))

    def get_intensity(self, indices):
        idx = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1, 3))
        out = np.zeros(len(idx), np.float32)
        self._lib.shimi_get_intensity(self.handle, _p(idx, I32), len(idx), _p(out, F))
        return out

    def insert(self, returns, intensities, threshold):
        """InsertIntensitiesIntoGrid: returns in the grid's frame."""
        r = np.ascontiguousarray(np.asarray(returns, np.float32).reshape(-1, 3))
        v = None
        if intensities is not None:
            v = np.ascontiguousarray(np.asarray(intensities, np.float32).reshape(-1))
            assert len(v) == len(r)
        self._lib.shimi_insert(self.handle, _p(r, F), None if v is None else _p(v, F), len(r),
                               float(np.float32(threshold)))

    def cells(self):
        n = int(self._lib.shimi_cells(self.handle, None, None, None))
        ijk = np.zeros((n, 3), np.int32)
        sums = np.zeros(n, np.float32)
        counts = np.zeros(n, np.int32)
        if n:
            self._lib.shimi_cells(self.handle, _p(ijk, I32), _p(sums, F), _p(counts, I32))
        return ijk, sums, counts

    def box(self):
        """((origin3, dims3, grid_size), sums[z, y, x], counts[z, y, x]) over
        the box of the cells with count > 0."""
        ijk, sums, counts = self.cells()
        assert (counts > 0).all()
        if len(ijk) == 0:
            e = np.zeros((0, 0, 0))
            return ((0, 0, 0), (0, 0, 0), self.grid_size), e.astype(np.float32), e.astype(np.int32)
        lo, hi = ijk.min(0), ijk.max(0)
        d = hi - lo + 1
        bs = np.zeros((d[2], d[1], d[0]), np.float32)
        bc = np.zeros((d[2], d[1], d[0]), np.int32)
        at = (ijk[:, 2] - lo[2], ijk[:, 1] - lo[1], ijk[:, 0] - lo[0])
        bs[at] = sums
        bc[at] = counts
        return (tuple(int(x) for x in lo), tuple(int(x) for x in d), self.grid_size), bs, bc


def assert_same_intensity_grid(dev, ora, what="", rng=None):
    """csm_intensity_grid_info == (box of the restatement's cells, its
    DynamicGrid size); csm_intensity_grid_read == its sums and counts scattered
    into that box, bit for bit; csm_intensity_grid_get_intensity == its
    GetIntensity, bit for bit, at every cell of the box, one cell beyond each
    face and a few far away."""
    want_info, want_s, want_c = ora.box()
    got_info = dev.info()
    if want_c.size == 0:
        assert got_info[1] == (0, 0, 0) and got_info[2] == want_info[2], (what, got_info, want_info)
        assert dev.device_bytes() == 0, what
        probe = np.array([[0, 0, 0], [1, -2, 3]], np.int32)
        assert dev.get_intensity(probe).tobytes() == np.zeros(2, np.float32).tobytes(), what
        return
    assert got_info == want_info, (what, got_info, want_info)
    got_s, got_c = dev.read()
    assert got_c.shape == want_c.shape and got_s.shape == want_s.shape, what
    assert got_c.tobytes() == want_c.tobytes(), (what, int((got_c != want_c).sum()))
    assert got_s.tobytes() == want_s.tobytes(), \
        (what, int((got_s.view(np.uint32) != want_s.view(np.uint32)).sum()))
    (ox, oy, oz), (nx, ny, nz), _ = got_info
    if (nx + 2) * (ny + 2) * (nz + 2) <= 20000:
        z, y, x = np.meshgrid(np.arange(oz - 1, oz + nz + 1), np.arange(oy - 1, oy + ny + 1),
                              np.arange(ox - 1, ox + nx + 1), indexing="ij")
        idx = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)
    else:  # a large box: every known cell and a seeded sample of the rest
        rng = rng or np.random.default_rng(3)
        lo = np.array([ox - 1, oy - 1, oz - 1])
        sample = lo + rng.integers(0, np.array([nx + 2, ny + 2, nz + 2]), (20000, 3))
        idx = np.concatenate([ora.cells()[0], sample.astype(np.int32)])
    far = np.array([[ox - 1000, oy, oz], [ox, oy + 100000, oz], [2 ** 30, -2 ** 30, 0]], np.int32)
    idx = np.ascontiguousarray(np.concatenate([idx, far]))
    assert dev.get_intensity(idx).tobytes() == ora.get_intensity(idx).tobytes(), what


def cost_block(grid, points, intensities, pose, scale, threshold):
    """IntensityCostFunction3D alone on an OracleIntensityGrid at pose (t, q):
    (residuals (n,), Jacobian (n, 6) in the tangent space), no loss."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(intensities, np.float32).reshape(-1)
    p = np.concatenate([np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)])
    r = np.zeros(len(pts))
    J = np.zeros((len(pts), 6))
    shim().shimi_cost_block(grid.handle, _p(pts, F), _p(v, F), len(pts), _p(p, D), float(scale),
                            float(np.float32(threshold)), _p(r, D), _p(J, D))
    return r, J


def huber(a, s):
    """ceres::HuberLoss(a) at s: (rho, rho', rho'')."""
    out = np.zeros(3)
    shim().shimi_huber(float(a), float(s), _p(out, D))
    return tuple(out)


def ceres3d_match(high, low, high_cloud, low_cloud, options, target, initial_t, initial_q,
                  intensity_grid=None, intensities=None, intensity_options=None):
    """CeresScanMatcher3D::Match restated with the optional intensity block on
    the high-resolution cloud: ((t, q), iterations, S at the initial pose).
    high / low: oracle_lib OracleHybridGrid objects; options as
    Oracle.ceres3d_match takes them; intensity_options: (weight, huber_scale,
    intensity_threshold)."""
    hc = np.ascontiguousarray(high_cloud, np.float32).reshape(-1, 3)
    lc = np.ascontiguousarray(low_cloud, np.float32).reshape(-1, 3)
    o = np.asarray(tuple(options) + ((0.0,) if len(options) == 5 else ()), np.float64)
    t = np.asarray(target, np.float64)
    init = np.concatenate([np.asarray(initial_t, np.float64), np.asarray(initial_q, np.float64)])
    out = np.zeros(7)
    s0 = D()
    v = io = None
    if intensity_grid is not None:
        v = np.ascontiguousarray(intensities, np.float32).reshape(-1)
        assert len(v) == len(hc)
        io = np.asarray(intensity_options, np.float64)
    it = shim().shimi_ceres3d_match(
        high.h, low.h, _p(hc, F), len(hc), _p(lc, F), len(lc), _p(o, D), _p(t, D), _p(init, D),
        None if intensity_grid is None else intensity_grid.handle,
        None if v is None else _p(v, F), None if io is None else _p(io, D), _p(out, D),
        C.byref(s0))
    return (tuple(out[:3]), tuple(out[3:])), int(it), s0.value


def seeded_intensities(n, seed, low=0.0, high=255.0):
    return np.random.default_rng(seed).uniform(low, high, n).astype(np.float32)
