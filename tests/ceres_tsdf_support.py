"""Shared by the TSDF Ceres tests: the CPU restatement of
CeresScanMatcher2D::Match on a TSDF2D (tests/cpp/oracle_ceres_tsdf_shim.cc,
built against oracle/_build/liboracle.so the way tsdf_support.py builds its
shim), the reference's cost-function fixture, the `room` TSDF with its clouds,
and a numpy restatement of the PrecomputationGridStack2D levels."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import tsdf_support as ts
from conftest import ROOT, ensure_built
from oracle_lib import Oracle

SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "oracle_ceres_tsdf_shim.cc")
SHIM_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "liboracle_ceres_tsdf_shim.so")

F, D, I32, U16 = C.c_float, C.c_double, C.c_int32, C.c_uint16
P = C.POINTER

# test_ceres2d.py:114's four option sets, each with both settings of
# use_nonmonotonic_steps: (occupied, translation, rotation, iterations, nonmonotonic).
OPTION_SETS = [o + (nm,) for o in [(20.0, 10.0, 1.0, 10), (5.0, 1.0, 0.5, 25),
                                   (20.0, 10.0, 1.0, 1)] for nm in (True, False)]

_shim = None


def _p(a, t):
    return a.ctypes.data_as(P(t))


def shim():
    """The compiled restatement (once per process)."""
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
    grid = [D, D, D, I32, I32, F, F, P(U16), P(U16)]
    lib.shim_ceres_tsdf_evaluate.restype = I32
    lib.shim_ceres_tsdf_evaluate.argtypes = grid + [P(F), I32, D, P(D), P(D), P(D)]
    lib.shim_ceres_tsdf_match.restype = I32
    lib.shim_ceres_tsdf_match.argtypes = grid + [P(D), P(D), P(D), P(F), I32, P(D), P(I32)]
    lib.shim_interpolated_tsdf_ref_tests.restype = I32
    lib.shim_interpolated_tsdf_ref_tests.argtypes = []
    _shim = lib
    return lib


def _grid_args(grid):
    """A TSDF2D (the package's dataclass) as the shim's leading arguments; the
    arrays are returned too so that they outlive the call."""
    tsd = np.ascontiguousarray(grid.tsd_cells, np.uint16)
    wgt = np.ascontiguousarray(grid.weight_cells, np.uint16)
    return ([grid.resolution, grid.max_x, grid.max_y, grid.num_x_cells, grid.num_y_cells,
             grid.truncation_distance, grid.max_weight, _p(tsd, U16), _p(wgt, U16)], (tsd, wgt))


def _cloud(points):
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    return pts


def restated_evaluate(grid, cloud, scaling, pose):
    """TSDFMatchCostFunction2D at `pose`: (valid, residuals (n,), jacobian (n, 3))."""
    args, keep = _grid_args(grid)
    pts = _cloud(cloud)
    pose = np.asarray(pose, np.float64)
    res = np.zeros(len(pts))
    jac = np.zeros((len(pts), 3))
    ok = shim().shim_ceres_tsdf_evaluate(*args, _p(pts, F), len(pts), float(scaling), _p(pose, D),
                                         _p(res, D), _p(jac, D))
    return bool(ok), res, jac


def restated_match(grid, opts, target, initial, cloud):
    """CeresScanMatcher2D::Match: (pose, iterations, failed candidate evaluations).
    opts: (occupied, translation, rotation, iterations[, nonmonotonic = True])."""
    args, keep = _grid_args(grid)
    pts = _cloud(cloud)
    o = np.asarray(tuple(opts[:4]) + ((1.0 if opts[4] else 0.0) if len(opts) > 4 else 1.0,),
                   np.float64)
    tgt = np.asarray(target, np.float64)
    init = np.asarray(initial, np.float64)
    out = np.zeros(3)
    failed = I32(0)
    iters = shim().shim_ceres_tsdf_match(*args, _p(o, D), _p(tgt, D), _p(init, D), _p(pts, F),
                                         len(pts), _p(out, D), C.byref(failed))
    return tuple(out.tolist()), int(iters), int(failed.value)


def make_options(csm, opts):
    return csm.CeresOptions2D.make(*opts)


# ---- fixtures ----------------------------------------------------------------

# tsdf_match_cost_function_2d_test.cc:36-55.
REF_LIMITS = (0.1, 2.05, 2.05, 40, 40)
REF_TRUNCATION, REF_MAX_WEIGHT = 0.3, 1.0
REF_INSERTER = (0.3, 1.0, 0, 2, 10.0, 1, 0, 0.0, 0.0)
REF_CLOUD = np.array([[0.0, 1.0, 0.0]], np.float32)
# (pose, valid, residual, jacobian) of the file's four tests, all to its 1e-3.
REF_CASES = [((0.0, 0.0, 0.0), True, 0.0, (0.0, -1.0, 0.0)),
             ((0.0, 0.1, 0.0), True, -0.1, (0.0, -1.0, 0.0)),
             ((0.0, -0.1, 0.0), True, 0.1, (0.0, -1.0, 0.0)),
             ((0.0, 0.4, 0.0), False, None, None),
             ((0.0, -0.4, 0.0), False, None, None)]


# Configurations in which candidate evaluations fail, pinned by
# test_ceres_tsdf_host.py: (options, cloud, failed candidate evaluations), start
# and target (0, 0, 0) on the room TSDF. A point at the outer edge of the
# weighted band of the wall at x = 4 m (the weights end at 4.35 m), a large
# occupied-space weight and a small translation weight: LM steps push the point
# off the band, where the summed weight is 0.
CANDIDATE_FAILURES = [((200.0, 1.0, 1.0, 10, False), [[4.3, -0.6, 0.0]], 3),
                      ((1000.0, 1.0, 1.0, 20, True), [[4.3, -0.6, 0.0]], 5)]


def _to_tsdf(csm, ora, truncation, max_weight):
    (res, max_x, max_y), tsd, wgt = ora.get()
    return csm.TSDF2D(res, max_x, max_y, tsd, wgt, truncation, max_weight)


def reference_fixture(csm, empty=False):
    """The reference test's TSDF (InsertPointcloud, :57-66; `empty`: before it)."""
    ora = ts.OracleTSDF(Oracle(), REF_LIMITS, REF_TRUNCATION, REF_MAX_WEIGHT)
    if not empty:
        returns = []
        x = np.float32(-0.5)
        while x < np.float32(0.5):  # for (float x = -.5; x < 0.5f; x += 0.1)
            returns.append((x, 1.0, 0.0))
            x = np.float32(np.float64(x) + 0.1)
        ora.insert((np.array([-0.5, -0.5, 0.0], np.float32), np.asarray(returns, np.float32)),
                   REF_INSERTER)
    return _to_tsdf(csm, ora, REF_TRUNCATION, REF_MAX_WEIGHT)


@functools.lru_cache(maxsize=None)
def _room_oracle():
    ora = ts.OracleTSDF(Oracle())
    for scan in ts.room():
        ora.insert(scan, ts.OPTION_SETS["A"])
    return ora


def room_tsdf(csm):
    """tsdf_support.room() inserted with option set A by the oracle: 200 x 200."""
    return _to_tsdf(csm, _room_oracle(), ts.TRUNCATION, ts.MAX_WEIGHT)


def room_cloud(scan_index, n):
    """Scan `scan_index` of room() in its sensor frame, decimated to n points."""
    origin, pts = ts.room()[scan_index]
    keep = np.linspace(0, len(pts) - 1, n).round().astype(np.int64)
    cloud = pts[keep] - origin
    cloud[:, 2] = 0.0
    return np.ascontiguousarray(cloud, np.float32), tuple(float(v) for v in origin[:2]) + (0.0,)


# ---- PrecomputationGridStack2D in numpy ----------------------------------------

def quantized_level0(cells, min_cc, max_cc):
    """PrecomputationGrid2D's cell values at width 1
    (fast_correlative_scan_matcher_2d.cc:97-98, :151-160): the uint8 of
    1 - correspondence cost over [1 - max, 1 - min], per uint16 cell."""
    f32 = np.float32
    min_cc, max_cc = f32(min_cc), f32(max_cc)
    lo, hi = f32(1.0) - max_cc, f32(1.0) - min_cc
    # ValueConversionTables (value_conversion_tables.cc:26-60) in float:
    # value * scale + (lower - scale), unknown (0) -> max.
    scale = (max_cc - min_cc) / f32(32766.0)
    cost = np.arange(32768, dtype=np.float32) * scale + (min_cc - scale)
    cost[0] = max_cc
    s = f32(1.0) - np.abs(cost)
    x = ((s - lo) * (f32(255.0) / (hi - lo))).astype(np.float64)
    q = np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))  # lround: halves away from zero
    assert q.min() >= 0 and q.max() <= 255
    return q.astype(np.uint8)[np.asarray(cells, np.int64) & 0x7fff]


def sliding_max_level(level0, width):
    """Level with cell width `width`: the widened (ny + w - 1, nx + w - 1) grid
    of maxima over the w x w window ending at each cell (:105-160)."""
    ny, nx = level0.shape
    w = width
    padded = np.zeros((ny + 2 * (w - 1), nx + 2 * (w - 1)), np.uint8)
    padded[w - 1:w - 1 + ny, w - 1:w - 1 + nx] = level0
    out = np.zeros((ny + w - 1, nx + w - 1), np.uint8)
    for dy in range(w):
        for dx in range(w):
            np.maximum(out, padded[dy:dy + ny + w - 1, dx:dx + nx + w - 1], out=out)
    return out


# ---- brute-force FastCorrelativeScanMatcher2D ----------------------------------

def sum_to_score(total, n, min_cc, max_cc):
    """PrecomputationGrid2D::ToScore of the mean cell value
    (fast_correlative_scan_matcher_2d.cc:357-365, .h:81-84) in float."""
    f32 = np.float32
    min_s, max_s = f32(1.0) - f32(max_cc), f32(1.0) - f32(min_cc)
    mean = f32(int(total)) / f32(n)
    return f32(min_s + mean * ((max_s - min_s) / f32(255.0)))


def brute_force_match(oracle, limits, cells, min_cc, max_cc, initial, lin, ang, cloud):
    """Every level-0 candidate of Match(initial, cloud) scored from the cells:
    the oracle's SearchParameters, rotated scans, DiscretizeScans and
    ShrinkToFit (oracle.discretize), sums of the quantised level-0 values in
    numpy. Returns (score float32, pose, number of candidates at the maximum)."""
    res = limits[0]
    level0 = quantized_level0(cells, min_cc, max_cc).astype(np.int32)
    ny, nx = level0.shape
    num_scans, bounds, discrete, step = oracle.discretize(limits, np.asarray(cells), initial, lin,
                                                          ang, cloud)
    num_angular = (num_scans - 1) // 2
    n = discrete.shape[1]
    best, best_at, ties = -1, None, 0
    for s in range(num_scans):
        min_x, max_x, min_y, max_y = (int(v) for v in bounds[s])
        if max_x < min_x or max_y < min_y:
            continue
        w, h = max_x - min_x + 1, max_y - min_y + 1
        total = np.zeros((h, w), np.int32)
        for px, py in discrete[s]:
            # Cells (px + x_off, py + y_off) over the offsets, 0 outside the grid.
            x0, y0 = int(px) + min_x, int(py) + min_y
            ax0, ay0 = max(x0, 0), max(y0, 0)
            ax1, ay1 = min(x0 + w, nx), min(y0 + h, ny)
            if ax1 > ax0 and ay1 > ay0:
                total[ay0 - y0:ay1 - y0, ax0 - x0:ax1 - x0] += level0[ay0:ay1, ax0:ax1]
        m = int(total.max())
        if m > best:
            iy, ix = np.unravel_index(int(total.argmax()), total.shape)
            best, best_at, ties = m, (s, min_x + int(ix), min_y + int(iy)), int((total == m).sum())
        elif m == best:
            ties += int((total == m).sum())
    s, x_off, y_off = best_at
    pose = (initial[0] + (-y_off * res), initial[1] + (-x_off * res),
            initial[2] + (s - num_angular) * step)
    return sum_to_score(best, n, min_cc, max_cc), pose, ties


def full_submap_centre(limits):
    """MatchFullSubmap's initial pose (fast_correlative_scan_matcher_2d.cc:217-221)."""
    res, max_x, max_y, nx, ny = limits
    return (max_x - 0.5 * res * ny, max_y - 0.5 * res * nx, 0.0)


def room_near_cloud(scan_index, max_range, n):
    """The returns of room() scan `scan_index` within max_range of the sensor,
    in its frame, decimated to n points: a short range keeps MatchFullSubmap's
    angular step, and with it the brute force, small."""
    origin, pts = ts.room()[scan_index]
    near = pts[np.hypot(pts[:, 0] - origin[0], pts[:, 1] - origin[1]) < max_range] - origin
    keep = np.linspace(0, len(near) - 1, n).round().astype(np.int64)
    cloud = np.ascontiguousarray(near[keep], np.float32)
    cloud[:, 2] = 0.0
    return cloud
