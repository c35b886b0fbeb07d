"""An independent restatement of the two occupied-space costs, and the
fixtures of the row tests (test_ceres_rows_host.py, test_ceres_rows_gpu.py).

Plain numpy in np.longdouble (80-bit here, eps 1.08e-19). Written from the
definitions, not from the kernels or the oracle: Ceres' CubicHermiteSpline /
BiCubicInterpolator (cubic_interpolation.h) under
OccupiedSpaceCostFunction2D's GridArrayAdapter
(occupied_space_cost_function_2d.cc:39-96), and InterpolatedGrid
(interpolated_grid.h:51-140) under OccupiedSpaceCostFunction3D with Eigen's
quaternion rotation, plus the delta functors. Value functions only: there is
no analytic derivative in this module. Jacobians are central differences of
the value functions through the whole chain, in 3D in the tangent space of
ceres::QuaternionParameterization, q <- (cos|d|, sin|d|/|d| d) * q at d = 0.

Cell values come from the value table (probability_values.cc:29-37), which is
not the subject here.

The 2D coordinate. The reference adds kPadding = INT_MAX / 4 to the grid
coordinate in double, which quantises it to 2^-23 cells (error up to 2^-24 =
6e-8). The restatement reproduces that single rounding (the sum taken in
float64, everything after it in long double). Differences are taken with the
centre point's rounding offset held fixed, so that they differentiate the
smooth function at the coordinate the reference evaluates, not the staircase
the rounding makes of it.

The 3D float steps (CenterOfLowerVoxel, GetCellIndex, GetCenterOfCell) stay
float32, one correctly rounded np.float32 operation each, with lround's
half-away-from-zero."""
import math

import numpy as np

LD = np.longdouble
F32 = np.float32
K_PADDING = (2 ** 31 - 1) // 4

# Difference steps (pose units). Long double leaves room for small steps:
# truncation h^2 f'''/6 against rounding eps |f| / h with eps = 1.08e-19.
H_2D = LD(1e-7)
H_3D = LD(1e-7)

# ---- measured deviations and the bounds derived from them ------------------
# Largest deviation of the oracle's rows (oracle/ceres2d.cc Evaluate,
# oracle/ceres3d.cc Evaluate3) from this restatement over every random fixture
# below, and the bound: 4 x the measured figure, the margin for libm and
# summation differences between machines. Jacobian figures are relative to the
# largest |entry| of the case's Jacobian. DESIGN.md §8c repeats them.
MEASURED_VALUE_2D = 4.4e-15
BOUND_VALUE_2D = 4 * MEASURED_VALUE_2D
MEASURED_JACOBIAN_REL_2D = 2.2e-11
BOUND_JACOBIAN_REL_2D = 4 * MEASURED_JACOBIAN_REL_2D
MEASURED_VALUE_3D = 3.6e-15
BOUND_VALUE_3D = 4 * MEASURED_VALUE_3D
MEASURED_JACOBIAN_REL_3D = 3.0e-12
BOUND_JACOBIAN_REL_3D = 4 * MEASURED_JACOBIAN_REL_3D


def value_table(unknown_result, lower, upper):
    """PrecomputeValueToBoundedFloat's first half in float32: value 0 is
    unknown, else value * scale + (lower - scale)."""
    lower, upper = F32(lower), F32(upper)
    scale = (upper - lower) / F32(32766.0)
    v = np.arange(32768, dtype=F32)
    t = v * scale + (lower - scale)
    t[0] = F32(unknown_result)
    return t.astype(F32)


K_MIN_PROBABILITY = F32(0.1)
K_MAX_PROBABILITY = F32(1.0) - K_MIN_PROBABILITY
K_MIN_CC = F32(1.0) - K_MAX_PROBABILITY
K_MAX_CC = F32(1.0) - K_MIN_PROBABILITY
COST_TABLE = value_table(K_MAX_CC, K_MIN_CC, K_MAX_CC)
PROBABILITY_TABLE = value_table(K_MIN_PROBABILITY, K_MIN_PROBABILITY, K_MAX_PROBABILITY)


# ============================================================== 2D ==========
class Grid2D:
    """MapLimits and the uint16 cells, cells[y, x] of shape (num_y_cells,
    num_x_cells)."""

    def __init__(self, resolution, max_x, max_y, cells):
        self.resolution, self.max_x, self.max_y = float(resolution), float(max_x), float(max_y)
        self.cells = np.ascontiguousarray(cells, np.uint16)
        self.ny, self.nx = self.cells.shape
        # GridArrayAdapter::GetValue over a margin of kMaxCorrespondenceCost:
        # row < num_y_cells, column < num_x_cells read cell (x = column, y = row).
        self._pad = 4
        padded = np.full((self.ny + 2 * self._pad, self.nx + 2 * self._pad), LD(K_MAX_CC), LD)
        padded[self._pad:-self._pad, self._pad:-self._pad] = \
            COST_TABLE[self.cells & 0x7fff].astype(LD)
        self._padded = padded

    @property
    def limits(self):
        return (self.resolution, self.max_x, self.max_y)

    def value(self, row, col):
        r = np.clip(row + self._pad, 0, self._padded.shape[0] - 1)
        c = np.clip(col + self._pad, 0, self._padded.shape[1] - 1)
        return self._padded[r, c]


def _hermite(p0, p1, p2, p3, x):
    """ceres::CubicHermiteSpline, value only."""
    half = LD(0.5)
    a = half * (-p0 + LD(3) * p1 - LD(3) * p2 + p3)
    b = half * (LD(2) * p0 - LD(5) * p1 + LD(4) * p2 - p3)
    c = half * (-p0 + p2)
    return p1 + x * (c + x * (b + x * a))


def _bicubic(grid, r, c):
    """ceres::BiCubicInterpolator::Evaluate, value only, at grid coordinates
    (r, c) without the padding."""
    row = np.floor(r).astype(np.int64)
    col = np.floor(c).astype(np.int64)
    fr, fc = r - row, c - col
    along = [_hermite(grid.value(row - 1 + k, col - 1), grid.value(row - 1 + k, col),
                      grid.value(row - 1 + k, col + 1), grid.value(row - 1 + k, col + 2), fc)
             for k in range(4)]
    return _hermite(along[0], along[1], along[2], along[3], fr)


def _coords2d(grid, cloud, pose):
    """Pose -> world point -> grid coordinate (row from x, column from y), in
    long double and without the padding."""
    x, y, theta = (LD(v) for v in pose)
    s, c = np.sin(theta), np.cos(theta)
    px, py = cloud[:, 0].astype(LD), cloud[:, 1].astype(LD)
    wx = c * px - s * py + x
    wy = s * px + c * py + y
    res = LD(grid.resolution)
    return (LD(grid.max_x) - wx) / res - LD(0.5), (LD(grid.max_y) - wy) / res - LD(0.5)


def padding_offsets(grid, cloud, pose):
    """What the float64 sum with kPadding does to each coordinate."""
    out = []
    for u in _coords2d(grid, cloud, pose):
        rounded = u.astype(np.float64) + np.float64(K_PADDING)
        out.append((rounded.astype(LD) - LD(K_PADDING)) - u)
    return out


def residuals2d(grid, cloud, weights, target, pose, offsets=None):
    """The n + 3 residuals of CeresScanMatcher2D's problem at `pose`, long
    double. weights: (occupied, translation, rotation); target: (x, y, theta).
    offsets: coordinate shifts (padding_offsets), default those of `pose`."""
    cloud = np.asarray(cloud, F32).reshape(-1, 3)
    if offsets is None:
        offsets = padding_offsets(grid, cloud, pose)
    u, v = _coords2d(grid, cloud, pose)
    scale = LD(weights[0]) / np.sqrt(LD(len(cloud)))
    occupied = scale * _bicubic(grid, u + offsets[0], v + offsets[1])
    delta = [LD(weights[1]) * (LD(pose[0]) - LD(target[0])),
             LD(weights[1]) * (LD(pose[1]) - LD(target[1])),
             LD(weights[2]) * (LD(pose[2]) - LD(target[2]))]
    return np.concatenate([occupied, np.array(delta, LD)])


def jacobian2d(grid, cloud, weights, target, pose, h=H_2D):
    """(n + 3) x 3 central differences of residuals2d."""
    cloud = np.asarray(cloud, F32).reshape(-1, 3)
    offsets = padding_offsets(grid, cloud, pose)
    cols = []
    for k in range(3):
        hi = [LD(v) for v in pose]
        lo = [LD(v) for v in pose]
        hi[k] += h
        lo[k] -= h
        cols.append((residuals2d(grid, cloud, weights, target, hi, offsets) -
                     residuals2d(grid, cloud, weights, target, lo, offsets)) / (LD(2) * h))
    return np.stack(cols, 1)


# ---- 2D fixtures -----------------------------------------------------------
WEIGHTS_2D = (20.0, 10.0, 1.0)
THETAS_2D = (0.0, 0.3, -2.8, 3.5)
SIZES_2D = (1, 2, 253, 254, 255, 256, 257, 515)
RESOLUTION_2D = 0.05
# (num_x_cells, num_y_cells, max_x, max_y): the maxima are dyadic, so that the
# deliberate points below are exact, and no multiples of the resolution.
_GRIDS_2D = ((24, 40, 1.0 + 13.0 / 1024.0, 785.0 / 1024.0),
             (40, 24, 705.0 / 1024.0, 1349.0 / 1024.0))


def grids2d():
    out = []
    for g, (nx, ny, max_x, max_y) in enumerate(_GRIDS_2D):
        rng = np.random.default_rng(100 + g)
        cells = rng.integers(1, 32768, (ny, nx)).astype(np.uint16)
        cells[rng.random((ny, nx)) < 0.10] = 0  # unknown
        out.append(Grid2D(RESOLUTION_2D, max_x, max_y, cells))
    return out


def _pose2d(g, k):
    return (0.31 - 0.07 * k + 0.02 * g, -0.17 + 0.05 * k, THETAS_2D[k])


def _target2d(pose):
    return (pose[0] + 0.013, pose[1] - 0.021, pose[2] + 0.017)


def cloud2d(grid, pose, n, seed):
    """n points whose world positions are uniform over the grid plus three
    cells beyond every side; clouds of 253 points and more also hold two far
    outside (constant residual, zero row)."""
    rng = np.random.default_rng(seed)
    res = grid.resolution
    # Rows run along world x over num_y_cells, columns along y over num_x_cells.
    wx = grid.max_x - rng.uniform(-3.0, grid.ny + 3.0, n) * res
    wy = grid.max_y - rng.uniform(-3.0, grid.nx + 3.0, n) * res
    if n >= 253:
        wx[5], wy[5] = grid.max_x + 40.0, grid.max_y - 55.0
        wx[n - 1], wy[n - 1] = grid.max_x - 70.0, grid.max_y + 3.0
    c, s = math.cos(pose[2]), math.sin(pose[2])
    dx, dy = wx - pose[0], wy - pose[1]
    cloud = np.zeros((n, 3), F32)
    cloud[:, 0] = c * dx + s * dy
    cloud[:, 1] = -s * dx + c * dy
    return cloud


def cases2d():
    """The random fixtures: (name, grid index, cloud, pose, target), every
    grid, angle and size."""
    out = []
    for g, grid in enumerate(grids2d()):
        for k in range(len(THETAS_2D)):
            pose = _pose2d(g, k)
            for n in SIZES_2D:
                cloud = cloud2d(grid, pose, n, 1000 * g + 100 * k + n)
                out.append((f"grid{g}-theta{THETAS_2D[k]}-n{n}", g, cloud, pose, _target2d(pose)))
    return out


def taps_reach_the_long_side(grid, cloud, pose):
    """True when some point's taps lie at rows >= num_x_cells (a grid longer
    in y) or at columns >= num_y_cells (longer in x), inside the grid: what a
    rows/columns mix-up in the bounds or the index would get wrong."""
    u, v = _coords2d(grid, np.asarray(cloud, F32), pose)
    row, col = np.floor(u), np.floor(v)
    if grid.ny > grid.nx:
        return bool(np.any((row - 1 >= grid.nx) & (row + 2 < grid.ny) & (col >= 1) &
                           (col + 2 < grid.nx)))
    return bool(np.any((col - 1 >= grid.ny) & (col + 2 < grid.nx) & (row >= 1) &
                       (row + 2 < grid.ny)))


def exact_case2d(g, grid):
    """Points exactly on cell centres and on cell boundaries, at theta = 0.
    With dyadic maxima, pose and points, max - (p + pose) = j / 8 is exact, and
    j / 8 / 0.05 - 0.5 is 2.5 j - 0.5: a centre for odd j, a boundary for even
    j, where the double division is exact, which is checked here and not
    assumed. Returns (name, grid index, cloud, pose, target, on_centre mask)."""
    pose = (0.3125, -0.1875, 0.0)
    half_cols = (int(grid.nx * 0.4) + 2) // 2
    pts, centre = [], []
    # Each row position with a column of its own parity and one of the other.
    pairs = [(jr, (jr + flip) % 2 + 2 * ((3 * jr + flip) % half_cols))
             for jr in range(0, int(grid.ny * 0.4) + 2) for flip in (0, 1)]
    for jr, jc in pairs:
        px = grid.max_x - jr / 8.0 - pose[0]
        py = grid.max_y - jc / 8.0 - pose[1]
        assert float(F32(px)) == px and float(F32(py)) == py
        # The reference's arithmetic at theta = 0: cos = 1, sin = 0.
        u = (grid.max_x - (1.0 * px + (-0.0 * py + pose[0] * 1.0))) / grid.resolution - 0.5
        v = (grid.max_y - (0.0 * px + (1.0 * py + pose[1] * 1.0))) / grid.resolution - 0.5
        if u != 2.5 * jr - 0.5 or v != 2.5 * jc - 0.5:
            continue  # the division rounded: not an exact point
        pts.append((px, py, 0.0))
        centre.append(jr % 2 == 1 and jc % 2 == 1)
    centre = np.array(centre)
    assert centre.sum() >= 3 and (~centre).sum() >= 3, "too few exact points"
    return (f"grid{g}-exact", g, np.array(pts, F32), pose, _target2d(pose), centre)


# ============================================================== 3D ==========
class Grid3D:
    """A HybridGrid's known cells: indices (n, 3) and uint16 values; every
    other cell is unknown (kMinProbability)."""

    def __init__(self, resolution, indices, values):
        self.resolution = F32(resolution)
        self.indices = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
        self.values = np.ascontiguousarray(values, np.uint16)
        self._pad = 2
        self._lo = self.indices.min(0).astype(np.int64) - self._pad
        shape = self.indices.max(0).astype(np.int64) - self._lo + 1 + self._pad
        dense = np.full(tuple(shape), LD(K_MIN_PROBABILITY), LD)
        at = self.indices.astype(np.int64) - self._lo
        dense[at[:, 0], at[:, 1], at[:, 2]] = PROBABILITY_TABLE[self.values & 0x7fff].astype(LD)
        self._dense = dense

    def probability(self, ix, iy, iz):
        """HybridGrid::GetProbability."""
        at = [np.clip(i - self._lo[a], 0, self._dense.shape[a] - 1)
              for a, i in enumerate((ix, iy, iz))]
        return self._dense[at[0], at[1], at[2]]


def _lround(v):
    """std::lround of float32 values: half away from zero."""
    v = v.astype(np.float64)  # exact
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def _cell_index(coordinate_f32, res):
    """HybridGrid::GetCellIndex per axis: lround(float / float)."""
    return _lround((coordinate_f32 / res).astype(F32))


def _interpolate(grid, w):
    """InterpolatedGrid::GetInterpolatedValue at world points w (n, 3), long
    double, value only."""
    res = grid.resolution
    lower_index, t = [], []
    for a in range(3):
        x = w[:, a]
        xf = x.astype(np.float64).astype(F32)  # Eigen::Vector3f(x, y, z) of doubles
        # GetCenterOfCell(GetCellIndex(.)): index.cast<float>() * resolution.
        centre = (_cell_index(xf, res).astype(F32) * res).astype(F32)
        centre = np.where(centre.astype(LD) > x, (centre - res).astype(F32), centre).astype(F32)
        x1 = centre.astype(LD)
        x2 = (centre + res).astype(F32).astype(LD)  # lower + resolution, in float
        lower_index.append(_cell_index(centre, res))
        t.append((x - x1) / (x2 - x1))
    ix, iy, iz = lower_index

    def q(dx, dy, dz):
        return grid.probability(ix + dx, iy + dy, iz + dz)

    def step(a, b, n):
        return (a - b) * (n * (n * n)) * LD(2) + (b - a) * (n * n) * LD(3) + a

    nx, ny, nz = t
    q11, q12 = step(q(0, 0, 0), q(0, 0, 1), nz), step(q(0, 1, 0), q(0, 1, 1), nz)
    q21, q22 = step(q(1, 0, 0), q(1, 0, 1), nz), step(q(1, 1, 0), q(1, 1, 1), nz)
    return step(step(q11, q12, ny), step(q21, q22, ny), nx)


def _quat_product(a, b):
    """common::QuaternionProduct / ceres::QuaternionProduct, (w, x, y, z)."""
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def _rotate(q, v):
    """Eigen's Quaternion * vector: v + w uv + qv x uv with uv = 2 qv x v."""
    qv = np.array(q[1:4], LD)
    uv = LD(2) * np.cross(qv[None, :], v)
    return v + q[0] * uv + np.cross(qv[None, :], uv)


def residuals3d(grids, clouds, weights, target, t, q):
    """The n0 + n1 + 6 residuals of CeresScanMatcher3D's problem at (t, q),
    long double. grids / clouds: (high, low); weights: (w0, w1, translation,
    rotation); target: ((t), (w, x, y, z))."""
    t = [LD(v) for v in t]
    q = [LD(v) for v in q]
    out = []
    for k in range(2):
        cloud = np.asarray(clouds[k], F32).reshape(-1, 3)
        w = _rotate(q, cloud.astype(LD)) + np.array(t, LD)[None, :]
        scale = LD(weights[k]) / np.sqrt(LD(len(cloud)))
        out.append(scale * (LD(1) - _interpolate(grids[k], w)))
    out.append(np.array([LD(weights[2]) * (t[a] - LD(target[0][a])) for a in range(3)], LD))
    tq = [LD(v) for v in target[1]]
    delta = _quat_product([tq[0], -tq[1], -tq[2], -tq[3]], q)
    out.append(np.array([LD(weights[3]) * delta[a] for a in (1, 2, 3)], LD))
    return np.concatenate(out)


def jacobian3d(grids, clouds, weights, target, t, q, h=H_3D):
    """N x 6 central differences of residuals3d in the tangent space:
    translation, then q <- (cos h, sin h e_k) * q."""
    cols = []
    for k in range(3):
        hi = [LD(v) for v in t]
        lo = [LD(v) for v in t]
        hi[k] += h
        lo[k] -= h
        cols.append((residuals3d(grids, clouds, weights, target, hi, q) -
                     residuals3d(grids, clouds, weights, target, lo, q)) / (LD(2) * h))
    ql = [LD(v) for v in q]
    for k in range(3):
        dq = [np.cos(h), LD(0), LD(0), LD(0)]
        dq[1 + k] = np.sin(h)
        hi = _quat_product(dq, ql)
        dq[1 + k] = -dq[1 + k]
        lo = _quat_product(dq, ql)
        cols.append((residuals3d(grids, clouds, weights, target, t, hi) -
                     residuals3d(grids, clouds, weights, target, t, lo)) / (LD(2) * h))
    return np.stack(cols, 1)


# ---- 3D fixtures -----------------------------------------------------------
WEIGHTS_3D = (5.0, 30.0, 10.0, 1.0)
# Index boxes [lo, hi] per axis, neither cubic nor one-signed.
_BOX_HIGH = ((-5, 6), (-3, 4), (-2, 3))  # 12 x 8 x 6 cells at 0.1
_BOX_LOW = ((-4, 3), (-3, 2), (-2, 2))   # 8 x 6 x 5 cells at 0.45
RESOLUTIONS_3D = (0.1, 0.45)
COUNTS_3D = tuple((249 + k - 119, 119) for k in range(9)) + ((1, 1), (300, 215))


def _grid3d(resolution, box, seed):
    rng = np.random.default_rng(seed)
    axes = [np.arange(lo, hi + 1) for lo, hi in box]
    ijk = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    keep = rng.random(len(ijk)) >= 0.20  # about 20% of the cells absent
    # The box's corners stay, so that the brick is the whole box.
    corner = np.all((ijk == np.array([b[0] for b in box])) |
                    (ijk == np.array([b[1] for b in box])), 1)
    keep |= corner
    values = rng.integers(1, 32768, len(ijk)).astype(np.uint16)
    return Grid3D(resolution, ijk[keep].astype(np.int32), values[keep])


def grids3d():
    return (_grid3d(RESOLUTIONS_3D[0], _BOX_HIGH, 300), _grid3d(RESOLUTIONS_3D[1], _BOX_LOW, 301))


def _unit(q):
    q = np.asarray(q, np.float64)
    return tuple(float(v) for v in q / np.sqrt((q * q).sum()))


def poses3d():
    """(t, q): identity, two general rotations with four non-zero components,
    one within 0.05 rad of a half turn, one with w < 0."""
    half = math.pi - 0.03
    axis = np.array([0.48, -0.6, 0.64])
    axis /= np.sqrt((axis * axis).sum())
    near_half_turn = (math.cos(half / 2),) + tuple(math.sin(half / 2) * axis)
    return [((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)),
            ((0.04, -0.03, 0.02), _unit((0.9, 0.2, -0.3, 0.25))),
            ((-0.11, 0.07, 0.05), _unit((0.5, -0.6, 0.4, 0.48))),
            ((0.02, 0.03, -0.04), _unit(near_half_turn)),
            ((-0.05, 0.02, 0.03), _unit((-0.8, 0.3, 0.35, -0.38)))]


def _target3d(pose):
    """A target translation and rotation that both differ from the pose."""
    t, q = pose
    a = 0.021
    dq = (math.cos(a), math.sin(a) * 0.6, -math.sin(a) * 0.48, math.sin(a) * 0.64)
    tq = _quat_product(dq, q)
    return ((t[0] + 0.012, t[1] - 0.02, t[2] + 0.007), _unit(tq))


def _cloud3d(resolution, box, pose, n, rng):
    """n points whose world positions cover the box and 1.5 cells beyond each
    face; from 12 points on, one within a cell of each face on either side
    (alternating) and, from 14 on, two far outside."""
    lo = np.array([b[0] - 0.5 for b in box]) * resolution  # faces of the box
    hi = np.array([b[1] + 0.5 for b in box]) * resolution
    w = rng.uniform(lo - 1.5 * resolution, hi + 1.5 * resolution, (n, 3))
    if n >= 12:
        for f in range(12):
            a, side = f // 4, f % 4
            face = (lo, hi)[side // 2][a]
            w[f, a] = face + (0.45 if side % 2 else -0.45) * resolution
    if n >= 14:
        w[12] = hi + 60.0 * resolution
        w[13] = lo - np.array([7.0, 45.0, 90.0])
    t, q = pose
    inverse = [LD(q[0]), -LD(q[1]), -LD(q[2]), -LD(q[3])]
    return _rotate(inverse, (w - np.array(t))[:, :].astype(LD)).astype(F32)


def cases3d():
    """The random fixtures: (name, high cloud, low cloud, pose, target), every
    pose and pair of counts."""
    out = []
    for p, pose in enumerate(poses3d()):
        for n0, n1 in COUNTS_3D:
            rng = np.random.default_rng(7000 + 1000 * p + n0 + n1)
            high = _cloud3d(RESOLUTIONS_3D[0], _BOX_HIGH, pose, n0, rng)
            low = _cloud3d(RESOLUTIONS_3D[1], _BOX_LOW, pose, n1, rng)
            out.append((f"pose{p}-n{n0}+{n1}", high, low, pose, _target3d(pose)))
    return out


def _exact_cloud3d(resolution, box):
    """Points exactly on voxel centres (float(k) * resolution, as
    GetCenterOfCell gives them) and on half-cell positions (where the float
    quotient is exactly k + 0.5), negative ones included."""
    res = F32(resolution)
    pts = []
    ks = [range(b[0] - 1, b[1] + 2) for b in box]
    for a, kx in enumerate(ks[0]):
        ky = ks[1][(2 * a + 1) % len(ks[1])]
        kz = ks[2][(3 * a + 2) % len(ks[2])]
        centre = [F32(k) * res for k in (kx, ky, kz)]
        pts.append(centre)
        half = []
        for k in (kx, ky, kz):
            v = F32((k + 0.5) * float(res))
            cands = [c for c in (v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf)))
                     if float(F32(c / res)) == k + 0.5]
            half.append(cands[0] if cands else F32(k) * res)
        pts.append(half)
        pts.append([centre[0], half[1], centre[2]])
    return np.array(pts, F32)


def exact_case3d():
    """(name, high cloud, low cloud, pose, target) at the identity pose, where
    the world point is the cloud point exactly."""
    pose = poses3d()[0]
    return ("exact", _exact_cloud3d(RESOLUTIONS_3D[0], _BOX_HIGH),
            _exact_cloud3d(RESOLUTIONS_3D[1], _BOX_LOW), pose, _target3d(pose))


# ---- comparisons -----------------------------------------------------------
def deviation(got, want):
    """Largest |got - want|, the difference taken in long double."""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - np.asarray(want).astype(LD))))


def packed_sums(r, jac):
    """What Pass / Pass3 reduce, from rows, in float64: sum r^2, the upper
    triangle of J^T J by rows, J^T r; and per entry the sum of the |terms|."""
    r = np.asarray(r, np.float64)
    jac = np.asarray(jac, np.float64)
    terms = [r * r]
    k = jac.shape[1]
    for a in range(k):
        for b in range(a, k):
            terms.append(jac[:, a] * jac[:, b])
    for a in range(k):
        terms.append(jac[:, a] * r)
    terms = np.array(terms)
    return terms.sum(1), np.abs(terms).sum(1)
