"""GPU: the octet bricks fast3d_search loads and the levels above
branch_and_bound_depth it roots at, read back and compared byte for byte
with a reference made from the oracle's levels (planes_support.py). Each
HybridGrid is read through a single create and through
csm_fast3d_create_batch (whose row kernels stage source rows in LDS as
dwords, with reads that start before the row and alignment masking); the two
must equal each other and the reference. Every comparison is equality on
integers."""
import numpy as np
import pytest

import planes_support as ps

pytestmark = pytest.mark.gpu

K_MAX_LEVELS_3D = 12
K_EXTRA_LEVELS_3D = 2
RESOLUTION = 0.1

# (origin, dims): rows of 1, 2, 3, 5 and 7 cells start at every byte alignment
# and the octet rows start H cells before them; negative and odd origins (the
# half-resolution boxes shift negative numbers right); rows of more than one
# 128-dword staging pass; one known cell.
SMALL_BRICKS = [
    ((0, 0, 0), (1, 2, 3)),
    ((3, -2, 1), (2, 3, 2)),
    ((-1, 5, -4), (3, 2, 2)),
    ((10, 1, 1), (5, 3, 2)),
    ((-13, -1, 2), (7, 2, 3)),
    ((-7, -5, -3), (6, 5, 4)),
    ((-301, 3, -1), (600, 3, 2)),
    ((5, -9, 7), (1, 1, 1)),
]
EMPTY = (np.zeros((0, 3), np.int32), np.zeros(0, np.uint16))


def options(csm, depth, full_depth):
    return csm.FastCorrelativeScanMatcherOptions3D(depth, full_depth, 0.1, 0.15, 0.8, 0.8, 0.3)


def opt_tuple(o, depth=None):
    return (depth or o.branch_and_bound_depth, o.full_resolution_depth, o.min_rotational_score,
            o.min_low_resolution_score, o.linear_xy_search_window, o.linear_z_search_window,
            o.angular_search_window)


def sorted_cells(ijk, v):
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))
    return ijk[order], v[order]


def build(csm, cell_lists, o):
    """The grids, one matcher each from single creates and the same from one
    csm_fast3d_create_batch."""
    grids = csm.HybridGrid.create_batch(RESOLUTION, cell_lists)
    hist = np.zeros(10, np.float32)
    single = [csm.FastCorrelativeScanMatcher3D(g, g, hist, o) for g in grids]
    batch = csm.FastCorrelativeScanMatcher3D.create_batch([(g, g) for g in grids],
                                                          [hist] * len(grids), o)
    return grids, single, batch


def close_all(grids, single, batch):
    for m in single + batch:
        m.close()
    for g in grids:
        g.close()


def check_matcher(csm, oracle, cells, o, single, batch, tag):
    """Levels 0..search_levels-1 and octets 0..search_levels-2 of the two
    matchers against the oracle; returns the octet levels checked."""
    bbd, frd = o.branch_and_bound_depth, o.full_resolution_depth
    levels = min(bbd + K_EXTRA_LEVELS_3D, K_MAX_LEVELS_3D)
    for m in (single, batch):
        assert m.search_levels() == levels, tag
        with pytest.raises(csm.CsmError):
            m.read_level(levels)
        with pytest.raises(csm.CsmError):
            m.read_octets(levels - 1)
    ijk, values = cells
    if len(values) == 0:  # an empty grid: every read-back has zero dims
        for m in (single, batch):
            for level in range(levels):
                assert m.read_level(level)[1].shape == (0, 0, 0), (tag, level)
            for level in range(levels - 1):
                origin, octs, h = m.read_octets(level)
                assert octs.shape == (0, 0, 0) and h == ps.oct_h(level, frd), (tag, level)
        return 0
    og = oracle.hybrid_grid(RESOLUTION)
    og.set_values(ijk, values)
    hist = np.zeros(10, np.float32)
    shallow = oracle.fast3d(og, og, hist, opt_tuple(o))
    deep = oracle.fast3d(og, og, hist, opt_tuple(o, levels))
    boxes = []
    for level in range(levels):
        cells_l, v_l = sorted_cells(*deep.level(level))
        if level < bbd:  # the deeper stack's lower levels are the same recurrence
            cells_s, v_s = sorted_cells(*shallow.level(level))
            assert np.array_equal(cells_l, cells_s) and np.array_equal(v_l, v_s), (tag, level)
        origin, brick = single.read_level(level)
        origin_b, brick_b = batch.read_level(level)
        assert origin == origin_b and np.array_equal(brick, brick_b), (tag, level)
        assert np.count_nonzero(brick) == np.count_nonzero(v_l), (tag, level)
        dims = brick.shape[::-1]
        want = ps.dense_from_cells(cells_l, v_l, origin, dims)
        assert np.array_equal(brick, want), (tag, level)
        boxes.append((origin, dims, cells_l, v_l))
    for level in range(levels - 1):
        origin, dims, cells_l, v_l = boxes[level]
        h = ps.oct_h(level, frd)
        want_box = ps.octet_box(origin, dims, h)
        ref = ps.octet_reference(cells_l, v_l, origin, dims, h)
        for name, m in (("single", single), ("batch", batch)):
            o_origin, octs, o_h = m.read_octets(level)
            assert o_h == h, (tag, name, level)
            assert (o_origin, octs.shape[::-1]) == want_box, (tag, name, level)
            bad = np.argwhere(octs != ref)
            assert len(bad) == 0, (
                f"{tag} {name} level {level} H {h}: {len(bad)} octets differ, first (z, y, x) "
                f"{bad[0].tolist()}: device {int(octs[tuple(bad[0])]):016x} "
                f"reference {int(ref[tuple(bad[0])]):016x}")
    return levels - 1


@pytest.mark.parametrize("depth,full_depth", [(3, 3), (4, 2), (6, 3), (11, 3)])
def test_octets_and_extra_levels_match_oracle(csm, oracle, depth, full_depth):
    """One batch of unequal bricks, a one-cell grid and an empty grid (the
    batch launch's rows and LDS come from another job than most jobs' own).
    Depth 11 caps the extra levels at kMaxLevels3d."""
    o = options(csm, depth, full_depth)
    bricks = SMALL_BRICKS if depth < 11 else SMALL_BRICKS[3:6] + SMALL_BRICKS[7:]
    cell_lists = [ps.random_brick_cells(origin, dims, seed=20 + i)
                  for i, (origin, dims) in enumerate(bricks)] + [EMPTY]
    grids, single, batch = build(csm, cell_lists, o)
    try:
        checked = 0
        for i, cells in enumerate(cell_lists):
            dims = bricks[i][1] if i < len(bricks) else (0, 0, 0)
            checked += check_matcher(csm, oracle, cells, o, single[i], batch[i],
                                     f"grid {i} dims {dims}")
        assert checked == len(bricks) * (min(depth + K_EXTRA_LEVELS_3D, K_MAX_LEVELS_3D) - 1)
    finally:
        close_all(grids, single, batch)


def test_rows_past_the_lds_budget_fall_back_to_per_cell_kernels(csm, oracle):
    """A brick about 16 500 cells wide: its staged rows exceed 64 KiB, so the
    full-resolution levels and octets are built by the per-cell kernels
    inside a batch too, next to a small brick built by the row kernels."""
    o = options(csm, 3, 3)
    cell_lists = [ps.random_brick_cells((-8251, -1, 0), (16500, 2, 2), seed=40),
                  ps.random_brick_cells((2, 1, -3), (5, 3, 2), seed=41)]
    grids, single, batch = build(csm, cell_lists, o)
    try:
        for i, cells in enumerate(cell_lists):
            assert check_matcher(csm, oracle, cells, o, single[i], batch[i], f"grid {i}") == 4
    finally:
        close_all(grids, single, batch)
