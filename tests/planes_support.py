"""Plain numpy references of the layouts the branch-and-bound kernels load:
the 2D quad / hex planes (fast2d_search_v4 / v5) and the 3D octets
(fast3d_search). Everything is made from level 0 (2D) or from the oracle's
dense levels (3D) by brute force; nothing here calls the code under test.

2D conventions (SubmapDesc, csm_device.h): Q0 is the quantised level 0,
``q0[y, x]``, 0 outside. For level l, h = 2^l and km1 = 2^cshift[l] - 1. The
widened level M has size (nx + h - 1 + km1) x (ny + h - 1 + km1) and
M(mx, my) = max Q0 over x in [mx - (h - 1) - km1, mx], y likewise. A quad
entry (X', Y') packs M(X + a h, Y + b h), a, b in {0, 1}, X = X' - h, at byte
2a + b; a hex entry packs a, b in 0..3, X = X' - 3h, at byte 4a + b (dword a,
byte b). Storage is polyphase with period P = 2h (quad) or 4h (hex): entry
(X', Y') = (kx P + fx, ky P + fy) is at ((fy P + fx) pph + ky) pws + kx.
"""
import numpy as np

K_MAX_LEVELS = 12
K_MAX_CLUSTER_SHIFT = 3
DEFAULT_CLUSTER = (0, 0, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3)


# ---------------------------------------------------------------- 2D ------

def random_cells(ny, nx, seed):
    """uint16 cells in [0, 32768), about a third zero (unknown), non-zero on
    all four border rows and columns."""
    rng = np.random.RandomState(seed)
    cells = rng.randint(1, 32768, size=(ny, nx))
    cells[rng.random_sample((ny, nx)) < 1.0 / 3.0] = 0
    border = np.zeros((ny, nx), bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    fill = rng.randint(1, 32768, size=(ny, nx))
    cells[border & (cells == 0)] = fill[border & (cells == 0)]
    return cells.astype(np.uint16)


def auto_depth(configured, nx, ny):
    """The device's automatic search depth: coarser levels until the top
    lattice step reaches half of the grid."""
    d = configured
    while d < K_MAX_LEVELS and (1 << (d - 1)) < max(nx, ny) // 2:
        d += 1
    return d


def expected_depth(branch_and_bound_depth, search_depth, nx, ny):
    d = search_depth if search_depth > 0 else auto_depth(branch_and_bound_depth, nx, ny)
    return min(max(d, branch_and_bound_depth), K_MAX_LEVELS)


def expected_hex_mask(depth, env):
    """Node levels that expand two levels at once, from the variables a create
    reads (CSM_SEARCH_KERNEL, CSM_HEX_LEVELS)."""
    kernel = int(env.get("CSM_SEARCH_KERNEL", "0"))
    if kernel == 5:
        levels = set(range(2, depth, 2))
    elif kernel in (4, 2):
        levels = set()
    else:
        levels = {l for l in (depth - 1, depth - 3) if l >= 2}
    if "CSM_HEX_LEVELS" in env:
        levels = {int(t) for t in env["CSM_HEX_LEVELS"].split(",") if t}
        levels = {l for l in levels if 2 <= l < depth}
    return levels


def expected_kinds(depth, hex_levels):
    """Entry bytes per level by the node chain: the top level has a quad
    plane; a node level L in the hex set gives a hex plane at L - 2, any
    other a quad plane at L - 1."""
    kind = [0] * depth
    kind[depth - 1] = 4
    level = depth - 1
    while level >= 1:
        if level >= 2 and level in hex_levels:
            kind[level - 2] = 16
            level -= 2
        else:
            kind[level - 1] = 4
            level -= 1
    return kind


def expected_cshift(env):
    shifts = list(DEFAULT_CLUSTER)
    if "CSM_CLUSTER" in env:
        given = [int(t) for t in env["CSM_CLUSTER"].split(",")]
        shifts = [given[min(l, len(given) - 1)] for l in range(K_MAX_LEVELS)]
    return [max(0, min(s, l, K_MAX_CLUSTER_SHIFT)) for l, s in enumerate(shifts)]


def widened(q0, h, km1):
    """M (above) as a direct windowed maximum of width w = h + km1 over the
    zero-padded level 0, one axis after the other (the maximum over a box is
    the maximum over y of the maxima over x)."""
    ny, nx = q0.shape
    w = h + km1
    pad = np.zeros((ny + 2 * (w - 1), nx + 2 * (w - 1)), np.uint8)
    pad[w - 1:w - 1 + ny, w - 1:w - 1 + nx] = q0
    mw, mh = nx + w - 1, ny + w - 1
    rows = np.zeros((pad.shape[0], mw), np.uint8)
    for dx in range(w):  # q range [mx - (w - 1), mx] is pad range [mx, mx + w)
        np.maximum(rows, pad[:, dx:dx + mw], out=rows)
    out = np.zeros((mh, mw), np.uint8)
    for dy in range(w):
        np.maximum(out, rows[dy:dy + mh, :], out=out)
    return out


def widened_naive(q0, h, km1):
    """The same, cell by cell (tiny grids only)."""
    ny, nx = q0.shape
    w = h + km1
    out = np.zeros((ny + w - 1, nx + w - 1), np.uint8)
    for my in range(out.shape[0]):
        for mx in range(out.shape[1]):
            best = 0
            for y in range(my - (w - 1), my + 1):
                for x in range(mx - (w - 1), mx + 1):
                    if 0 <= x < nx and 0 <= y < ny:
                        best = max(best, int(q0[y, x]))
            out[my, mx] = best
    return out


def plane_reference(q0, level, km1, entry_size):
    """Logical entries [Y', X', byte] of the quad (4) or hex (16) plane of a
    level, X' < mw + reach, Y' < mh + reach."""
    h = 1 << level
    n = {4: 2, 16: 4}[entry_size]
    reach = (n - 1) * h
    m = widened(q0, h, km1)
    mh, mw = m.shape
    pad = np.zeros((mh + 2 * reach, mw + 2 * reach), np.uint8)
    pad[reach:reach + mh, reach:reach + mw] = m
    qh, qw = mh + reach, mw + reach
    out = np.zeros((qh, qw, entry_size), np.uint8)
    for a in range(n):
        for b in range(n):  # M(X + a h, Y + b h), X = X' - reach
            out[:, :, a * n + b] = pad[b * h:b * h + qh, a * h:a * h + qw]
    return out


def storage_index(xq, yq, period, pws, pph):
    kx, fx = divmod(xq, period)
    ky, fy = divmod(yq, period)
    return ((fy * period + fx) * pph + ky) * pws + kx


def decode_plane(raw, period, pws, pph, entry_size):
    """Raw plane bytes -> logical [Y', X', byte] over the whole storage,
    (pph P) x (pws P) entries."""
    raw = np.asarray(raw, np.uint8)
    assert raw.size == period * period * pws * pph * entry_size
    a = raw.reshape(period, period, pph, pws, entry_size)  # fy, fx, ky, kx
    return a.transpose(2, 0, 3, 1, 4).reshape(pph * period, pws * period, entry_size)


# ---------------------------------------------------------------- 3D ------

def random_brick_cells(origin, dims, seed):
    """Cell list of a HybridGrid whose known cells fill about two thirds of
    the box and include its eight corners (so the box is the brick)."""
    rng = np.random.RandomState(seed)
    nx, ny, nz = dims
    keep = rng.random_sample((nz, ny, nx)) < 2.0 / 3.0
    for z in (0, nz - 1):
        for y in (0, ny - 1):
            for x in (0, nx - 1):
                keep[z, y, x] = True
    z, y, x = np.nonzero(keep)
    ijk = np.stack([x, y, z], axis=1).astype(np.int32) + np.asarray(origin, np.int32)
    values = rng.randint(1, 32768, size=len(ijk)).astype(np.uint16)
    return ijk, values


def dense_from_cells(ijk, values, origin, dims):
    """Sparse cells -> dense [z, y, x] over a box, 0 elsewhere; every cell
    must lie in the box."""
    nx, ny, nz = dims
    out = np.zeros((nz, ny, nx), np.uint8)
    if len(ijk) == 0:
        return out
    loc = np.asarray(ijk, np.int64) - np.asarray(origin, np.int64)
    assert (loc >= 0).all() and (loc < np.array([nx, ny, nz])).all(), "cell outside the box"
    out[loc[:, 2], loc[:, 1], loc[:, 0]] = values
    return out


def oct_h(level, full_resolution_depth):
    return 1 << (level if level < full_resolution_depth else full_resolution_depth - 1)


def octet_box(level_origin, level_dims, h):
    """The level's box grown by H towards -inf on each axis."""
    if level_dims[0] == 0:
        return tuple(level_origin), tuple(level_dims)
    return tuple(o - h for o in level_origin), tuple(d + h for d in level_dims)


def octet_reference(ijk, values, level_origin, level_dims, h):
    """uint64 [z, y, x] over the octet box: byte k of cell c is the level at
    c + H (k & 1, k >> 1 & 1, k >> 2 & 1), 0 outside the level."""
    (ox, oy, oz), (nx, ny, nz) = octet_box(level_origin, level_dims, h)
    ext = dense_from_cells(ijk, values, (ox, oy, oz), (nx + h, ny + h, nz + h))
    out = np.zeros((nz, ny, nx), np.uint64)
    for k in range(8):
        dx, dy, dz = h * (k & 1), h * ((k >> 1) & 1), h * ((k >> 2) & 1)
        part = ext[dz:dz + nz, dy:dy + ny, dx:dx + nx].astype(np.uint64)
        out |= part << np.uint64(8 * k)
    return out
