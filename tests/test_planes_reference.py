"""CPU: the numpy references of the search planes and octets
(planes_support.py) agree with the oracle where the oracle defines the same
thing, so the GPU tests built on them are not vacuous."""
import numpy as np
import pytest

import planes_support as ps


@pytest.mark.parametrize("ny,nx,depth", [(4, 4, 8), (29, 37, 6), (1, 1, 3)])
def test_quad_reference_byte0_is_the_oracle_level(oracle, ny, nx, depth):
    """Without clustering (km1 = 0) M is the oracle's level l, so byte 0 of
    the quad entry (X', Y') is level l at wide cell (X' - h, Y' - h), 0
    outside; the other bytes are the same level h further."""
    cells = ps.random_cells(ny, nx, seed=11)
    limits = (0.05, 0.05 * ny, 0.05 * nx)
    om = oracle.fast2d(limits, cells, 1.0, 1.0, depth)
    q0 = om.level(0)
    assert q0.shape == (ny, nx) and q0.any()
    for level in range(depth):
        h = 1 << level
        lv = om.level(level)
        np.testing.assert_array_equal(ps.widened(q0, h, 0), lv)
        ref = ps.plane_reference(q0, level, 0, 4)
        wny, wnx = lv.shape
        assert ref.shape == (wny + h, wnx + h, 4)
        pad = np.zeros((wny + 2 * h, wnx + 2 * h), np.uint8)
        pad[h:h + wny, h:h + wnx] = lv
        np.testing.assert_array_equal(ref[:, :, 0], pad[:wny + h, :wnx + h])
        np.testing.assert_array_equal(ref[:, :, 1], pad[h:, :wnx + h])
        np.testing.assert_array_equal(ref[:, :, 2], pad[:wny + h, h:])
        np.testing.assert_array_equal(ref[:, :, 3], pad[h:, h:])


def test_hex_reference_bytes_are_the_oracle_level(oracle):
    cells = ps.random_cells(13, 9, seed=5)
    om = oracle.fast2d((0.05, 1.0, 1.0), cells, 1.0, 1.0, 4)
    q0 = om.level(0)
    for level in range(4):
        h = 1 << level
        lv = om.level(level)
        wny, wnx = lv.shape
        ref = ps.plane_reference(q0, level, 0, 16)
        assert ref.shape == (wny + 3 * h, wnx + 3 * h, 16)
        pad = np.zeros((wny + 6 * h, wnx + 6 * h), np.uint8)
        pad[3 * h:3 * h + wny, 3 * h:3 * h + wnx] = lv
        for a in range(4):
            for b in range(4):
                np.testing.assert_array_equal(
                    ref[:, :, 4 * a + b],
                    pad[b * h:b * h + wny + 3 * h, a * h:a * h + wnx + 3 * h], err_msg=f"{a} {b}")


@pytest.mark.parametrize("h,km1", [(1, 0), (2, 1), (4, 3), (8, 7), (4, 0)])
def test_windowed_maximum_against_cell_by_cell(h, km1):
    q0 = np.random.RandomState(3).randint(0, 256, size=(5, 7)).astype(np.uint8)
    q0[q0 < 80] = 0
    np.testing.assert_array_equal(ps.widened(q0, h, km1), ps.widened_naive(q0, h, km1))


@pytest.mark.parametrize("h,km1", [(2, 1), (4, 3), (8, 7), (16, 3)])
def test_wider_window_dominates_and_equals_over_zero_cells(h, km1):
    """The window of M with km1 > 0 ending at a cell contains the km1 = 0
    window ending there: it is never smaller, and equal wherever the cells it
    adds are all zero."""
    q0 = np.zeros((23, 31), np.uint8)
    q0[6:15, 9:20] = np.random.RandomState(9).randint(1, 256, size=(9, 11))
    wide, narrow = ps.widened(q0, h, km1), ps.widened(q0, h, 0)
    mh, mw = narrow.shape
    assert (wide[:mh, :mw] >= narrow).all()
    assert (wide[:mh, :mw] > narrow).any()
    ny, nx = q0.shape
    pad = np.zeros((ny + 2 * (h + km1), nx + 2 * (h + km1)), np.uint8)
    o = h + km1
    pad[o:o + ny, o:o + nx] = q0
    checked = 0
    for my in range(mh):
        for mx in range(mw):
            y1, x1 = my + o + 1, mx + o + 1  # one past the window's end in pad
            big = pad[y1 - h - km1:y1, x1 - h - km1:x1]
            small = pad[y1 - h:y1, x1 - h:x1]
            if big.sum(dtype=np.int64) == small.sum(dtype=np.int64):  # only zeros added
                assert wide[my, mx] == narrow[my, mx], (mx, my)
                checked += 1
    assert checked > 0


@pytest.mark.parametrize("period,pws,pph,es", [(2, 3, 2, 4), (8, 2, 3, 16), (4, 1, 1, 4)])
def test_decode_follows_the_polyphase_index(period, pws, pph, es):
    n = period * period * pws * pph
    raw = np.random.RandomState(1).randint(0, 256, size=n * es).astype(np.uint8)
    logical = ps.decode_plane(raw, period, pws, pph, es)
    assert logical.shape == (pph * period, pws * period, es)
    entries = raw.reshape(n, es)
    seen = set()
    for yq in range(pph * period):
        for xq in range(pws * period):
            i = ps.storage_index(xq, yq, period, pws, pph)
            seen.add(i)
            assert np.array_equal(logical[yq, xq], entries[i]), (xq, yq)
    assert seen == set(range(n))


def test_expected_layout_rules():
    assert ps.expected_kinds(8, {7, 5}) == [4, 4, 4, 16, 0, 16, 0, 4]
    assert ps.expected_kinds(8, set()) == [4] * 8
    assert ps.expected_kinds(8, {2, 4, 6}) == [16, 0, 16, 0, 16, 0, 4, 4]
    assert ps.expected_kinds(1, set()) == [4]
    assert ps.expected_hex_mask(8, {}) == {7, 5}
    assert ps.expected_hex_mask(3, {}) == {2}
    assert ps.expected_hex_mask(8, {"CSM_SEARCH_KERNEL": "5"}) == {2, 4, 6}
    assert ps.expected_hex_mask(6, {"CSM_HEX_LEVELS": "8,6,3"}) == {3}
    assert ps.expected_cshift({})[:7] == [0, 0, 2, 2, 2, 3, 3]
    assert ps.expected_cshift({"CSM_CLUSTER": "3"})[:6] == [0, 1, 2, 3, 3, 3]
    assert ps.expected_cshift({"CSM_CLUSTER": "0"}) == [0] * 12
    assert ps.expected_depth(5, 0, 130, 70) == 8
    assert ps.expected_depth(8, 0, 4, 4) == 8


@pytest.mark.parametrize("depth,full_depth", [(3, 3), (4, 2)])
def test_octet_reference_byte0_is_the_oracle_level(oracle, depth, full_depth):
    """Byte 0 of the octet at c is the oracle's level at c; byte k the level H
    (k's bits) further; the box is the cells' own box grown by H below."""
    ijk, values = ps.random_brick_cells((-7, -5, -3), (6, 5, 4), seed=2)
    og = oracle.hybrid_grid(0.1)
    og.set_values(ijk, values)
    om = oracle.fast3d(og, og, np.zeros(10, np.float32), (depth, full_depth, 0.1, 0.15, 0.8, 0.8, 0.3))
    for level in range(depth):
        cells, v = om.level(level)
        assert len(v) > 0
        lo, hi = cells.min(axis=0), cells.max(axis=0)
        origin, dims = tuple(lo), tuple(hi - lo + 1)
        h = ps.oct_h(level, full_depth)
        assert h == (1 << level if level < full_depth else 1 << (full_depth - 1))
        (ox, oy, oz), (nx, ny, nz) = ps.octet_box(origin, dims, h)
        assert (ox, oy, oz) == tuple(lo - h) and (nx, ny, nz) == tuple(hi - lo + 1 + h)
        ref = ps.octet_reference(cells, v, origin, dims, h)
        assert ref.shape == (nz, ny, nx)
        lookup = {tuple(c): int(x) for c, x in zip(cells.tolist(), v.tolist())}
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    c = (ox + x, oy + y, oz + z)
                    word = int(ref[z, y, x])
                    for k in range(8):
                        at = (c[0] + h * (k & 1), c[1] + h * ((k >> 1) & 1), c[2] + h * ((k >> 2) & 1))
                        assert (word >> (8 * k)) & 0xff == lookup.get(at, 0), (level, c, k)
