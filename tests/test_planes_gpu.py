"""GPU: the quad and hex planes fast2d_search_v4 / v5 load (pyramid_quad,
pyramid_widen, pyramid_hex, laid out by Fast2dCreate), read back raw and
compared byte for byte with a brute-force reference made from level 0 alone
(planes_support.py): the widening by the cluster size, the 0-outside rule at
the grid edges, the polyphase index and the zero padding of the storage.
Every comparison is equality on integers."""
import numpy as np
import pytest

import planes_support as ps

pytestmark = pytest.mark.gpu

# name: (ny, nx, branch_and_bound_depth, search_depth)
GRIDS = {
    "4x4-d8": (4, 4, 8, 8),          # every window and period wider than the grid
    "37x29-d6": (29, 37, 6, 6),      # no dimension a multiple of any period
    "130x70-auto": (70, 130, 5, 0),  # automatic depth above branch_and_bound_depth
    "1x1-d3": (1, 1, 3, 3),
}
KERNELS = {
    "default": {},
    "v4": {"CSM_SEARCH_KERNEL": "4"},
    "v5-all-hex": {"CSM_SEARCH_KERNEL": "5"},
    "mixed": {"CSM_HEX_LEVELS": "8,6,3"},
}
CLUSTERS = {"cluster-default": None, "cluster-0": "0", "cluster-3": "3"}
LIMITS = (0.05, 2.0, 3.0)
CREATE_VARIABLES = ("CSM_SEARCH_KERNEL", "CSM_HEX_LEVELS", "CSM_SEARCH_ORDER", "CSM_CLUSTER")


@pytest.fixture(scope="module")
def level0(oracle):
    """Per grid: its cells and the quantised level 0 (the oracle's, which the
    device's level 0 equals bit for bit)."""
    out = {}
    for i, (name, (ny, nx, _, _)) in enumerate(GRIDS.items()):
        cells = ps.random_cells(ny, nx, seed=100 + i)
        out[name] = (cells, oracle.fast2d(LIMITS, cells, 1.0, 1.0, 1).level(0))
    return out


@pytest.fixture(scope="module")
def reference_planes():
    return {}  # (grid, level, km1, entry size) -> logical entries, made once


def set_create_variables(monkeypatch, env):
    """The plane layout is fixed when a matcher is created: the variables are
    set before."""
    for var in CREATE_VARIABLES:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)


def read_all_planes(matcher, depth):
    return [matcher.read_plane(level) for level in range(depth)]


def check_planes(csm, matcher, grid_name, q0, bbd, search_depth, env, cache):
    ny, nx = q0.shape
    depth = ps.expected_depth(bbd, search_depth, nx, ny)
    kinds = ps.expected_kinds(depth, ps.expected_hex_mask(depth, env))
    cshift = ps.expected_cshift(env)
    with pytest.raises(csm.CsmError):
        matcher.read_plane(depth)
    checked = {4: 0, 16: 0}
    for level in range(depth):
        lay, raw = matcher.read_plane(level)
        es = lay["entry_size"]
        assert es == kinds[level], (level, lay, kinds)
        assert lay["cshift"] == cshift[level], (level, lay)
        if es == 0:
            assert lay["bytes"] == 0 and raw.size == 0
            continue
        h, km1 = 1 << level, (1 << cshift[level]) - 1
        reach, period = (3 * h, 4 * h) if es == 16 else (h, 2 * h)
        qw, qh = nx + h - 1 + km1 + reach, ny + h - 1 + km1 + reach
        pws, pph = -(-qw // period), -(-qh // period)
        want = dict(entry_size=es, quad_w=qw, quad_h=qh, quad_pws=pws, quad_pph=pph,
                    quad_bias=(h - 1) + km1 + reach, cshift=cshift[level],
                    bytes=period * period * pws * pph * es)
        assert lay == want, level
        assert raw.size == want["bytes"]
        key = (grid_name, level, km1, es)
        if key not in cache:
            cache[key] = ps.plane_reference(q0, level, km1, es)
        ref = cache[key]
        assert ref.shape == (qh, qw, es)
        got = ps.decode_plane(raw, period, pws, pph, es)
        bad = np.argwhere(got[:qh, :qw] != ref)
        assert len(bad) == 0, (
            f"level {level} entry bytes {es}: {len(bad)} bytes differ, first (Y', X', byte) "
            f"{bad[0].tolist()}: device {got[tuple(bad[0])]} reference {ref[tuple(bad[0])]}")
        # Storage entries past quad_w x quad_h are zero.
        assert not got[qh:].any() and not got[:, qw:].any(), level
        checked[es] += 1
    assert checked[4] == kinds.count(4) and checked[16] == kinds.count(16)
    assert checked[4] >= 1  # the top level always has a quad plane
    return kinds


@pytest.mark.parametrize("cluster", list(CLUSTERS))
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("grid_name", list(GRIDS))
def test_planes_match_reference(csm, level0, reference_planes, monkeypatch, grid_name, kernel,
                                cluster):
    env = dict(KERNELS[kernel])
    if CLUSTERS[cluster] is not None:
        env["CSM_CLUSTER"] = CLUSTERS[cluster]
    set_create_variables(monkeypatch, env)
    _, _, bbd, search_depth = GRIDS[grid_name]
    cells, q0 = level0[grid_name]
    opts = csm.FastCorrelativeScanMatcherOptions2D(3.0, 1.0, bbd, search_depth=search_depth)
    m = csm.FastCorrelativeScanMatcher2D(csm.ProbabilityGrid(*LIMITS, cells), opts)
    try:
        np.testing.assert_array_equal(m.read_level(0), q0)
        kinds = check_planes(csm, m, grid_name, q0, bbd, search_depth, env, reference_planes)
    finally:
        m.close()
    if kernel == "v4":
        assert 16 not in kinds
    elif len(kinds) >= 3 and kernel != "mixed":
        assert 16 in kinds
    if kernel == "mixed" and len(kinds) >= 6:
        assert 16 in kinds and kinds.count(4) >= 3


def test_device_grid_planes_equal_host_cells_planes(csm, level0, monkeypatch):
    """csm_fast2d_create_from_grid: the planes of a device-resident grid are
    those of a create from the same cells on the host."""
    set_create_variables(monkeypatch, {})
    cells, _ = level0["37x29-d6"]
    opts = csm.FastCorrelativeScanMatcherOptions2D(3.0, 1.0, 6, search_depth=6)
    host = csm.FastCorrelativeScanMatcher2D(csm.ProbabilityGrid(*LIMITS, cells), opts)
    dev_grid = csm.DeviceProbabilityGrid(*LIMITS, cells.shape[1], cells.shape[0], cells)
    dev = csm.FastCorrelativeScanMatcher2D(dev_grid, opts)
    kinds = set()
    for level in range(6):
        (hl, hb), (dl, db) = host.read_plane(level), dev.read_plane(level)
        assert hl == dl and np.array_equal(hb, db), level
        kinds.add(hl["entry_size"])
    assert {4, 16} <= kinds
    for x in (host, dev, dev_grid):
        x.close()


def test_tsdf_planes_equal_host_cells_planes(csm, level0, monkeypatch):
    """csm_fast2d_create_tsdf: the planes of a TSDF matcher are those of a
    create from the same TSD cells with the TSDF's cost bounds."""
    set_create_variables(monkeypatch, {})
    cells, _ = level0["37x29-d6"]
    weights = np.random.RandomState(8).randint(0, 32768, size=cells.shape).astype(np.uint16)
    truncation = 0.3
    opts = csm.FastCorrelativeScanMatcherOptions2D(3.0, 1.0, 6, search_depth=6)
    host = csm.FastCorrelativeScanMatcher2D(
        csm.ProbabilityGrid(*LIMITS, cells, -truncation, truncation), opts)
    tsdf = csm.FastCorrelativeScanMatcher2D(
        csm.TSDF2D(*LIMITS, cells, weights, truncation, 10.0), opts)
    kinds = set()
    for level in range(6):
        (hl, hb), (tl, tb) = host.read_plane(level), tsdf.read_plane(level)
        assert hl == tl and np.array_equal(hb, tb), level
        assert hb.any() or hl["entry_size"] == 0
        kinds.add(hl["entry_size"])
    assert {4, 16} <= kinds
    host.close()
    tsdf.close()
