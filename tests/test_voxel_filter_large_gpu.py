"""GPU: csm_voxel_filter_large and csm_adaptive_voxel_filter_large against the
oracle, bit-exact on the kept set and the count: cloud sizes on both sides of
the LDS kernel's 8192-point limit, of the 1024-point tiles and of 65 536 (where
16-bit ranks end), a single voxel of 140 000 points (four rejected draws, five
draw passes, ranks above 65 535), wrapping keys, identical points, the 2^20
limit, and every branch of the adaptive edge-length search with both option
sets of trajectory_builder_3d.lua."""
import numpy as np
import pytest

import local3d_support as sup

SIZES = [1, 8192, 8193, 16384, 16385, 65537, 100003]
RESOLUTIONS = [0.075, 0.15, 1.0]

_reference = {}


def _oracle_mask(oracle, key, cloud, resolution):
    """The oracle's mask, computed once per (cloud, resolution)."""
    k = (key, resolution)
    if k not in _reference:
        _reference[k] = oracle.voxel_filter_masks([cloud], resolution)[0]
        _reference[k].setflags(write=False)
    return _reference[k]


def _check(csm, oracle, key, cloud, resolution):
    keep, count = csm.voxel_filter_large_mask(cloud, resolution)
    want = _oracle_mask(oracle, key, cloud, resolution)
    assert count == int(want.sum())
    np.testing.assert_array_equal(keep, want)
    return keep


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_cloud3d_sizes_match_oracle(csm, oracle, n):
    cloud = sup.cloud3d(n, 100 + n % 13)
    for res in RESOLUTIONS:
        _check(csm, oracle, ("cloud3d", n), cloud, res)


@pytest.mark.gpu
def test_single_voxel_of_140000_points(csm, oracle):
    """Ranks up to 139 999 and the four rejected draws of
    test_local3d_host.py::test_rejections_of_a_single_voxel_of_140000_points:
    the kept point is the reference's only if every redraw lands in place."""
    cloud = sup.single_voxel_cloud(140000)
    keep = _check(csm, oracle, "voxel140000", cloud, 0.3)
    assert keep.sum() == 1


@pytest.mark.gpu
def test_single_voxel_of_2000_points(csm, oracle):
    cloud = sup.single_voxel_cloud(2000)
    assert _check(csm, oracle, "voxel2000", cloud, 0.3).sum() == 1
    # Several voxels with long runs each: the rejection falls inside one of them.
    _check(csm, oracle, "voxel2000", cloud, 0.02)


@pytest.mark.gpu
def test_negative_coordinates_whose_keys_wrap(csm, oracle):
    cloud = -np.abs(sup.cloud3d(9000, 5, 0.5))
    for res in (0.01, 0.15):
        _check(csm, oracle, "negative", cloud, res)
    big = sup.cloud3d(9001, 6, 1e4)
    _check(csm, oracle, "big", big, 0.01)


@pytest.mark.gpu
def test_identical_points(csm, oracle):
    cloud = np.tile(np.array([[1e5, -2e5, 3.0]], np.float32), (300, 1))
    for res in RESOLUTIONS:
        assert _check(csm, oracle, "identical", cloud, res).sum() == 1


@pytest.mark.gpu
def test_empty_cloud(csm):
    keep, count = csm.voxel_filter_large_mask(np.zeros((0, 3), np.float32), 0.1)
    assert len(keep) == 0 and count == 0
    opts = csm.AdaptiveVoxelFilterOptions.make(*sup.HIGH_OPTIONS)
    keep, count = csm.adaptive_voxel_filter_large_mask(np.zeros((0, 3), np.float32), opts)
    assert len(keep) == 0 and count == 0


@pytest.mark.gpu
def test_cloud_at_the_limit(csm, oracle):
    n = 2**20
    cloud = sup.cloud3d(n, 77, 40.0)
    _check(csm, oracle, "limit", cloud, 0.15)
    with pytest.raises(csm.CsmError):
        csm.voxel_filter_large_mask(np.zeros((n + 1, 3), np.float32), 0.15)


@pytest.mark.gpu
def test_results_do_not_depend_on_what_ran_before(csm, oracle):
    """The working memory grows on demand and is reused: a small cloud after
    a large one, and the same cloud twice."""
    big, small = sup.cloud3d(100003, 100 + 100003 % 13), sup.cloud3d(8193, 100 + 8193 % 13)
    a = _check(csm, oracle, ("cloud3d", 100003), big, 0.15)
    _check(csm, oracle, ("cloud3d", 8193), small, 0.15)
    b = _check(csm, oracle, ("cloud3d", 100003), big, 0.15)
    assert a.tobytes() == b.tobytes()


# ---- AdaptiveVoxelFilter ----------------------------------------------------

ADAPTIVE_BRANCH = {
    "far_8193_high": "none", "tiled_8193_low": "exhausted",
    "compact_20000_high": "bisect", "compact_20000_low": "bisect",
    "wide_70000_high": "one", "wide_70000_low": "one",
}


def adaptive_cases():
    """(name, cloud, (max_length, min_num_points, max_range)): both option sets
    on clouds of 8193, 20 000 and 70 000 points. test_local3d_host.py checks on
    the CPU that they take the branches ADAPTIVE_BRANCH names."""
    tiled = np.tile(sup.cloud3d(100, 3, 5.0), (82, 1))[:8193]
    return [
        ("far_8193_high", sup.cloud3d(8193, 41, 200.0), sup.HIGH_OPTIONS),
        ("tiled_8193_low", np.ascontiguousarray(tiled), sup.LOW_OPTIONS),
        ("compact_20000_high", sup.cloud3d(20000, 42, 1.0), sup.HIGH_OPTIONS),
        ("compact_20000_low", sup.cloud3d(20000, 43, 1.5), sup.LOW_OPTIONS),
        ("wide_70000_high", sup.cloud3d(70000, 44, 20.0), sup.HIGH_OPTIONS),
        ("wide_70000_low", sup.cloud3d(70000, 45, 20.0), sup.LOW_OPTIONS),
    ]


def branch_of(passes, kept, min_num_points):
    """Which way AdaptivelyVoxelFiltered (voxel_filter.cc:38-76) went."""
    if passes == 0:
        return "none"
    if passes == 1:
        return "one"
    if kept < min_num_points:
        return "exhausted"
    return "bisect" if passes > 2 else "halved"


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(6))
def test_adaptive_matches_oracle(csm, oracle, index):
    name, cloud, options = adaptive_cases()[index]
    opts = csm.AdaptiveVoxelFilterOptions.make(*options)
    keep, count = csm.adaptive_voxel_filter_large_mask(cloud, opts)
    want, _ = oracle.adaptive_voxel_filter_masks([cloud], *options)
    assert count == int(want.sum())
    np.testing.assert_array_equal(keep, want)
    shim_keep, passes = sup.adaptive(cloud, options)
    np.testing.assert_array_equal(keep, shim_keep)
    assert branch_of(passes, count, options[1]) == ADAPTIVE_BRANCH[name]
