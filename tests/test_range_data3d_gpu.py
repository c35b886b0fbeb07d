"""GPU: csm_range_data3d_prepare against the CPU restatement
(tests/cpp/oracle_local3d_shim.cc): every output cloud, intensity array, count
and the origin equal in bits. Sizes on both sides of a wave, of the LDS voxel
filter's limit and of the compaction tiles, the reference test's 16 000-point
sweep, a pose per point, three origins, with and without intensities, and the
degenerate sweeps: all dropped, all misses, alternating, a NaN coordinate, an
empty high-resolution cloud."""
import numpy as np
import pytest

import local3d_support as sup

SIZES = [0, 1, 63, 65, 8192, 8193, 16000, 70001]

# A current pose that is neither at the origin nor axis-aligned.
CURRENT_POSE = ((1.25, -0.5, 0.3), sup.quat_from_rpy(0.02, -0.03, 0.7))


def _both(csm, options, hits, idx, poses, inten):
    tfl, lo = sup.tracking_from_local(CURRENT_POSE)
    got = csm.range_data3d_prepare(options, hits, idx, poses, sup.ORIGINS, tfl, lo,
                                   intensities=inten)
    want = sup.prepare(options, hits, idx, poses, sup.ORIGINS, tfl, lo, intensities=inten)
    sup.assert_prepared_equal(got, want)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("with_intensities", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_prepare_equals_restatement(csm, n, with_intensities):
    hits, idx, poses, inten = sup.sweep_inputs(n, 300 + n % 17, with_intensities)
    got, _ = _both(csm, csm.RangeData3DOptions.make(), hits, idx, poses, inten)
    if n >= 63:
        # Both classes and both filtered clouds are really there.
        assert len(got["returns"]) > 0 and len(got["high"]) > 0 and len(got["low"]) > 0
    if n >= 8192:
        assert len(got["misses"]) > 0
        assert len(got["high"]) < len(got["returns"])


@pytest.mark.gpu
def test_all_below_min_range(csm):
    hits, idx, poses, inten = sup.sweep_inputs(500, 1)
    got, _ = _both(csm, csm.RangeData3DOptions.make(min_range=200.0, max_range=300.0), hits, idx,
                   poses, inten)
    assert [len(got[k]) for k in ("returns", "misses", "high", "low")] == [0, 0, 0, 0]


@pytest.mark.gpu
def test_all_beyond_max_range(csm):
    hits, idx, poses, inten = sup.sweep_inputs(9000, 2)
    got, _ = _both(csm, csm.RangeData3DOptions.make(min_range=0.1, max_range=1.0), hits, idx,
                   poses, inten)
    assert len(got["returns"]) == 0 and len(got["high"]) == 0 and len(got["misses"]) > 0


@pytest.mark.gpu
def test_alternating_returns_and_misses(csm):
    hits, idx, poses, inten = sup.sweep_inputs(9001, 3, far_fraction=0.0)
    hits[1::2] *= np.float32(40.0)  # every other ray far beyond max_range
    got, _ = _both(csm, csm.RangeData3DOptions.make(), hits, idx, poses, inten)
    assert len(got["returns"]) > 0 and len(got["misses"]) > 0


@pytest.mark.gpu
def test_one_nan_coordinate(csm):
    hits, idx, poses, inten = sup.sweep_inputs(2000, 4)
    hits[777, 1] = np.nan
    clean = np.delete(hits, 777, 0), np.delete(idx, 777), np.delete(poses, 777, 0), \
        np.delete(inten, 777)
    got, _ = _both(csm, csm.RangeData3DOptions.make(), hits, idx, poses, inten)
    # The NaN ray is dropped: the sweep without it gives the same clouds.
    tfl, lo = sup.tracking_from_local(CURRENT_POSE)
    other = csm.range_data3d_prepare(csm.RangeData3DOptions.make(), clean[0], clean[1], clean[2],
                                     sup.ORIGINS, tfl, lo, intensities=clean[3])
    sup.assert_prepared_equal(got, other)


@pytest.mark.gpu
def test_high_resolution_max_range_that_empties_the_high_cloud(csm):
    hits, idx, poses, inten = sup.sweep_inputs(9000, 5)
    high = csm.AdaptiveVoxelFilterOptions.make(2.0, 150, 0.5)  # the walls are metres away
    got, _ = _both(csm, csm.RangeData3DOptions.make(high_resolution_adaptive_voxel_filter=high),
                   hits, idx, poses, inten)
    assert len(got["high"]) == 0 and len(got["low"]) > 0


@pytest.mark.gpu
def test_same_input_twice_gives_the_same_bytes(csm):
    hits, idx, poses, inten = sup.sweep_inputs(16000, 6)
    tfl, lo = sup.tracking_from_local(CURRENT_POSE)
    runs = [csm.range_data3d_prepare(csm.RangeData3DOptions.make(), hits, idx, poses, sup.ORIGINS,
                                     tfl, lo, intensities=inten) for _ in range(2)]
    for key, value in runs[0].items():
        assert value.tobytes() == runs[1][key].tobytes(), key
