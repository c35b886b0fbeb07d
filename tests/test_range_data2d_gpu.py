"""GPU: csm_range_data2d_prepare and csm_range_data_transform against the CPU
restatement (tests/cpp/oracle_local2d_shim.cc): equal counts and every float
bit-equal. The sizes sit on the wave (64), workgroup (1024) and limit (8192)
edges of the ordered compaction; the clouds are room sweeps jittered in z, with
a pose per point, three origins and a tilted gravity alignment."""
import ctypes as C
import functools

import numpy as np
import pytest

import local2d_support as sup

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 257, 1025, 8192]
ORIGINS = np.array([[0.0, 0.0, 0.0], [0.1, -0.05, 0.02], [-0.08, 0.06, -0.01]], np.float32)
# The tracking frame against gravity: a small tilt, a yaw and a shift.
GRAVITY_FROM_LOCAL = np.array([0.3, -0.2, 0.01, *sup.quat_from_rpy(0.02, -0.015, 0.4)], np.float32)
LOCAL_ORIGIN = np.array([0.05, -0.02, 0.01], np.float32)


def _options(csm, **kw):
    # The room's walls are 3 to 5 m away: max_range 4.2 m leaves both returns
    # and misses; the z crop cuts into what the jitter, the per-point rotations
    # and the tilt spread over about +-0.2 m.
    base = dict(min_range=0.5, max_range=4.2, missing_data_ray_length=2.5, min_z=-0.12,
                max_z=0.12, voxel_filter_size=0.05,
                adaptive_voxel_filter=csm.AdaptiveVoxelFilterOptions.make(0.5, 10, 50.0))
    base.update(kw)
    return csm.RangeData2DOptions.make(**base)


@functools.lru_cache(maxsize=None)
def _sweep(n):
    """(hits, origin_index, poses) of a seeded n-point sweep."""
    rng = np.random.default_rng(1000 + n)
    hits = sup.room_hits(rng, n)
    index = rng.integers(0, len(ORIGINS), n).astype(np.int32)
    poses = sup.random_poses(rng, n)
    for a in (hits, index, poses):
        a.setflags(write=False)
    return hits, index, poses


def _assert_same(got, want, what):
    names = ("origin", "returns", "misses", "filtered")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert g.dtype == np.float32 and w.dtype == np.float32
        diff = int((g.view(np.uint32) != w.view(np.uint32)).sum())
        assert diff == 0, (what, name, diff)


def _run_both(csm, options, hits, index, poses, origins=ORIGINS, gravity=GRAVITY_FROM_LOCAL,
              local_origin=LOCAL_ORIGIN):
    want = sup.prepare(options, hits, index, poses, origins, gravity, local_origin)
    got = csm.range_data2d_prepare(options, hits, index, poses, origins, gravity, local_origin)
    return got, want


@pytest.mark.parametrize("n", SIZES)
def test_prepare_equals_restatement(csm, n):
    hits, index, poses = _sweep(n)
    got, want = _run_both(csm, _options(csm), hits, index, poses)
    print(n, [len(w) for w in want[1:]])
    if n >= 63:  # chosen so that the restatement alone yields every kind of output
        assert len(want[1]) >= 10 and len(want[2]) >= 10 and len(want[3]) >= 5
    if n >= 255:
        assert len(want[3]) < len(want[1])  # the adaptive filter did filter
    _assert_same(got, want, n)


def test_prepare_with_the_lua_filter_sizes(csm):
    """trajectory_builder_2d.lua's 0.025 m voxels and (0.5, 200, 50) adaptive filter."""
    hits, index, poses = _sweep(1025)
    o = _options(csm, voxel_filter_size=0.025,
                 adaptive_voxel_filter=csm.AdaptiveVoxelFilterOptions.make(0.5, 200, 50.0))
    got, want = _run_both(csm, o, hits, index, poses)
    assert len(want[1]) >= 200 and len(want[2]) >= 10 and 5 <= len(want[3]) < len(want[1])
    _assert_same(got, want, "lua")


def test_prepare_oversized_is_erange(csm):
    n = 8193
    hits = np.ones((n, 3), np.float32)
    with pytest.raises(csm.CsmError) as e:
        csm.range_data2d_prepare(_options(csm), hits, np.zeros(n, np.int32),
                                 sup.identity_poses(n), ORIGINS, sup.IDENTITY_TQ, LOCAL_ORIGIN)
    assert f"({csm.CSM_ERANGE})" in str(e.value)


DEGENERATE = {
    "all_below_min_range": dict(min_range=100.0),
    "all_misses": dict(min_range=0.0, max_range=0.1),
    "all_cropped": dict(min_z=10.0, max_z=11.0),
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_prepare_degenerate_clouds(csm, name):
    hits, index, poses = _sweep(257)
    got, want = _run_both(csm, _options(csm, **DEGENERATE[name]), hits, index, poses)
    nr, nm, nf = (len(w) for w in want[1:])
    if name == "all_misses":
        assert nr == 0 and nm >= 10 and nf == 0
    else:
        assert nr == 0 and nm == 0 and nf == 0
    _assert_same(got, want, name)


def test_prepare_alternating_returns_and_misses(csm):
    """Even points at 2 m, odd points at 6 m, max_range 4 m: both compactions
    take every other point."""
    n = 1025
    ang = np.linspace(-np.pi, np.pi, n, endpoint=False)
    rad = np.where(np.arange(n) % 2 == 0, 2.0, 6.0)
    hits = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n)], 1).astype(np.float32)
    o = _options(csm, min_range=0.0, max_range=4.0, missing_data_ray_length=3.0, min_z=-1.0,
                 max_z=1.0, voxel_filter_size=0.01)
    index = np.zeros(n, np.int32)
    want = sup.prepare(o, hits, index, sup.identity_poses(n), ORIGINS[:1], sup.IDENTITY_TQ,
                       np.zeros(3, np.float32))
    assert len(want[1]) == (n + 1) // 2 and len(want[2]) == n // 2  # one point per voxel
    assert np.array_equal(want[1], hits[0::2])
    got = csm.range_data2d_prepare(o, hits, index, sup.identity_poses(n), ORIGINS[:1],
                                   sup.IDENTITY_TQ, np.zeros(3, np.float32))
    _assert_same(got, want, "alternating")


def test_prepare_one_nan_point_in_the_middle(csm):
    hits, index, poses = _sweep(257)
    hits = hits.copy()
    hits[128, 1] = np.nan
    got, want = _run_both(csm, _options(csm), hits, index, poses)
    assert len(want[1]) >= 10 and len(want[2]) >= 10 and len(want[3]) >= 5
    assert not np.isnan(want[1]).any() and not np.isnan(want[2]).any()
    _assert_same(got, want, "nan")


def test_prepare_hand_computed_boundaries(csm):
    """The cases test_local2d_host.py works out by hand, on the device."""
    below = np.nextafter(np.float32(1.0), np.float32(0.0))
    z_above = np.nextafter(np.float32(0.5), np.float32(1.0))
    hits = np.array([[3, 4, 0], [6, 8, 0], [1, 0, 0], [below, 0, 0], [np.nan, 0, 0],
                     [2, 0, -0.5], [0, 2, 0.5], [-2, 0, z_above]], np.float32)
    n = len(hits)
    o = _options(csm, min_range=1.0, max_range=5.0, missing_data_ray_length=2.0, min_z=-0.5,
                 max_z=0.5, voxel_filter_size=0.025)
    got = csm.range_data2d_prepare(o, hits, np.zeros(n, np.int32), sup.identity_poses(n),
                                   np.zeros((1, 3), np.float32), sup.IDENTITY_TQ,
                                   np.zeros(3, np.float32))
    s = np.float32(2.0) / np.float32(10.0)
    assert got[1].tolist() == [[3, 4, 0], [1, 0, 0], [2, 0, -0.5], [0, 2, 0.5]]
    assert got[2].tobytes() == np.array([[s * np.float32(6), s * np.float32(8), 0]],
                                        np.float32).tobytes()
    assert got[3].tolist() == got[1].tolist()  # fewer than min_num_points: all kept
    assert got[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("counts", [(0, 0), (1, 0), (65, 257), (100000, 3)])
def test_transform_equals_restatement(csm, counts):
    rng = np.random.default_rng(counts[0] + 7)
    returns = rng.uniform(-30, 30, (counts[0], 3)).astype(np.float32)
    misses = rng.uniform(-30, 30, (counts[1], 3)).astype(np.float32)
    origin = np.array([1.5, -2.5, 0.25], np.float32)
    tq = np.array([3.0, -1.0, 0.5, *sup.quat_from_rpy(0.1, -0.2, 2.0)], np.float32)
    want = sup.transform(tq, origin, returns, misses)
    got = csm.range_data_transform(tq, origin, returns, misses)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes()
    if counts[0]:
        assert not np.array_equal(got[1], returns)


def test_prepare_rejects_bad_arguments(csm):
    hits, index, poses = _sweep(65)
    ok = _options(csm)

    def code(options=ok, index=index, num_origins=len(ORIGINS), null=None):
        ctx = csm.default_context()
        F, I = C.c_float, C.c_int32
        origin = np.zeros(3, np.float32)
        outs = [np.zeros((65, 3), np.float32) for _ in range(3)]
        counts = [I(0) for _ in range(3)]
        idx = np.ascontiguousarray(index, np.int32)
        args = dict(hits=csm._ptr(hits, F), index=csm._ptr(idx, I), poses=csm._ptr(poses, F),
                    origins=csm._ptr(ORIGINS, F), returns=csm._ptr(outs[0], F),
                    misses=csm._ptr(outs[1], F), filtered=csm._ptr(outs[2], F))
        if null:
            args[null] = None
        return ctx._lib.csm_range_data2d_prepare(
            ctx.handle, C.byref(options), args["hits"], args["index"], args["poses"], 65,
            args["origins"], num_origins, csm._ptr(GRAVITY_FROM_LOCAL, F),
            csm._ptr(LOCAL_ORIGIN, F), csm._ptr(origin, F), args["returns"], C.byref(counts[0]),
            args["misses"], C.byref(counts[1]), args["filtered"], C.byref(counts[2]))

    assert code() == csm.CSM_OK
    for null in ("hits", "index", "poses", "origins", "returns", "misses", "filtered"):
        assert code(null=null) == csm.CSM_EINVAL, null
    low, high = index.copy(), index.copy()
    low[7], high[64] = -1, len(ORIGINS)
    assert code(index=low) == csm.CSM_EINVAL
    assert code(index=high) == csm.CSM_EINVAL
    assert code(num_origins=2) == csm.CSM_EINVAL  # _sweep(65) uses all three origins
    assert code(options=_options(csm, voxel_filter_size=0.0)) == csm.CSM_EINVAL
    assert code(options=_options(csm, voxel_filter_size=-0.05)) == csm.CSM_EINVAL
    bad = _options(csm, adaptive_voxel_filter=csm.AdaptiveVoxelFilterOptions.make(0.0, 40, 50.0))
    assert code(options=bad) == csm.CSM_EINVAL
    assert code() == csm.CSM_OK  # and the context still works
