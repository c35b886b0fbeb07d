"""CPU: the host side of 3D range-data insertion on device HybridGrids: the
update lookup tables and RotateHistogram against the oracle's, the new C-ABI
entries (declared, exported, bound), and the argument checks that return before
any device is touched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, ensure_built

import insert3d_support as sup

NEW_ENTRIES = [
    "csm_hybrid_grid_insert", "csm_hybrid_grid_insert_batch", "csm_hybrid_grid_read",
    "csm_hybrid_grid_insert_stats", "csm_inserter3d_lookup_table", "csm_rotate_histogram",
]

FP = C.POINTER(C.c_float)


def fp(a):
    return a.ctypes.data_as(FP)


@pytest.mark.parametrize("p", [0.55, 0.49, 0.7, 0.4])
def test_lookup_table_equals_oracle(csm, oracle, p):
    """ComputeLookupTableToApplyOdds(Odds(p)), all 32768 entries with the
    update marker, against the oracle's table."""
    from cartographer_amd import matching3d
    got = matching3d.inserter3d_lookup_table(p)
    want = sup.oracle_table(p)
    assert got.dtype == np.uint16 and got.shape == (32768,)
    assert np.array_equal(got, want)
    assert (got >= 32768).all()  # every entry carries the marker


def test_lookup_table_rejects_bad_probability(csm):
    lib = csm.load_library()
    out = np.zeros(32768, np.uint16)
    ptr = out.ctypes.data_as(C.POINTER(C.c_uint16))
    for p in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert lib.csm_inserter3d_lookup_table(p, ptr) == csm.CSM_EINVAL
    assert lib.csm_inserter3d_lookup_table(0.5, None) == csm.CSM_EINVAL


def _boundary_angle(size, buckets):
    """An angle whose rotate_by_buckets = -angle * size / pi is exactly
    `buckets` in the reference's float arithmetic (searched for, then checked)."""
    a = np.float32(-buckets * math.pi / size)
    for cand in (a, np.nextafter(a, np.float32(0)), np.nextafter(a, np.float32(-10))):
        got = np.float32(np.float64(np.float32(-cand) * np.float32(size)) / math.pi)
        if got == np.float32(buckets):
            return float(cand)
    raise AssertionError("no float angle lands on the bucket boundary")


ANGLES = [0.0, math.pi / 2, -math.pi / 2,
          float(np.nextafter(np.float32(math.pi), np.float32(0))),
          float(np.nextafter(np.float32(-math.pi), np.float32(0))),
          0.3, -2.9, _boundary_angle(120, 7), _boundary_angle(120, -13)]


@pytest.mark.parametrize("angle", ANGLES)
def test_rotate_histogram_equals_oracle(csm, oracle, angle):
    """RotationalScanMatcher::RotateHistogram at size 120: 0, +-pi/2, just
    inside +-pi, two ordinary angles and two that land exactly on a bucket
    boundary (fraction 0.5 after the -0.5 shift is the lround tie)."""
    from cartographer_amd import matching3d
    rng = np.random.default_rng(5)
    h = rng.uniform(0.0, 3.0, 120).astype(np.float32)
    got = matching3d.rotate_histogram(h, angle)
    want = sup.oracle_rotate_histogram(h, angle)
    assert got.tobytes() == want.tobytes()
    if angle == 0.0:
        assert got.tobytes() == h.tobytes()


def test_rotate_histogram_arguments(csm):
    lib = csm.load_library()
    h = np.ones(8, np.float32)
    out = np.zeros(8, np.float32)
    assert lib.csm_rotate_histogram(None, 8, 0.1, fp(out)) == csm.CSM_EINVAL
    assert lib.csm_rotate_histogram(fp(h), 8, 0.1, None) == csm.CSM_EINVAL
    assert lib.csm_rotate_histogram(fp(h), -1, 0.1, fp(out)) == csm.CSM_EINVAL
    assert lib.csm_rotate_histogram(fp(h), 8, float("nan"), fp(out)) == csm.CSM_EINVAL
    assert lib.csm_rotate_histogram(None, 0, 0.1, None) == csm.CSM_OK  # empty: returned as is
    # In place.
    want = sup.oracle_rotate_histogram(np.arange(8, dtype=np.float32), 0.7)
    buf = np.arange(8, dtype=np.float32)
    assert lib.csm_rotate_histogram(fp(buf), 8, 0.7, fp(buf)) == csm.CSM_OK
    assert buf.tobytes() == want.tobytes()


def test_header_declares_and_library_exports_new_entries(csm):
    text = open(os.path.join(ROOT, "include", "csm_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(csm_[a-z0-9_]+)\s*\(", text))
    ensure_built()
    lib = C.CDLL(os.path.join(ROOT, "cartographer-1_amd", "libcsm_amd.so"))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in csm._SIGNATURES, name
    assert "csm_inserter3d_options" in text


def test_insert_rejects_bad_arguments_without_a_device(csm):
    """Null pointers, n < 0, probabilities outside (0, 1), a negative
    num_free_space_voxels and non-finite coordinates return CSM_EINVAL before
    the handle is read or anything is enqueued (no device exists here). The
    cases past the null grid pass a handle-sized block of zeros: it must not
    be dereferenced."""
    lib = csm.load_library()
    good = csm.Inserter3DOptions(0.55, 0.49, 2)
    origin = np.zeros(3, np.float32)
    ret = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    ins = lib.csm_hybrid_grid_insert
    assert ins(None, C.byref(good), fp(origin), fp(ret), 2) == csm.CSM_EINVAL
    fake = (C.c_uint8 * 4096)()
    handle = C.cast(fake, C.c_void_p)
    assert ins(handle, None, fp(origin), fp(ret), 2) == csm.CSM_EINVAL
    assert ins(handle, C.byref(good), None, fp(ret), 2) == csm.CSM_EINVAL
    assert ins(handle, C.byref(good), fp(origin), None, 2) == csm.CSM_EINVAL
    assert ins(handle, C.byref(good), fp(origin), fp(ret), -1) == csm.CSM_EINVAL
    for hit, miss, free in [(0.0, 0.49, 2), (1.0, 0.49, 2), (0.55, 0.0, 2), (0.55, 1.0, 2),
                            (-0.1, 0.49, 2), (0.55, 1.5, 2), (float("nan"), 0.49, 2),
                            (0.55, 0.49, -1)]:
        bad = csm.Inserter3DOptions(hit, miss, free)
        rc = ins(handle, C.byref(bad), fp(origin), fp(ret), 2)
        assert rc == csm.CSM_EINVAL, (hit, miss, free)
    for v in (float("nan"), float("inf")):
        r = ret.copy()
        r[1, 2] = v
        assert ins(handle, C.byref(good), fp(origin), fp(r), 2) == csm.CSM_EINVAL
        o = origin.copy()
        o[1] = v
        assert ins(handle, C.byref(good), fp(o), fp(ret), 2) == csm.CSM_EINVAL
    # The batch form and the other handle-free entries.
    batch = lib.csm_hybrid_grid_insert_batch
    handles = (C.c_void_p * 1)(handle)
    off = np.array([0, 2], np.int64)
    zero = np.zeros(1, np.int32)
    ip = zero.ctypes.data_as(C.POINTER(C.c_int32))
    op = off.ctypes.data_as(C.POINTER(C.c_int64))
    assert batch(None, handles, 1, C.byref(good), 1, fp(origin), fp(ret), op, 1, ip, ip, None, 0,
                 None, None) == csm.CSM_EINVAL
    assert batch(handle, None, 1, C.byref(good), 1, fp(origin), fp(ret), op, 1, ip, ip, None, 0,
                 None, None) == csm.CSM_EINVAL
    assert batch(handle, handles, 1, C.byref(good), 1, fp(origin), fp(ret), op, -1, ip, ip, None, 0,
                 None, None) == csm.CSM_EINVAL
    assert batch(handle, handles, 1, C.byref(good), 1, fp(origin), fp(ret), op, 1, None, ip, None,
                 0, None, None) == csm.CSM_EINVAL
    one = np.ones(1, np.int32)
    assert batch(handle, handles, 1, C.byref(good), 1, fp(origin), fp(ret), op, 1,
                 one.ctypes.data_as(C.POINTER(C.c_int32)), ip, None, 0, None,
                 None) == csm.CSM_EINVAL  # grid index out of range
    assert batch(handle, handles, 1, C.byref(good), 1, fp(origin), fp(ret), op, 1, ip, ip, None, 0,
                 one.ctypes.data_as(C.POINTER(C.c_int32)), None) == csm.CSM_EINVAL  # no transform 1
    assert lib.csm_hybrid_grid_read(None, None, 0) == csm.CSM_EINVAL
    assert lib.csm_hybrid_grid_insert_stats(None, None, None) == csm.CSM_EINVAL
