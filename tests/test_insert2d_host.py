"""CPU: the host side of range-data insertion on device grids: the update
lookup tables against the oracle's, the new C-ABI entries (declared, exported,
bound), and the argument checks that return before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, ensure_built

import insert2d_support as sup

NEW_ENTRIES = [
    "csm_probability_grid_create", "csm_probability_grid_destroy", "csm_probability_grid_limits",
    "csm_probability_grid_read", "csm_probability_grid_insert",
    "csm_probability_grid_insert_batch", "csm_probability_grid_finish",
    "csm_fast2d_create_from_grid", "csm_rt2d_match_grid", "csm_ray_to_pixel_mask",
    "csm_inserter2d_lookup_table",
]


@pytest.mark.parametrize("p", [0.55, 0.7, 0.4, 0.49, 0.9])
def test_lookup_table_equals_oracle(csm, oracle, p):
    """ComputeLookupTableToApplyCorrespondenceCostOdds(Odds(p)), all 32768
    entries with the update marker, against the oracle's table."""
    got = csm.inserter2d_lookup_table(p)
    want = sup.oracle_table(p)
    assert got.dtype == np.uint16 and got.shape == (32768,)
    assert np.array_equal(got, want)
    assert (got >= 32768).all()  # every entry carries the marker


def test_lookup_table_rejects_bad_probability(csm):
    lib = csm.load_library()
    out = np.zeros(32768, np.uint16)
    ptr = out.ctypes.data_as(C.POINTER(C.c_uint16))
    for p in (0.0, 1.0, -0.5, float("nan")):
        assert lib.csm_inserter2d_lookup_table(p, ptr) == csm.CSM_EINVAL
    assert lib.csm_inserter2d_lookup_table(0.5, None) == csm.CSM_EINVAL


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
    assert "typedef struct csm_probability_grid csm_probability_grid;" in text
    assert "csm_inserter2d_options" in text


def test_insert_rejects_null_grid_and_nan_without_a_device(csm):
    """A null grid and a non-finite coordinate return CSM_EINVAL before the
    handle is read or anything is enqueued (no device exists here). The NaN
    case passes a handle-sized block of zeros: it must not be dereferenced."""
    lib = csm.load_library()
    opts = csm.Inserter2DOptions(0.55, 0.49, 1)
    origin = np.zeros(3, np.float32)
    ret = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert lib.csm_probability_grid_insert(None, C.byref(opts), fp(origin), fp(ret), 2, None,
                                           0) == csm.CSM_EINVAL
    fake = (C.c_uint8 * 4096)()
    handle = C.cast(fake, C.c_void_p)
    for bad in (float("nan"), float("inf")):
        r = ret.copy()
        r[1, 1] = bad
        assert lib.csm_probability_grid_insert(handle, C.byref(opts), fp(origin), fp(r), 2, None,
                                               0) == csm.CSM_EINVAL
        o = origin.copy()
        o[0] = bad
        assert lib.csm_probability_grid_insert(handle, C.byref(opts), fp(o), fp(ret), 2, None,
                                               0) == csm.CSM_EINVAL
        assert lib.csm_probability_grid_insert(handle, C.byref(opts), fp(origin), fp(ret), 2,
                                               fp(r), 2) == csm.CSM_EINVAL
    # The other handle-free entries.
    assert lib.csm_probability_grid_finish(None) == csm.CSM_EINVAL
    assert lib.csm_probability_grid_limits(None, None) == csm.CSM_EINVAL
    assert lib.csm_probability_grid_read(None, None, 0) == csm.CSM_EINVAL
    lib.csm_probability_grid_destroy(None)
    assert lib.csm_fast2d_create_from_grid(None, None, None, None) == csm.CSM_EINVAL
    assert lib.csm_rt2d_match_grid(None, None, None, None, None, 0, None, None) == csm.CSM_EINVAL
    assert lib.csm_ray_to_pixel_mask(None, None, 0, 1000, None, 0, None) == csm.CSM_EINVAL
