"""CPU: the host side of TSDF range-data insertion on device grids: the new
C-ABI entries (declared, exported, bound), the argument checks that return
before any handle is read, the per-scan plan (csm_tsdf_plan_scan: ray order,
normals, skip flags) against the oracle, and the converter's round-trip
tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, ensure_built

import tsdf_support as sup

NEW_ENTRIES = [
    "csm_tsdf_grid_create", "csm_tsdf_grid_destroy", "csm_tsdf_grid_limits", "csm_tsdf_grid_read",
    "csm_tsdf_grid_insert", "csm_tsdf_grid_insert_batch", "csm_tsdf_grid_finish",
    "csm_rt2d_match_tsdf_grid", "csm_tsdf_plan_scan", "csm_tsdf_round_trip_tables",
]

OPTION_FIELDS = [
    ("truncation_distance", "double"), ("maximum_weight", "double"),
    ("update_free_space", "int32_t"), ("num_normal_samples", "int32_t"),
    ("sample_radius", "double"), ("project_sdf_distance_to_scan_normal", "int32_t"),
    ("update_weight_range_exponent", "int32_t"),
    ("update_weight_angle_scan_normal_to_ray_kernel_bandwidth", "double"),
    ("update_weight_distance_cell_to_hit_kernel_bandwidth", "double"),
]


def test_header_declares_and_library_exports_new_entries(csm):
    raw = open(os.path.join(ROOT, "include", "csm_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(csm_[a-z0-9_]+)\s*\(", text))
    ensure_built()
    lib = C.CDLL(os.path.join(ROOT, "cartographer-1_amd", "libcsm_amd.so"))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in csm._SIGNATURES, name
    assert "typedef struct csm_tsdf_grid csm_tsdf_grid;" in text
    body = re.search(r"typedef struct csm_tsdf_inserter_options \{(.*?)\}", text, re.S).group(1)
    fields = re.findall(r"(double|int32_t)\s+([a-z_]+);", body)
    assert fields == [(t, n) for n, t in OPTION_FIELDS]
    # The ctypes mirror has the same fields in the same order and types.
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    assert csm.TSDFInserterOptions._fields_ == [(n, ctype[t]) for n, t in OPTION_FIELDS]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_insert_rejects_bad_arguments_without_a_device(csm):
    """A null grid, a non-finite coordinate and bad options return CSM_EINVAL
    before the handle is read or anything is enqueued (no device exists here).
    The handle is a block of zeros: it must not be dereferenced."""
    lib = csm.load_library()
    good = csm.TSDFInserterOptions.make(sup.OPTION_SETS["A"])
    origin = np.zeros(3, np.float32)
    ret = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    assert lib.csm_tsdf_grid_insert(None, C.byref(good), _fp(origin), _fp(ret), 2) == csm.CSM_EINVAL
    fake = (C.c_uint8 * 4096)()
    handle = C.cast(fake, C.c_void_p)
    assert lib.csm_tsdf_grid_insert(handle, None, _fp(origin), _fp(ret), 2) == csm.CSM_EINVAL
    for bad in (float("nan"), float("inf")):
        r = ret.copy()
        r[1, 1] = bad
        assert lib.csm_tsdf_grid_insert(handle, C.byref(good), _fp(origin), _fp(r), 2) == \
            csm.CSM_EINVAL
        o = origin.copy()
        o[0] = bad
        assert lib.csm_tsdf_grid_insert(handle, C.byref(good), _fp(o), _fp(ret), 2) == \
            csm.CSM_EINVAL
    a = sup.OPTION_SETS["A"]
    for opts in ((0.0,) + a[1:], (-0.3,) + a[1:], a[:1] + (0.0,) + a[2:],
                 a[:1] + (-1.0,) + a[2:], a[:3] + (-1,) + a[4:], (float("nan"),) + a[1:]):
        o = csm.TSDFInserterOptions.make(opts)
        assert lib.csm_tsdf_grid_insert(handle, C.byref(o), _fp(origin), _fp(ret), 2) == \
            csm.CSM_EINVAL, opts
        assert lib.csm_tsdf_plan_scan(C.byref(o), _fp(origin), _fp(ret), 2, None, None, None,
                                      None) == csm.CSM_EINVAL, opts
    # The batch entry: the same checks come before any grid handle is read.
    handles = (C.c_void_p * 1)(handle)
    gos = np.zeros(1, np.int32)
    off = np.array([0, 2], np.int64)
    r = ret.copy()
    r[0, 0] = float("nan")
    assert lib.csm_tsdf_grid_insert_batch(
        handle, handles, 1, C.byref(good), 1, gos.ctypes.data_as(C.POINTER(C.c_int32)),
        _fp(origin), _fp(r), off.ctypes.data_as(C.POINTER(C.c_int64))) == csm.CSM_EINVAL
    assert lib.csm_tsdf_grid_insert_batch(None, None, 0, None, 0, None, None, None, None) == \
        csm.CSM_EINVAL
    # The other handle-free entries.
    lim = csm.MapLimits(0.05, 2.5, 2.5, 100, 100)
    out = C.c_void_p()
    cells = np.zeros(100 * 100, np.uint16)
    u16 = cells.ctypes.data_as(C.POINTER(C.c_uint16))
    assert lib.csm_tsdf_grid_create(None, C.byref(lim), 0.3, 10.0, None, None, C.byref(out)) == \
        csm.CSM_EINVAL
    for trunc, max_w in ((0.0, 10.0), (0.3, 0.0), (-1.0, 10.0), (0.3, float("nan"))):
        assert lib.csm_tsdf_grid_create(handle, C.byref(lim), trunc, max_w, None, None,
                                        C.byref(out)) == csm.CSM_EINVAL
    # One cell array alone.
    assert lib.csm_tsdf_grid_create(handle, C.byref(lim), 0.3, 10.0, u16, None, C.byref(out)) == \
        csm.CSM_EINVAL
    assert lib.csm_tsdf_grid_create(handle, C.byref(lim), 0.3, 10.0, None, u16, C.byref(out)) == \
        csm.CSM_EINVAL
    assert lib.csm_tsdf_grid_finish(None) == csm.CSM_EINVAL
    assert lib.csm_tsdf_grid_limits(None, None) == csm.CSM_EINVAL
    assert lib.csm_tsdf_grid_read(None, None, None, 0) == csm.CSM_EINVAL
    lib.csm_tsdf_grid_destroy(None)
    assert lib.csm_rt2d_match_tsdf_grid(None, None, None, None, None, 0, None, None) == \
        csm.CSM_EINVAL
    assert lib.csm_tsdf_round_trip_tables(0.3, 10.0, None, None) == csm.CSM_EINVAL


def _plan_inputs():
    room = sup.room()
    return {"room360": room[0], "room1080": room[7], "growth3": sup.growth()[3],
            "dup": sup.dup()[0], "dup_shuffled": sup.shuffled(sup.dup())[0]}


PLAN_INPUTS = _plan_inputs()


@pytest.mark.parametrize("opt", ["A", "C", "D"])
@pytest.mark.parametrize("name", sorted(PLAN_INPUTS))
def test_plan_scan_against_oracle(csm, oracle, name, opt):
    """The plan of one Insert: `order` is a permutation (the identity when the
    options need no normals) that the RangeDataSorter's comparator finds
    sorted, `normals` are the oracle's EstimateNormals of the returns in that
    order bit for bit, and `cast` is false exactly where range < truncation."""
    origin, returns = PLAN_INPUTS[name]
    options = sup.OPTION_SETS[opt]
    order, normals, weight, cast = csm.tsdf_plan_scan(origin, returns, options)
    n = len(returns)
    assert np.array_equal(np.sort(order), np.arange(n))
    needs_normals = bool(options[5]) or options[7] != 0.0
    sorted_returns = np.ascontiguousarray(returns[order])
    if not needs_normals:
        assert np.array_equal(order, np.arange(n))
        assert np.isnan(normals).all()
    else:
        assert sup.out_of_order(origin, returns, order) == 0
        want = sup.oracle_normals(origin, sorted_returns, int(options[3]), options[4])
        assert np.array_equal(normals.view(np.uint32), want.view(np.uint32))
    # Eigen's 2-vector norm in float (x*x + y*y, sqrt), as InsertHit computes it.
    d = sorted_returns[:, :2] - np.asarray(origin, np.float32)[:2]
    rng = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(cast, ~(rng < np.float32(options[0])))
    assert np.isfinite(weight).all() and (weight >= 0).all()
    if options[6] == 0 and options[7] == 0.0:
        assert (weight == 1.0).all()


def test_plan_scan_marks_short_rays_uncast(csm):
    """Returns nearer than the truncation distance are not cast (:174)."""
    origin = np.zeros(3, np.float32)
    returns = np.array([[0.1, 0.0, 0], [1.0, 0.0, 0], [0.0, 0.29, 0], [0.0, 0.31, 0]], np.float32)
    order, _, _, cast = csm.tsdf_plan_scan(origin, returns, sup.OPTION_SETS["C"])
    assert np.array_equal(order, [0, 1, 2, 3])
    assert cast.tolist() == [False, True, False, True]


@pytest.mark.parametrize("truncation,max_weight", [(0.3, 10.0), (0.2, 10.0), (0.5, 50.0)])
def test_round_trip_tables_equal_oracle(csm, oracle, truncation, max_weight):
    """TSDToValue(ValueToTSD(v)) and WeightToValue(ValueToWeight(v)) for every
    v < 32768 against the oracle converter's. 0 (unknown) maps to 1."""
    tsd, wgt = csm.tsdf_round_trip_tables(truncation, max_weight)
    want_tsd, want_wgt = sup.oracle_round_trip(truncation, max_weight)
    assert np.array_equal(tsd, want_tsd)
    assert np.array_equal(wgt, want_wgt)
    assert tsd[0] == 1 and wgt[0] == 1
