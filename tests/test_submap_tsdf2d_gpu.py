"""GPU: ActiveSubmaps2D with grid_type = TSDF, the Python mirror and the C++
drop-in (include/cartographer_amd/submap_2d.h through
tests/cpp/submap_tsdf_2d_test.cc): the reference's submap bookkeeping
(submap_2d_test.cc:35-96) on TSDF submaps, both active submaps fed through one
batch call, and the first finished submap against the oracle fed the same scans
and cropped; the real-time matcher on the device TSDF."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import tsdf_support as sup

pytestmark = pytest.mark.gpu

CPP_SRC = os.path.join(ROOT, "tests", "cpp", "submap_tsdf_2d_test.cc")
CPP_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "submap_tsdf_2d_test")
K_NUM_RANGE_DATA = 3
RT = (0.1, 20.0 * np.pi / 180.0, 0.1, 0.1)  # RealTimeCorrelativeScanMatcherOptions' defaults


@pytest.fixture(scope="module")
def bin_path(csm):
    os.makedirs(os.path.dirname(CPP_BIN), exist_ok=True)
    libdir = os.path.join(ROOT, "cartographer-1_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), CPP_SRC, "-o", CPP_BIN, "-L", libdir,
                           "-lcsm_amd", "-Wl,-rpath," + libdir])
    return CPP_BIN


@pytest.fixture(scope="module")
def scans():
    return sup.room()[:2 * K_NUM_RANGE_DATA + 1]


@pytest.fixture(scope="module")
def oracle_first_submap(oracle, scans):
    """The oracle fed the first 2 * num_range_data scans with the lua's default
    TSDF options (option set A), then ComputeCroppedGrid."""
    res = float(np.float32(0.05))  # `float resolution` (submap_2d.cc:195)
    origin = scans[0][0]
    half = 0.5 * 100 * res
    ora = sup.OracleTSDF(oracle, (res, float(origin[0]) + half, float(origin[1]) + half, 100, 100))
    for scan in scans[:2 * K_NUM_RANGE_DATA]:
        ora.insert(scan, sup.OPTION_SETS["A"])
    limits, tsd, wgt = ora.get()
    return sup.oracle_crop(limits, tsd, wgt, sup.TRUNCATION, sup.MAX_WEIGHT)


def _match_inputs(scans):
    origin, ret = scans[-1]
    cloud = np.zeros_like(ret)
    cloud[:, :2] = ret[:, :2] - origin[:2]
    return (float(origin[0]) + 0.03, float(origin[1]) - 0.02, 0.01), cloud


def test_python_right_number_of_range_data(csm):
    """submap_2d_test.cc:35-96 with num_range_data = 10 on TSDF submaps."""
    active = csm.ActiveSubmaps2D(10, 0.05, grid_type="TSDF")
    empty = csm.RangeData(np.zeros(3, np.float32), np.zeros((0, 3), np.float32))
    all_submaps = {}
    for _ in range(100):
        insertion_submaps = active.InsertRangeData(empty)
        assert len(insertion_submaps) <= 2
        for s in insertion_submaps:
            assert isinstance(s.tsdf(), csm.DeviceTSDF2D) and s.grid() is None
            all_submaps[id(s)] = s
        if len(active.submaps()) > 1:
            assert 10 <= active.submaps()[0].num_range_data()
    assert len(active.submaps()) == 2
    finished = [s for s in all_submaps.values() if s.num_range_data() == 20]
    rest = [s for s in all_submaps.values() if s.num_range_data() != 20]
    assert len(finished) == len(all_submaps) - 1
    assert all(s.insertion_finished() for s in finished)
    assert len(rest) == 1 and rest[0].num_range_data() == 10


def test_default_grid_type_stays_probability_grid(csm):
    active = csm.ActiveSubmaps2D(10, 0.05)
    active.InsertRangeData(csm.RangeData(np.zeros(3, np.float32), np.zeros((0, 3), np.float32)))
    s = active.submaps()[0]
    assert isinstance(s.grid(), csm.DeviceProbabilityGrid) and s.tsdf() is None
    with pytest.raises(ValueError):
        csm.ActiveSubmaps2D(10, 0.05, grid_type="HYBRID")


def test_python_first_finished_submap_equals_oracle(csm, oracle, scans, oracle_first_submap):
    active = csm.ActiveSubmaps2D(K_NUM_RANGE_DATA, 0.05, grid_type="TSDF")
    first = None
    for origin, ret in scans:
        submaps = active.InsertRangeData(csm.RangeData(origin, ret))
        assert len(submaps) <= 2
        if first is None and submaps[0].insertion_finished():
            first = submaps[0]
    assert first is not None and first.num_range_data() == 2 * K_NUM_RANGE_DATA
    host = first.tsdf().to_host()
    (res, max_x, max_y, nx, ny), tsd, wgt = oracle_first_submap
    assert (host.resolution, host.max_x, host.max_y) == (res, max_x, max_y)
    assert host.tsd_cells.shape == tsd.shape
    assert np.array_equal(host.tsd_cells, tsd) and np.array_equal(host.weight_cells, wgt)
    # The second submap took the scans from num_range_data on in the same batch calls.
    second = next(s for s in active.submaps() if s.num_range_data() == K_NUM_RANGE_DATA + 1)
    origin = scans[K_NUM_RANGE_DATA][0]
    half = 0.5 * 100 * res
    ora = sup.OracleTSDF(oracle, (res, float(origin[0]) + half, float(origin[1]) + half, 100, 100))
    for scan in scans[K_NUM_RANGE_DATA:]:
        ora.insert(scan, sup.OPTION_SETS["A"])
    sup.assert_same_tsdf(second.tsdf(), ora, "second submap")
    # The real-time matcher dispatches on the device TSDF.
    init, cloud = _match_inputs(scans)
    m = csm.RealTimeCorrelativeScanMatcher2D(csm.RealTimeCorrelativeScanMatcherOptions(*RT))
    score, pose = m.Match(init, cloud, first.tsdf())
    assert (score, pose) == m.Match(init, cloud, host)
    ref_score, ref_pose, _ = oracle.rt2d_match_tsdf((res, max_x, max_y), tsd, wgt, sup.TRUNCATION,
                                                    sup.MAX_WEIGHT, RT, init, cloud)
    assert abs(score - ref_score) <= 1e-6 * abs(ref_score) and pose == ref_pose


def test_cpp_right_number_of_range_data(bin_path):
    out = subprocess.run([bin_path, "counts"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_cpp_first_finished_submap_equals_oracle(csm, oracle, bin_path, scans,
                                                 oracle_first_submap, tmp_path):
    path = tmp_path / "scans.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(scans)))
        for origin, ret in scans:
            f.write(np.asarray(origin, "<f4").tobytes())
            f.write(struct.pack("<i", len(ret)))
            f.write(np.ascontiguousarray(ret, "<f4").tobytes())
    out_path = tmp_path / "grid.bin"
    out = subprocess.run([bin_path, "insert", str(path), str(out_path), str(K_NUM_RANGE_DATA)],
                         capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    raw = open(out_path, "rb").read()
    res, max_x, max_y = struct.unpack_from("<3d", raw, 0)
    nx, ny = struct.unpack_from("<2i", raw, 24)
    got_tsd = np.frombuffer(raw, "<u2", count=nx * ny, offset=32).reshape(ny, nx)
    got_wgt = np.frombuffer(raw, "<u2", count=nx * ny, offset=32 + 2 * nx * ny).reshape(ny, nx)
    score, px, py, ptheta = struct.unpack_from("<4d", raw, 32 + 4 * nx * ny)
    (ores, omax_x, omax_y, onx, ony), tsd, wgt = oracle_first_submap
    assert (res, max_x, max_y, nx, ny) == (ores, omax_x, omax_y, onx, ony)
    assert np.array_equal(got_tsd, tsd) and np.array_equal(got_wgt, wgt)
    init, cloud = _match_inputs(scans)
    m = csm.RealTimeCorrelativeScanMatcher2D(csm.RealTimeCorrelativeScanMatcherOptions(*RT))
    host = csm.TSDF2D(res, max_x, max_y, got_tsd, got_wgt, float(np.float32(sup.TRUNCATION)),
                      sup.MAX_WEIGHT)
    assert (score, (px, py, ptheta)) == m.Match(init, cloud, host)
