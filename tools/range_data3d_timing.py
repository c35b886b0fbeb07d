#!/usr/bin/env python3
"""Times csm_range_data3d_prepare and csm_voxel_filter_large end to end (not
bench.py; the flagship metric is unchanged).

  prepare:  range_data3d_prepare with trajectory_builder_3d.lua's defaults on a
            16 000-point sweep (the size of the reference's
            LocalTrajectoryBuilderTest scan) and on a 65 536-point sweep of a
            room, a pose per point, three origins, with intensities.
  filter:   voxel_filter_large_mask alone at 8193, 65 536 and 2^20 points,
            0.15 m voxels.
  cpu:      for context, the CPU restatement of the same prepare inputs
            (tests/cpp/oracle_local3d_shim.cc over the oracle) on one thread
            of the same machine.

Each call goes through the Python wrapper and ends in the device synchronise
inside the call. After a warm-up, the median, the minimum and the maximum of
--repeats calls in microseconds, as one JSON line.

    python tools/range_data3d_timing.py [--repeats 40]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median": round(statistics.median(t), 1), "min": round(min(t), 1),
            "max": round(max(t), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement")
    args = ap.parse_args()
    import __graft_entry__ as entry
    csm = entry._load_package()
    import local3d_support as sup
    ctx = csm.default_context()
    options = csm.RangeData3DOptions.make()
    pose = ((1.25, -0.5, 0.3), sup.quat_from_rpy(0.02, -0.03, 0.7))
    tfl, lo = sup.tracking_from_local(pose)
    out = {"repeats": args.repeats, "prepare": {}, "filter": {}}
    for n in (16000, 65536):
        hits, idx, poses, inten = sup.sweep_inputs(n, 900 + n % 7)

        def prepare():
            return csm.range_data3d_prepare(options, hits, idx, poses, sup.ORIGINS, tfl, lo,
                                            intensities=inten, context=ctx)

        got = prepare()
        entry_out = {"sizes": {k: len(got[k]) for k in ("returns", "misses", "high", "low")},
                     "gpu_us": timed(prepare, args.repeats)}
        if not args.no_cpu:
            def restated():
                return sup.prepare(options, hits, idx, poses, sup.ORIGINS, tfl, lo,
                                   intensities=inten)

            entry_out["adaptive_passes"] = restated()["passes"]
            entry_out["cpu_us"] = timed(restated, args.repeats)
        out["prepare"][str(n)] = entry_out
    for n in (8193, 65536, 2**20):
        cloud = sup.cloud3d(n, 7, 40.0)
        out["filter"][str(n)] = timed(
            lambda: csm.voxel_filter_large_mask(cloud, 0.15, ctx), args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
