#!/usr/bin/env python3
"""Times TSDF range-data insertion into device-resident TSDF2D grids against
the host route it replaces (not bench.py; the flagship metric is unchanged).

1080-beam scans of SyntheticWorld2D, placed in the map frame and moved 5 cm
per step, so a submap grows from 100 x 100 cells as in local SLAM. Inserter
options: trajectory_builder_2d.lua's TSDF defaults (--free-space adds
update_free_space).

  (a) local SLAM step on a growing submap: one insert + one
      csm_rt2d_match_tsdf_grid, against the oracle's inserter on the host
      followed by csm_rt2d_match_tsdf on the changed host planes. Scores and
      poses must be identical at every step.
  (b) insert_batch of 64 submaps x 90 scans against the oracle's inserter on
      one thread, with equal cells.
  (c) the share of a single insert spent in the host plan (sort, normals,
      libm: csm_tsdf_plan_scan alone) against the whole insert, synchronised.

Every timed window ends in a device synchronise (a read-back, a match or
synchronize()); each leg is warmed up once, repeated, and the two sides of a
comparison alternate. Prints one JSON line.

    python tools/tsdf_insert_bench.py [--repeats 3] [--submaps 64] [--scans 90]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

TRUNCATION, MAX_WEIGHT = 0.3, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--submaps", type=int, default=64)
    ap.add_argument("--scans", type=int, default=90)
    ap.add_argument("--free-space", action="store_true")
    args = ap.parse_args()

    import __graft_entry__ as entry
    csm = entry._load_package()
    import oracle_lib
    import tsdf_support as sup
    from insert_bench import initial_limits, submap_scans
    oracle = oracle_lib.Oracle()

    options = sup.OPTION_SETS["B" if args.free_space else "A"]
    copts = csm.TSDFInserterOptions.make(options)
    world = csm.SyntheticWorld2D(num_nodes=max(args.submaps, 8), num_submaps=1, seed=777)
    res = world.resolution
    ctx = csm.default_context(0)
    rt_opts = csm.RealTimeCorrelativeScanMatcherOptions()
    rt = csm.RealTimeCorrelativeScanMatcher2D(rt_opts, ctx)
    rt_host = csm.RealTimeCorrelativeScanMatcher2D(rt_opts, csm.Context(0))
    out = {"beams": int(len(world.cloud(0))), "scans_per_submap": args.scans,
           "repeats": args.repeats, "options": list(options)}

    def new_device(scan):
        return csm.DeviceTSDF2D(*initial_limits(scan, res), TRUNCATION, MAX_WEIGHT, context=ctx)

    def new_oracle(scan):
        return sup.OracleTSDF(oracle, initial_limits(scan, res), TRUNCATION, MAX_WEIGHT)

    # ---- (a) insert + match per step ---------------------------------------
    scans = [(o, r) for o, r, _ in submap_scans(world, 0, args.scans + 1)]
    clouds = [world.cloud(0)] * (args.scans + 1)
    poses = [(float(s[0][0]), float(s[0][1]), float(world.node_poses[0][2])) for s in scans]

    def slam_device():
        grid = new_device(scans[0])
        t, results = [], []
        for i in range(args.scans):
            t0 = time.perf_counter()
            grid.insert(scans[i][0], scans[i][1], copts)
            results.append(rt.Match(poses[i + 1], clouds[i + 1], grid))
            t.append(time.perf_counter() - t0)
        return t, results, grid

    def slam_host():
        ora = new_oracle(scans[0])
        t, results, t_ins = [], [], []
        for i in range(args.scans):
            t0 = time.perf_counter()
            ora.insert(scans[i], options)
            t1 = time.perf_counter()
            (r, mx, my), tsd, wgt = ora.get()  # not timed: the reference's grid is host cells
            host = csm.TSDF2D(r, mx, my, tsd, wgt, float(np.float32(TRUNCATION)), MAX_WEIGHT)
            t2 = time.perf_counter()
            results.append(rt_host.Match(poses[i + 1], clouds[i + 1], host))
            t3 = time.perf_counter()
            t.append((t1 - t0) + (t3 - t2))
            t_ins.append(t1 - t0)
        return t, results, t_ins

    slam_device()
    slam_host()
    dev_t, host_t, host_ins = [], [], []
    same = True
    for _ in range(args.repeats):
        td, rd, grid = slam_device()
        th, rh, ti = slam_host()
        same = same and rd == rh
        dev_t += td
        host_t += th
        host_ins += ti
    out["a_step_ms"] = {"device": 1e3 * statistics.median(dev_t),
                        "host": 1e3 * statistics.median(host_t),
                        "host_insert_only": 1e3 * statistics.median(host_ins),
                        "device_p90": 1e3 * float(np.percentile(dev_t, 90)),
                        "host_p90": 1e3 * float(np.percentile(host_t, 90)),
                        "same_results": bool(same),
                        "final_cells": int(grid.limits().num_x_cells)}

    # ---- (c) host plan share of one insert ---------------------------------
    plan_t, ins_t = [], []
    grid = new_device(scans[0])
    for i in range(args.scans):
        t0 = time.perf_counter()
        csm.tsdf_plan_scan(scans[i][0], scans[i][1], copts)
        t1 = time.perf_counter()
        grid.insert(scans[i][0], scans[i][1], copts)
        csm.synchronize(ctx)
        t2 = time.perf_counter()
        plan_t.append(t1 - t0)
        ins_t.append(t2 - t1)
    out["c_single_insert_ms"] = {
        "host_plan": 1e3 * statistics.median(plan_t),
        "insert_synchronised": 1e3 * statistics.median(ins_t),
        "host_plan_p90": 1e3 * float(np.percentile(plan_t, 90)),
        "insert_p90": 1e3 * float(np.percentile(ins_t, 90)),
        "host_plan_share": statistics.median(plan_t) / statistics.median(ins_t)}

    # ---- (b) batch rebuild --------------------------------------------------
    per_submap = [[(o, r) for o, r, _ in
                   submap_scans(world, g % world.node_poses.shape[0], args.scans)]
                  for g in range(args.submaps)]
    flat, grid_of = [], []
    for i in range(args.scans):
        for g in range(args.submaps):
            flat.append(per_submap[g][i])
            grid_of.append(g)

    def batch_device():
        grids = [new_device(per_submap[g][0]) for g in range(args.submaps)]
        csm.synchronize(ctx)
        t0 = time.perf_counter()
        csm.DeviceTSDF2D.insert_batch(grids, grid_of, flat, copts)
        csm.synchronize(ctx)
        return time.perf_counter() - t0, grids

    def batch_host():
        grids = [new_oracle(per_submap[g][0]) for g in range(args.submaps)]
        t0 = time.perf_counter()
        for g in range(args.submaps):
            for scan in per_submap[g]:
                grids[g].insert(scan, options)
        return time.perf_counter() - t0, grids

    batch_device()
    bd, bh = [], []
    for r in range(args.repeats):
        t, dgrids = batch_device()
        bd.append(t)
        if r < 2:  # the single-thread host leg is long: two repeats
            t, ogrids = batch_host()
            bh.append(t)
    equal = True
    for g in (0, args.submaps - 1):
        host = dgrids[g].to_host()
        _, tsd, wgt = ogrids[g].get()
        equal = equal and np.array_equal(host.tsd_cells, tsd) and \
            np.array_equal(host.weight_cells, wgt)
    n_inserts = args.submaps * args.scans
    out["b_batch_s"] = {"device": statistics.median(bd), "host_one_thread": statistics.median(bh),
                        "device_inserts_per_s": n_inserts / statistics.median(bd),
                        "host_inserts_per_s": n_inserts / statistics.median(bh),
                        "device_all": bd, "host_all": bh, "cells_equal": bool(equal)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
