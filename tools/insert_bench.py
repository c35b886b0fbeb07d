#!/usr/bin/env python3
"""Times range-data insertion into device-resident probability grids against
the host paths it replaces (not bench.py; the flagship metric is unchanged).

1080-beam scans of SyntheticWorld2D, placed in the map frame and moved 5 cm
per step, so a submap grows from 100 x 100 cells as in local SLAM.

  (a) local SLAM step on a growing submap: one insert + one
      csm_rt2d_match_grid, against the oracle's inserter on the host followed
      by csm_rt2d_match on the changed host cells (the whole-grid memcmp, H2D
      and convert it triggers).
  (b) insert_batch of 64 submaps x 90 scans against the oracle's inserter on
      one thread.
  (c) finished device grid -> csm_fast2d_create_from_grid, against read-back +
      csm_fast2d_create.

Every timed window ends in a device synchronise (a read-back, a match or
synchronize()); each leg is warmed up once, repeated, and the two sides of a
comparison alternate. Prints one JSON line.

    python tools/insert_bench.py [--repeats 5] [--submaps 64] [--scans 90]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HIT, MISS = 0.55, 0.49
INITIAL = 100


def scan_at(cloud, pose):
    """(origin, returns, misses) of a node cloud at pose (x, y, theta)."""
    x, y, th = pose
    c, s = np.float32(math.cos(th)), np.float32(math.sin(th))
    ret = np.zeros((len(cloud), 3), np.float32)
    ret[:, 0] = c * cloud[:, 0] - s * cloud[:, 1] + np.float32(x)
    ret[:, 1] = s * cloud[:, 0] + c * cloud[:, 1] + np.float32(y)
    return (np.array([x, y, 0], np.float32), ret, np.zeros((0, 3), np.float32))


def submap_scans(world, node, count):
    x, y, th = world.node_poses[node]
    cloud = world.cloud(node)
    return [scan_at(cloud, (x + 0.05 * i, y + 0.02 * i, th)) for i in range(count)]


def initial_limits(scan, res):
    half = 0.5 * INITIAL * res
    return (res, float(scan[0][0]) + half, float(scan[0][1]) + half, INITIAL, INITIAL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--submaps", type=int, default=64)
    ap.add_argument("--scans", type=int, default=90)
    args = ap.parse_args()

    import __graft_entry__ as entry
    csm = entry._load_package()
    import insert2d_support as sup
    import oracle_lib
    oracle = oracle_lib.Oracle()
    sup.shim()

    world = csm.SyntheticWorld2D(num_nodes=max(args.submaps, 8), num_submaps=1, seed=777)
    res = world.resolution
    ctx = csm.default_context(0)
    rt_opts = csm.RealTimeCorrelativeScanMatcherOptions()
    rt = csm.RealTimeCorrelativeScanMatcher2D(rt_opts, ctx)
    rt_host = csm.RealTimeCorrelativeScanMatcher2D(rt_opts, csm.Context(0))
    out = {"beams": int(len(world.cloud(0))), "scans_per_submap": args.scans,
           "repeats": args.repeats}

    # ---- (a) insert + match per step ---------------------------------------
    scans = submap_scans(world, 0, args.scans + 1)
    clouds = [world.cloud(0)] * (args.scans + 1)
    poses = [(float(s[0][0]), float(s[0][1]), float(world.node_poses[0][2])) for s in scans]

    def slam_device():
        grid = csm.DeviceProbabilityGrid(*initial_limits(scans[0], res), context=ctx)
        t, results = [], []
        for i in range(args.scans):
            t0 = time.perf_counter()
            grid.insert(*scans[i], hit_probability=HIT, miss_probability=MISS)
            results.append(rt.Match(poses[i + 1], clouds[i + 1], grid))
            t.append(time.perf_counter() - t0)
        return t, results, grid

    def slam_host():
        ora = sup.OracleGrid(oracle, initial_limits(scans[0], res))
        t, results, t_ins = [], [], []
        for i in range(args.scans):
            t0 = time.perf_counter()
            ora.insert(scans[i], HIT, MISS, True)
            t1 = time.perf_counter()
            (r, mx, my), cells = ora.get()  # not timed: the reference's grid is already host cells
            host = csm.ProbabilityGrid(r, mx, my, cells)
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

    # ---- (b) batch rebuild --------------------------------------------------
    per_submap = [submap_scans(world, g % world.node_poses.shape[0], args.scans)
                  for g in range(args.submaps)]
    flat, grid_of = [], []
    for i in range(args.scans):
        for g in range(args.submaps):
            flat.append(per_submap[g][i])
            grid_of.append(g)

    def batch_device():
        grids = [csm.DeviceProbabilityGrid(*initial_limits(per_submap[g][0], res), context=ctx)
                 for g in range(args.submaps)]
        csm.synchronize(ctx)
        t0 = time.perf_counter()
        csm.DeviceProbabilityGrid.insert_batch(grids, grid_of, flat, HIT, MISS, True)
        csm.synchronize(ctx)
        return time.perf_counter() - t0, grids

    def batch_host():
        grids = [sup.OracleGrid(oracle, initial_limits(per_submap[g][0], res))
                 for g in range(args.submaps)]
        t0 = time.perf_counter()
        for g in range(args.submaps):
            for scan in per_submap[g]:
                grids[g].insert(scan, HIT, MISS, True)
        return time.perf_counter() - t0, grids

    batch_device()
    bd, bh = [], []
    for r in range(args.repeats):
        t, dgrids = batch_device()
        bd.append(t)
        if r < 2:  # the single-thread host leg is long: two repeats
            t, ogrids = batch_host()
            bh.append(t)
    equal = all(np.array_equal(dgrids[g].to_host().cells, ogrids[g].get()[1])
                for g in (0, args.submaps - 1))
    n_inserts = args.submaps * args.scans
    out["b_batch_s"] = {"device": statistics.median(bd), "host_one_thread": statistics.median(bh),
                        "device_inserts_per_s": n_inserts / statistics.median(bd),
                        "host_inserts_per_s": n_inserts / statistics.median(bh),
                        "device_all": bd, "host_all": bh, "cells_equal": bool(equal)}

    # ---- (c) finished grid -> pyramid --------------------------------------
    grid = dgrids[0]
    grid.finish()
    fopts = csm.FastCorrelativeScanMatcherOptions2D()

    def create_device():
        t0 = time.perf_counter()
        m = csm.FastCorrelativeScanMatcher2D(grid, fopts, ctx)  # returns synchronised
        dt = time.perf_counter() - t0
        m.close()
        return dt

    def create_host():
        t0 = time.perf_counter()
        m = csm.FastCorrelativeScanMatcher2D(grid.to_host(), fopts, ctx)
        dt = time.perf_counter() - t0
        m.close()
        return dt

    create_device()
    create_host()
    cd, ch = [], []
    for _ in range(max(20, args.repeats)):
        cd.append(create_device())
        ch.append(create_host())
    lim = grid.limits()
    out["c_create_ms"] = {"from_grid": 1e3 * statistics.median(cd),
                          "readback_create": 1e3 * statistics.median(ch),
                          "cells": [int(lim.num_x_cells), int(lim.num_y_cells)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
