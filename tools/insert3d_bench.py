#!/usr/bin/env python3
"""Times 3D range-data insertion into device-resident HybridGrids against the
only route the library offered before it (not bench.py; the flagship metric is
unchanged).

A sensor moves 0.1 m per scan through a 24 x 16 x 4 m room; every scan goes
into the four grids of two active submaps (0.1 m with a 20 m range filter and
0.45 m, each submap with its own submap-from-local transform), then one
RealTimeCorrelativeScanMatcher3D::Match runs on the first submap's 0.1 m grid.

  device  one csm_hybrid_grid_insert_batch (4 grids) + one csm_rt3d_match.
  host    the oracle's RangeDataInserter3D on the CPU for the four grids (the
          transform and the range filter in numpy), the iterator's cell list
          of each changed grid, csm_hybrid_grid_create for each, the same
          match. `host_insert_only` is the CPU insert alone.

Run at two sizes: a voxel-filtered scan (3000 returns) and a C4-sized one
(55000). Also: one insert into a 0.1 m grid that grows the brick against the
same insert repeated (no growth). Every timed window ends in a device
synchronise; each leg is warmed up once and the two sides alternate.

Intensities (`intensity_ms_<n>`): the same four-grid insert without and with
intensity grids on the two 0.1 m grids (csm_hybrid_grid_insert_intensities_batch,
seeded intensities in [0, 255], threshold 200), each window between two
synchronises; and CeresScanMatcher3D on the first submap's grids for 16 poses
around the true one (a 2000-point high-resolution cloud, 500 points low)
without and with the intensity block. Prints one JSON line.

    python tools/insert3d_bench.py [--scans 8] [--repeats 3]
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

HIT, MISS, FREE = 0.55, 0.49, 2
HIGH, LOW, MAX_RANGE = 0.1, 0.45, 20.0
ROOM = np.array([24.0, 16.0, 4.0])


def room_scan(rng, origin, n):
    """n returns where rays from origin meet the walls of the room."""
    d = rng.normal(size=(n, 3)) * [1.0, 1.0, 0.35]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lo, hi = -0.5 * ROOM, 0.5 * ROOM
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, (hi - origin) / d, (lo - origin) / d)
    r = t.min(1, keepdims=True)
    return (origin + d * r + rng.normal(scale=0.01, size=(n, 3))).astype(np.float32)


def rotate(q, v):
    w, x, y, z = [np.float32(c) for c in q]
    qv = np.array([x, y, z], np.float32)
    uv = 2 * np.cross(qv, v)
    return (v + w * uv + np.cross(qv, uv)).astype(np.float32)


def host_job(origin, returns, tf, max_range):
    t, q = tf
    org = rotate(q, origin[None])[0] + np.float32(t)
    ret = rotate(q, returns) + np.float32(t)
    if max_range:
        ret = ret[np.linalg.norm(ret - org, axis=1) <= np.float32(max_range)]
    return org, ret


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import __graft_entry__ as entry
    csm = entry._load_package()
    import oracle_lib
    oracle = oracle_lib.Oracle()
    ctx = csm.default_context(0)
    rt = csm.RealTimeCorrelativeScanMatcher3D(
        csm.RealTimeCorrelativeScanMatcherOptions(0.15, math.radians(1.0), 0.1, 0.1), ctx)
    tfs = [([0.5, -0.25, 0.0], [math.cos(0.15), 0.0, 0.0, math.sin(0.15)]),
           ([-0.5, 0.75, 0.0], [math.cos(-0.4), 0.0, 0.0, math.sin(-0.4)])]
    resolutions = [HIGH, LOW, HIGH, LOW]
    jobs = [(0, 0, tfs[0], MAX_RANGE), (1, 0, tfs[0], None), (2, 0, tfs[1], MAX_RANGE),
            (3, 0, tfs[1], None)]
    empty = np.zeros((0, 3), np.int32), np.zeros(0, np.uint16)
    out = {"scans": args.scans, "repeats": args.repeats}

    for n in (3000, 55000):
        rng = np.random.default_rng(n)
        scans = []
        for s in range(args.scans):
            origin = np.array([0.1 * s - 2.0, 0.05 * s, 0.0], np.float32)
            scans.append((origin, room_scan(rng, origin.astype(np.float64), n)))
        cloud = scans[0][1][:: max(1, n // 200)][:200]
        initial = (tuple(tfs[0][0]), tuple(tfs[0][1]))

        def device():
            grids = [csm.HybridGrid(r, *empty, context=ctx) for r in resolutions]
            t, res = [], []
            for scan in scans:
                t0 = time.perf_counter()
                csm.HybridGrid.insert_batch(grids, [scan], jobs, HIT, MISS, FREE)
                res.append(rt.Match(initial, cloud, grids[0]))
                t.append(time.perf_counter() - t0)
            return t, res, grids

        def host():
            oras = [oracle.hybrid_grid(r) for r in resolutions]
            t, t_ins, res = [], [], []
            for scan in scans:
                t0 = time.perf_counter()
                for g, _, tf, mr in jobs:
                    oras[g].insert(*host_job(scan[0], scan[1], tf, mr), HIT, MISS, FREE)
                t1 = time.perf_counter()
                grids = []
                for o in oras:
                    ijk, v = o.cells()
                    grids.append(csm.HybridGrid(o.resolution, ijk, v, grid_size=o.grid_size,
                                                context=ctx))
                res.append(rt.Match(initial, cloud, grids[0]))
                t.append(time.perf_counter() - t0)
                t_ins.append(t1 - t0)
            return t, t_ins, res

        device()
        dev_t, host_t, host_ins = [], [], []
        for r in range(args.repeats):
            td, rd, grids = device()
            dev_t += td
            if r == 0 or n <= 3000:  # the CPU leg at 55000 is long: one repeat
                th, ti, rh = host()
                host_t += th
                host_ins += ti
        out[f"step_ms_{n}"] = {
            "device": 1e3 * statistics.median(dev_t),
            "device_p90": 1e3 * float(np.percentile(dev_t, 90)),
            "host": 1e3 * statistics.median(host_t),
            "host_insert_only": 1e3 * statistics.median(host_ins),
            "high_brick": list(grids[0].info()[1])}

        def grow_pair():
            g = csm.HybridGrid(HIGH, *empty, context=ctx)
            g.insert(*scans[0], HIT, MISS, FREE)
            far = (scans[0][0] + np.float32([30.0, 0, 0]), scans[0][1] + np.float32([30.0, 0, 0]))
            csm.synchronize(ctx)
            t0 = time.perf_counter()
            g.insert(*far, HIT, MISS, FREE)  # the box doubles along x: a new brick
            csm.synchronize(ctx)
            t1 = time.perf_counter()
            g.insert(*far, HIT, MISS, FREE)  # the same cells again: no growth
            csm.synchronize(ctx)
            return t1 - t0, time.perf_counter() - t1, g.info()[1]

        grow_pair()
        pairs = [grow_pair() for _ in range(max(5, args.repeats))]
        out[f"insert_ms_{n}"] = {"growing": 1e3 * statistics.median(p[0] for p in pairs),
                                 "not_growing": 1e3 * statistics.median(p[1] for p in pairs),
                                 "brick": list(pairs[0][2])}

        vals = [rng.uniform(0.0, 255.0, n).astype(np.float32) for _ in scans]
        ijobs = [(0, 0, tfs[0], MAX_RANGE, 0), (1, 0, tfs[0], None, None),
                 (2, 0, tfs[1], MAX_RANGE, 1), (3, 0, tfs[1], None, None)]

        def insert_leg(with_intensities):
            grids = [csm.HybridGrid(r, *empty, context=ctx) for r in resolutions]
            igrids = [csm.IntensityHybridGrid(HIGH, context=ctx) for _ in range(2)]
            t = []
            for scan, v in zip(scans, vals):
                csm.synchronize(ctx)
                t0 = time.perf_counter()
                if with_intensities:
                    csm.HybridGrid.insert_batch(grids, [scan + (v,)], ijobs, HIT, MISS, FREE,
                                                intensity_grids=igrids, intensity_threshold=200.0)
                else:
                    csm.HybridGrid.insert_batch(grids, [scan], jobs, HIT, MISS, FREE)
                csm.synchronize(ctx)
                t.append(time.perf_counter() - t0)
            return t, grids, igrids

        insert_leg(True)
        plain_t, with_t = [], []
        for r in range(args.repeats):
            plain_t += insert_leg(False)[0]
            tw, grids, igrids = insert_leg(True)
            with_t += tw
        high = scans[-1][1][:: max(1, n // 2000)][:2000]
        node = csm.NodeData3D(high, high[::4], np.zeros(0, np.float32))
        node_vals = vals[-1][:: max(1, n // 2000)][:2000]
        prng = np.random.default_rng(7)
        items = []
        for _ in range(16):
            t = tuple(float(v) for v in np.asarray(tfs[0][0]) + prng.normal(0, 0.03, 3))
            items.append((0, 1, 0, (t, tuple(tfs[0][1])), t))
        copts = csm.CeresOptions3D.make(1.0, 6.0, 5.0, 4e2, 12)  # trajectory_builder_3d.lua:44-60

        def refine_leg(with_block):
            t0 = time.perf_counter()
            if with_block:
                csm.ceres_refine_batch_3d(grids, [node], [it + (0,) for it in items], copts,
                                          intensity_grids=igrids, node_intensities=[node_vals],
                                          intensity_options=(0.5, 0.3, 200.0))
            else:
                csm.ceres_refine_batch_3d(grids, [node], items, copts)
            return time.perf_counter() - t0

        refine_leg(False)
        refine_leg(True)
        ref_plain, ref_with = [], []
        for r in range(max(5, args.repeats)):
            ref_plain.append(refine_leg(False))
            ref_with.append(refine_leg(True))

        def spread(t):
            return {"median": 1e3 * statistics.median(t), "min": 1e3 * min(t), "max": 1e3 * max(t)}

        out[f"intensity_ms_{n}"] = {
            "insert": spread(plain_t), "insert_with_intensities": spread(with_t),
            "refine16": spread(ref_plain), "refine16_with_block": spread(ref_with),
            "intensity_brick": list(igrids[0].info()[1]),
            "intensity_returns": int(igrids[0].read()[1].sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
