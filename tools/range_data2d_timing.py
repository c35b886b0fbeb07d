#!/usr/bin/env python3
"""Times one csm_range_data2d_prepare call end to end against the same work
through the entry points that existed before it (not bench.py; the flagship
metric is unchanged).

A 1080-point sweep of a SyntheticWorld2D node, one origin, a pose per point and
trajectory_builder_2d.lua's filter sizes (0.025 m voxels; adaptive 0.5 m, 200
points, 50 m).

  fused:    range_data2d_prepare: one upload, five launches, one download, one
            synchronise.
  separate: the per-point transform, the range test, the alignment and the crop
            in numpy on the host (float32, vectorised; its last bits are not
            checked here), then csm_voxel_filter on the returns and on the
            misses and csm_adaptive_voxel_filter on the filtered returns: three
            uploads, three downloads, three synchronises.

Both sides are warmed up, then alternate; every timed window ends in a device
synchronise inside the call. Prints one JSON line with the median, the minimum
and the maximum of each side in microseconds.

    python tools/range_data2d_timing.py [--repeats 40] [--points 1080]
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


def rotate(q, v):
    """QuaternionBase::_transformVector over rows; q (n, 4) or (4,) as w, x, y, z."""
    u = q[..., 1:]
    uv = np.cross(u, v)
    uv = uv + uv
    return v + q[..., :1] * uv + np.cross(u, uv)


def separate(csm, options, hits, poses, origin, gravity, ctx):
    o = rotate(poses[:, 3:], origin[None, :]) + poses[:, :3]
    h = rotate(poses[:, 3:], hits) + poses[:, :3]
    delta = h - o
    rng = np.sqrt(delta[:, 0] ** 2 + (delta[:, 1] ** 2 + delta[:, 2] ** 2))
    keep = rng >= options.min_range
    ret = keep & (rng <= options.max_range)
    mis = keep & ~ret
    with np.errstate(divide="ignore", invalid="ignore"):
        m = o + (np.float32(options.missing_data_ray_length) / rng)[:, None] * delta
    out = []
    for cloud in (h[ret], m[mis]):
        g = rotate(gravity[3:], cloud) + gravity[:3]
        g = g[(options.min_z <= g[:, 2]) & (g[:, 2] <= options.max_z)]
        out.append(csm.VoxelFilter(g, options.voxel_filter_size, context=ctx))
    out.append(csm.AdaptiveVoxelFilter(out[0], options.adaptive_voxel_filter, context=ctx))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--points", type=int, default=1080)
    args = ap.parse_args()
    import __graft_entry__ as entry
    csm = entry._load_package()
    ctx = csm.default_context()
    world = csm.SyntheticWorld2D(num_nodes=1, num_submaps=1, submap_cells=100,
                                 beams=args.points, seed=77)
    hits = np.ascontiguousarray(world.cloud(0), np.float32)
    n = len(hits)
    rng = np.random.default_rng(1)
    hits[:, 2] = rng.uniform(-0.02, 0.02, n)
    poses = np.zeros((n, 7), np.float32)
    poses[:, :2] = np.linspace(0.0, 0.03, n)[:, None]
    yaw = np.linspace(0.0, 0.005, n)
    poses[:, 3], poses[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    origin = np.zeros(3, np.float32)
    gravity = np.array([0.0, 0.0, 0.0, 0.99995, 0.005, -0.0075, 0.0], np.float32)
    gravity[3:] /= np.linalg.norm(gravity[3:])
    options = csm.RangeData2DOptions.make(max_range=12.0)  # the lua's other defaults
    index = np.zeros(n, np.int32)

    def fused():
        return csm.range_data2d_prepare(options, hits, index, poses, origin[None, :], gravity,
                                        poses[-1, :3], ctx)

    def parted():
        return separate(csm, options, hits, poses, origin, gravity, ctx)

    a, b = fused(), parted()
    sizes = {"fused": [len(x) for x in a[1:]], "separate": [len(x) for x in b]}
    for _ in range(5):
        fused()
        parted()
    t = {"fused": [], "separate": []}
    for _ in range(args.repeats):
        for name, fn in (("fused", fused), ("separate", parted)):
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e6)
    out = {"points": n, "repeats": args.repeats, "sizes": sizes}
    for name, v in t.items():
        out[name + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                             "max": round(max(v), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
