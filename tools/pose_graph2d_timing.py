#!/usr/bin/env python3
"""Times one pose-graph solve on the device (csm_pose_graph2d_solve) and in the
CPU checker of the tests (tests/cpp/pose_graph2d_ref.cc: the same
Levenberg-Marquardt rules with a dense Cholesky solve), on the same problem
(not bench.py; the flagship metric runs none of this code).

The problem is the tests' noisy two-lap walk scaled up: --nodes nodes over
--submaps submaps, two INTRA constraints per node, the chain terms, and
--loops INTER constraints between random pairs, every tenth a gross outlier.
The checker's normal matrix is dense: 3 (nodes + submaps) squared doubles and
a cubic factorisation per iteration, single-threaded, which is what bounds the
size (2000 nodes and 100 submaps take it minutes per solve).

The device solve is warmed up once, then timed --repeats times; a solve ends
in a read-back, so the host clock sees the device. Prints one JSON line: the
device's median, minimum and maximum milliseconds, its host-clock phases
(set-up, linearisations, linear solves, candidate evaluations), the
Levenberg-Marquardt and conjugate-gradient iteration counts, the checker's
seconds and the ratio, and how far apart the two final costs are.

    python tools/pose_graph2d_timing.py [--nodes 600] [--submaps 30] [--loops 4200]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=600)
    ap.add_argument("--submaps", type=int, default=30)
    ap.add_argument("--loops", type=int, default=4200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-checker", action="store_true")
    args = ap.parse_args()

    import pose_graph2d_support as sup
    mod = sup.op2d()
    a = sup.assemble(sup.noisy_graph(args.seed, args.nodes, args.submaps, args.loops))
    mod.pose_graph2d_solve(a.poses, a.constant, a.edges)  # warm-up
    times, phases = [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        out, s = mod.pose_graph2d_solve(a.poses, a.constant, a.edges)
        times.append(1e3 * (time.perf_counter() - t0))
        phases.append(mod.last_phase_seconds())
    mid = sorted(range(len(times)), key=lambda i: times[i])[len(times) // 2]
    result = {
        "vertices": len(a.poses), "edges": len(a.edges),
        "device_ms": {"median": statistics.median(times), "min": min(times), "max": max(times)},
        "device_phase_ms": dict(zip(["setup", "linearise", "linear_solves", "candidates"],
                                    [1e3 * v for v in phases[mid]])),
        "lm_iterations": s.num_iterations, "successful_steps": s.num_successful_steps,
        "cg_iterations": s.num_cg_iterations, "cg_capped_steps": s.num_cg_capped_steps,
        "cg_iterations_per_lm_step": s.num_cg_iterations / max(1, s.num_iterations),
        "termination": s.termination, "final_cost": s.final_cost,
    }
    if not args.no_checker:
        t0 = time.perf_counter()
        ref_poses, rs = sup.ref_solve(a.poses, a.constant, a.edges)
        result["checker_s"] = time.perf_counter() - t0
        result["checker_lm_iterations"] = rs["num_iterations"]
        result["checker_termination"] = rs["termination"]
        result["checker_over_device"] = 1e3 * result["checker_s"] / result["device_ms"]["median"]
        cost_dev = sup.ref_evaluate(out, a.edges)[0]
        result["final_cost_relative_difference"] = abs(cost_dev - rs["final_cost"]) / rs["final_cost"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
