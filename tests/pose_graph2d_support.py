"""Shared by the pose-graph solve tests: the CPU checker
(tests/cpp/pose_graph2d_ref.cc, built with g++ into tests/cpp/_build/ the way
local2d_support.py builds its shim), wrappers over it, the golden SPA case, the
seeded graphs the CPU and GPU tests solve, and the script form the C++ test
program (tests/cpp/optimization_problem_2d_test.cc) reads."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np

from conftest import ROOT, load_package

REF_SRC = os.path.join(ROOT, "tests", "cpp", "pose_graph2d_ref.cc")
REF_LIB = os.path.join(ROOT, "tests", "cpp", "_build", "libpose_graph2d_ref.so")
CPP_SRC = os.path.join(ROOT, "tests", "cpp", "optimization_problem_2d_test.cc")
CPP_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "optimization_problem_2d_test")
GOLDEN = os.path.join(ROOT, "tests", "golden", "spa_cost_2d.json")

D, I32, I64, U8 = C.c_double, C.c_int32, C.c_int64, C.c_uint8
P = C.POINTER

# pose_graph.lua: the constraint builder's loop-closure weights (:25-26), the
# INTRA_SUBMAP weights of trajectory_builder_2d.lua's scan matcher as
# pose_graph_2d.cc:233-245 uses them (:61-62), huber_scale (:65).
LOOP_WEIGHTS = (1.1e4, 1e5)
INTRA_WEIGHTS = (5e2, 1.6e3)
HUBER_SCALE = 10.0

_ref = None


def _p(a, t):
    return a.ctypes.data_as(P(t))


def ref():
    """The compiled checker (once per process). No GPU, no library."""
    global _ref
    if _ref is not None:
        return _ref
    os.makedirs(os.path.dirname(REF_LIB), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Werror",
                           "-ffp-contract=off", REF_SRC, "-o", REF_LIB])
    lib = C.CDLL(REF_LIB)
    lib.pg2ref_evaluate.restype = C.c_int
    lib.pg2ref_evaluate.argtypes = [P(D), I32, C.c_void_p, I64, D, P(D), P(D), P(D), P(D)]
    lib.pg2ref_solve.restype = C.c_int
    lib.pg2ref_solve.argtypes = [P(D), P(U8), I32, C.c_void_p, I64, D, I32, P(D)]
    _ref = lib
    return lib


def op2d():
    """cartographer_amd.optimization_problem_2d (needs the built library to
    import, not a GPU)."""
    import importlib
    load_package()
    return importlib.import_module("cartographer_amd.optimization_problem_2d")


def edges_array(rows):
    return op2d().pose_graph2d_edges(rows)


def ref_evaluate(poses, edges, huber=HUBER_SCALE, jacobians=False):
    """(cost, residuals (E, 3), gradient (V, 3)[, jacobians (E, 18)]) by the checker."""
    p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 3))
    e = np.ascontiguousarray(edges)
    cost = D(0.0)
    r = np.zeros((len(e), 3))
    g = np.zeros((len(p), 3))
    j = np.zeros((len(e), 18)) if jacobians else None
    ref().pg2ref_evaluate(_p(p, D), len(p), e.ctypes.data, len(e), huber, C.byref(cost), _p(r, D),
                          _p(g, D), _p(j, D) if jacobians else None)
    return (cost.value, r, g, j) if jacobians else (cost.value, r, g)


def ref_solve(poses, constant, edges, huber=HUBER_SCALE, max_num_iterations=50):
    """(poses, summary dict) by the checker's dense Levenberg-Marquardt."""
    p = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 3)).copy()
    c = np.ascontiguousarray(np.asarray(constant, np.uint8))
    e = np.ascontiguousarray(edges)
    s = np.zeros(6)
    ref().pg2ref_solve(_p(p, D), _p(c, U8), len(p), e.ctypes.data, len(e), huber,
                       max_num_iterations, _p(s, D))
    return p, {"initial_cost": s[0], "final_cost": s[1], "num_iterations": int(s[2]),
               "num_successful_steps": int(s[3]), "termination": int(s[4]),
               "gradient_max": s[5]}


def golden_spa():
    """The reference's recorded SPA case as (poses, edges, golden dict)."""
    g = json.load(open(GOLDEN))
    yaw = math.atan2(*g["observation_yaw_atan2"])
    poses = np.array([g["start"], g["end"]], np.float64)
    edges = edges_array([(0, 1, (*g["observation_xy"], yaw), g["translation_weight"],
                          g["rotation_weight"], 0)])
    return poses, edges, g


# ---- 2D rigid algebra for the fixtures (double) ----

def compose(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (c * b[0] - s * b[1] + a[0], s * b[0] + c * b[1] + a[1], a[2] + b[2])


def inverse(a):
    c, s = math.cos(-a[2]), math.sin(-a[2])
    return (-(c * a[0] - s * a[1]), -(s * a[0] + c * a[1]), -a[2])


def between(a, b):
    """b seen from a."""
    return compose(inverse(a), b)


class Graph:
    """A problem as the OptimizationProblem2D classes take it: submaps and nodes
    by id with their initial global poses (nodes also their local poses),
    constraints, and the true poses where the fixture knows them."""

    def __init__(self):
        self.submaps = {}      # (t, i) -> global pose
        self.nodes = {}        # (t, i) -> (time, local pose, global pose)
        self.constraints = []  # (submap id, node id, relative pose, tw, rw, tag)
        self.truth_submaps = {}
        self.truth_nodes = {}
        self.frozen = set()

    def fill(self, problem, mod, constraint_type):
        """Loads `problem` (the Python mirror) and returns its constraint list."""
        for s in sorted(self.submaps):
            problem.InsertSubmap(s, self.submaps[s])
        for n in sorted(self.nodes):
            t, local, glob = self.nodes[n]
            problem.InsertTrajectoryNode(n, mod.NodeSpec2D(t, local, glob))
        return [constraint_type(s, n, rel, tw, rw, tag) for s, n, rel, tw, rw, tag in
                self.constraints]

    def states(self, mod):
        return {t: mod.FROZEN for t in self.frozen}

    def script(self, max_num_iterations=None):
        """The same problem for tests/cpp/optimization_problem_2d_test.cc."""
        out = []
        for s in sorted(self.submaps):
            out.append("S %d %d %r %r %r" % (*s, *self.submaps[s]))
        for n in sorted(self.nodes):
            t, local, glob = self.nodes[n]
            out.append("N %d %d %r %r %r %r %r %r %r" % (*n, t, *local, *glob))
        for s, n, rel, tw, rw, tag in self.constraints:
            out.append("C %d %d %d %d %r %r %r %r %r %d" % (*s, *n, *rel, tw, rw,
                                                            1 if tag == "INTER_SUBMAP" else 0))
        for t in sorted(self.frozen):
            out.append("F %d" % t)
        if max_num_iterations is not None:
            out.append("I %d" % max_num_iterations)
        return "\n".join(out) + "\n"


def ring_graph(num_nodes=40, num_submaps=4, radius=5.0, drift=(0.004, -0.003, 0.006)):
    """A closed ring of nodes over submaps with exact constraints: every node
    to its own submap and (past the first submap) to the one before, INTRA; the
    last node to the first submap, INTER: the loop closure. Initial global
    poses are dead reckoning with `drift` composed onto every step; the first
    submap sits at the truth, where the solve keeps it."""
    g = Graph()
    per = num_nodes // num_submaps
    truth = []
    for i in range(num_nodes):
        a = 2.0 * math.pi * i / num_nodes
        truth.append((radius * math.cos(a), radius * math.sin(a), a + math.pi / 2.0))
    init = [truth[0]]
    for i in range(1, num_nodes):
        init.append(compose(init[-1], compose(between(truth[i - 1], truth[i]), drift)))
    for s in range(num_submaps):
        g.submaps[(0, s)] = init[s * per]
        g.truth_submaps[(0, s)] = truth[s * per]
    for i in range(num_nodes):
        # Local SLAM poses: the truth seen from an arbitrary local frame.
        local = compose((0.7, -0.2, 0.3), truth[i])
        g.nodes[(0, i)] = (float(i), local, init[i])
        g.truth_nodes[(0, i)] = truth[i]
        own = i // per
        for s in ([own] if own == 0 else [own - 1, own]):
            g.constraints.append(((0, s), (0, i), between(truth[s * per], truth[i]),
                                  *INTRA_WEIGHTS, "INTRA_SUBMAP"))
    g.constraints.append(((0, 0), (0, num_nodes - 1), between(truth[0], truth[-1]),
                          *LOOP_WEIGHTS, "INTER_SUBMAP"))
    return g


def noisy_graph(seed=7, num_nodes=60, num_submaps=6, num_loops=40, outlier_every=10):
    """A noisy two-lap walk: INTRA constraints and local SLAM poses with small
    noise, `num_loops` INTER constraints between random (submap, node) pairs
    with small noise, every `outlier_every`-th of them a gross outlier (metres
    and radians off), so the Huber loss is active."""
    rng = np.random.RandomState(seed)
    g = Graph()
    per = num_nodes // num_submaps
    truth = []
    for i in range(num_nodes):
        a = 4.0 * math.pi * i / num_nodes
        r = 6.0 + 0.5 * math.sin(3.0 * a)
        truth.append((r * math.cos(a), r * math.sin(a), a + math.pi / 2.0))

    def noisy(rel, sigma_t, sigma_r):
        return (rel[0] + rng.normal(0, sigma_t), rel[1] + rng.normal(0, sigma_t),
                rel[2] + rng.normal(0, sigma_r))

    local = [truth[0]]
    for i in range(1, num_nodes):
        local.append(compose(local[-1], noisy(between(truth[i - 1], truth[i]), 2e-4, 5e-5)))
    for s in range(num_submaps):
        g.submaps[(0, s)] = local[s * per]
    for i in range(num_nodes):
        g.nodes[(0, i)] = (float(i), local[i], local[i])
        own = i // per
        for s in ([own] if own == 0 else [own - 1, own]):
            g.constraints.append(((0, s), (0, i),
                                  noisy(between(truth[s * per], truth[i]), 0.005, 0.002),
                                  *INTRA_WEIGHTS, "INTRA_SUBMAP"))
    for k in range(num_loops):
        s, i = int(rng.randint(num_submaps)), int(rng.randint(num_nodes))
        rel = noisy(between(truth[s * per], truth[i]), 2e-4, 2e-5)
        if k % outlier_every == outlier_every - 1:
            rel = (rel[0] + rng.uniform(2, 4), rel[1] - rng.uniform(2, 4), rel[2] + rng.uniform(1, 2))
        g.constraints.append(((0, s), (0, i), rel, *LOOP_WEIGHTS, "INTER_SUBMAP"))
    return g


def assemble(graph, options=None):
    """The flat problem of `graph` through the Python mirror's Assemble()."""
    mod = op2d()
    cb = __import__("importlib").import_module("cartographer_amd.constraint_builder")
    problem = mod.OptimizationProblem2D(options)
    constraints = graph.fill(problem, mod, cb.Constraint)
    return problem.Assemble(constraints, graph.states(mod))


def truth_array(graph, assembled):
    return np.array([graph.truth_submaps[s] for s in assembled.submap_ids] +
                    [graph.truth_nodes[n] for n in assembled.node_ids], np.float64)


def pose_distance(a, b):
    """Largest translation distance (m) and wrapped angle distance (rad)."""
    a, b = np.asarray(a).reshape(-1, 3), np.asarray(b).reshape(-1, 3)
    dt = np.hypot(a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]).max()
    da = np.abs((a[:, 2] - b[:, 2] + np.pi) % (2.0 * np.pi) - np.pi).max()
    return float(dt), float(da)


def evaluate_fixture(seed, num_vertices, degrees=(), huber=HUBER_SCALE):
    """(poses, edges) for the evaluate tests: `num_vertices` random poses with
    angles up to +-100 rad and some within 1e-9 of +-pi, random edges of both
    losses, Huber edges whose |r|^2 sits below, exactly at and above huber^2,
    an observation whose angle difference wraps, and for vertex k of `degrees`
    exactly degrees[k] incident edges (vertices past len(degrees) get random
    ones). The last vertex has degree 0 unless `degrees` says otherwise."""
    rng = np.random.RandomState(seed)
    V = num_vertices
    poses = np.stack([rng.uniform(-20, 20, V), rng.uniform(-20, 20, V),
                      rng.uniform(-100, 100, V)], 1)
    poses[1 % V, 2] = math.pi - 1e-9
    poses[2 % V, 2] = -math.pi + 1e-9
    poses[3 % V, 2] = 100.0
    rows = []
    first_free = len(degrees)
    poses[first_free + 2] = (0.0, 0.0, 0.0)
    poses[first_free + 3] = (3.0, 0.0, 0.0)

    def edge(a, b, loss=None):
        rel = between(tuple(poses[a]), tuple(poses[b]))
        z = (rel[0] + rng.normal(0, 0.002), rel[1] + rng.normal(0, 0.002),
             rel[2] + rng.normal(0, 0.0002))
        weights = LOOP_WEIGHTS if rng.rand() < 0.5 else INTRA_WEIGHTS
        rows.append((a, b, z, *weights, int(rng.randint(2)) if loss is None else loss))

    # Vertices with an exact degree connect to the free ones only (never the last).
    for k, deg in enumerate(degrees):
        for d in range(deg):
            other = first_free + (k * 131 + d) % max(1, V - 1 - first_free)
            if rng.rand() < 0.5:
                edge(k, other)
            else:
                edge(other, k)
    for _ in range(2 * V):
        a, b = rng.randint(first_free, V - 1, 2)
        if a != b:
            edge(int(a), int(b))
    # Huber edges at chosen |r|: weights 1, the end placed so that the residual
    # is (|r|, 0, 0) up to rounding; and exactly at the scale between two
    # vertices on the x axis with angle 0, where every product is exact.
    a, b = first_free, first_free + 1
    for norm in (0.5 * huber, 0.999999 * huber, 1.000001 * huber, 3.0 * huber):
        rel = between(tuple(poses[a]), tuple(poses[b]))
        rows.append((a, b, (rel[0] + norm, rel[1], rel[2]), 1.0, 1.0, 1))
    rows.append((first_free + 2, first_free + 3, (3.0 + huber, 0.0, 0.0), 1.0, 1.0, 1))
    # An observation whose angle difference leaves (-pi, pi].
    rows.append((a, b, (0.0, 0.0, poses[b, 2] - poses[a, 2] + 3.5), 1.0, 1.0, 0))
    rows.append((b, a, (0.0, 0.0, poses[a, 2] - poses[b, 2] - 3.5), 2.0, 3.0, 1))
    return poses, edges_array(rows)


def build_cpp_test():
    os.makedirs(os.path.dirname(CPP_BIN), exist_ok=True)
    lib = os.path.join(ROOT, "cartographer-1_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "include"), CPP_SRC, "-o", CPP_BIN, "-L", lib,
                           "-lcsm_amd", "-Wl,-rpath," + lib])
    return CPP_BIN


def run_cpp(mode, script, timeout=120):
    return subprocess.run([build_cpp_test(), mode], input=script, capture_output=True, text=True,
                          timeout=timeout, check=True).stdout


def parse_assembled(text):
    """The C++ program's `assemble` output as (poses, constant, edge rows, submap
    ids, node ids)."""
    poses, constant, rows, sids, nids = [], [], [], [], []
    for line in text.splitlines():
        f = line.split()
        if f[0] == "V":
            poses.append([float.fromhex(v) for v in f[1:4]])
            constant.append(int(f[4]))
        elif f[0] == "E":
            z = tuple(float.fromhex(v) for v in f[3:6])
            rows.append((int(f[1]), int(f[2]), z, float.fromhex(f[6]), float.fromhex(f[7]),
                         int(f[8])))
        elif f[0] == "SID":
            sids.append((int(f[1]), int(f[2])))
        elif f[0] == "NID":
            nids.append((int(f[1]), int(f[2])))
    return np.array(poses).reshape(-1, 3), np.array(constant, np.uint8), rows, sids, nids
