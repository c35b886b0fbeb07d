"""GPU: csm_pose_graph2d_evaluate and csm_pose_graph2d_solve against the CPU
checker (tests/cpp/pose_graph2d_ref.cc: the same cost and Levenberg-Marquardt
rules with a dense Cholesky solve), the reference's recorded SPA numbers, and
the OptimizationProblem2D classes of both languages. Every figure a test
bounds is printed before it is asserted (pytest -s shows them)."""
import importlib
import math

import numpy as np
import pytest

import pose_graph2d_support as sup

pytestmark = pytest.mark.gpu

# Largest deviation of the device's evaluate from the checker over the three
# fixtures below, measured on an MI355X (ROCm 7 device sin/cos against glibc's):
# a residual relative to w (|z| + |dx| + |dy|) (angles: w (|z| + |start| + |end|)),
# a gradient entry relative to the summed magnitudes of its terms. The tests
# assert 8 x these, because the fixtures are few.
EVAL_RESIDUAL_DEVIATION = 1.26e-16  # 1.035e-16, 1.132e-16, 1.255e-16 on the three fixtures
EVAL_GRADIENT_DEVIATION = 4.54e-12  # 9.747e-13, 4.535e-12, 1.956e-12
EVAL_MARGIN = 8.0

# Loop-closure ring: the device must come as close to the truth as the checker
# does on the same input, times this. Both stop under the same parameter
# tolerance after the same Levenberg-Marquardt steps; they differ by the
# conjugate-gradient solve's 1e-8 relative residual per step, which the
# damping of the next step (error / radius, radius >= 1e4) dwarfs. 4 leaves
# room for that and for sin/cos differing in the last bit.
RING_MARGIN = 4.0

# Noisy graph: |cost(device poses) - cost(checker poses)| / cost, both costs by
# the checker, and max |gradient| at the device's poses over the checker's.
# Measured on an MI355X: 2.405e-15 and 1.000000 (both solvers take the same
# four iterations). The cost assert is 8 x the measured difference plus the
# rounding of the checker's two sums of E terms, under the hard cap; the
# gradient assert is the measured ratio plus a tenth.
NOISY_COST_CAP = 1e-5
NOISY_COST_DIFFERENCE = 2.41e-15
NOISY_GRADIENT_RATIO = 1.0


@pytest.fixture(scope="module")
def mod(csm):
    return sup.op2d()


@pytest.fixture(scope="module")
def cb(csm):
    return importlib.import_module("cartographer_amd.constraint_builder")


@pytest.fixture(scope="module")
def ring():
    graph = sup.ring_graph()
    a = sup.assemble(graph)
    ref_poses, ref_summary = sup.ref_solve(a.poses, a.constant, a.edges)
    return graph, a, sup.truth_array(graph, a), ref_poses, ref_summary


@pytest.fixture(scope="module")
def noisy():
    a = sup.assemble(sup.noisy_graph())
    ref_poses, ref_summary = sup.ref_solve(a.poses, a.constant, a.edges)
    return a, ref_poses, ref_summary


EVAL_CASES = {
    # Vertex counts around the 256-thread workgroup; vertex degrees around the
    # 64 lanes of a row's wave (vertices 0..5), the last vertex with no edge.
    "v255_degrees": (11, 255, (0, 1, 63, 64, 65, 129)),
    "v256": (12, 256, ()),
    "v257": (13, 257, (129, 65)),
}


def _deviation(poses, edges, dev, ref, huber=sup.HUBER_SCALE):
    """(largest residual deviation, largest gradient deviation), relative as the
    constants above say."""
    _, r_dev, g_dev = dev
    _, r_ref, g_ref, jac = ref
    ps, pt = poses[edges["start"]], poses[edges["end"]]
    span = np.abs(pt[:, 0] - ps[:, 0]) + np.abs(pt[:, 1] - ps[:, 1])
    z = np.abs(edges["zbar"])
    wt, wr = np.abs(edges["translation_weight"]), np.abs(edges["rotation_weight"])
    scale_r = np.stack([wt * (z[:, 0] + span), wt * (z[:, 1] + span),
                        wr * (z[:, 2] + np.abs(ps[:, 2]) + np.abs(pt[:, 2]))], 1)
    diff_r = np.abs(r_dev - r_ref)
    assert np.all(diff_r[scale_r == 0] == 0)  # all-zero ingredients: an exact zero
    res = float((diff_r[scale_r > 0] / scale_r[scale_r > 0]).max())
    sq = (r_ref ** 2).sum(1)
    rho1 = np.where((edges["loss"] == 1) & (sq > huber * huber),
                    huber / np.sqrt(np.maximum(sq, 1e-300)), 1.0)
    scale_g = np.zeros_like(g_ref)
    for side, col in ((0, "start"), (1, "end")):
        block = np.abs(jac[:, 9 * side:9 * side + 9].reshape(-1, 3, 3))  # [edge][row][column]
        terms = (block * np.abs(r_ref)[:, :, None]).sum(1) * rho1[:, None]
        np.add.at(scale_g, edges[col], terms)
    diff = np.abs(g_dev - g_ref)
    assert np.all(diff[scale_g == 0] == 0)  # a vertex without edges has a zero gradient
    grad = float((diff[scale_g > 0] / scale_g[scale_g > 0]).max())
    # d cost = sum rho' r dr: what a residual deviation of 1 (relative) may move the cost by.
    cost_scale = float(((np.abs(r_ref) * scale_r).sum(1) * rho1).sum())
    return res, grad, cost_scale


@pytest.mark.parametrize("name", sorted(EVAL_CASES))
def test_evaluate_matches_the_checker(csm, mod, name):
    seed, V, degrees = EVAL_CASES[name]
    poses, edges = sup.evaluate_fixture(seed, V, degrees)
    degree = np.bincount(np.concatenate([edges["start"], edges["end"]]), minlength=V)
    assert degree[:len(degrees)].tolist() == list(degrees) and degree[-1] == 0
    ref = sup.ref_evaluate(poses, edges, jacobians=True)
    dev = mod.pose_graph2d_evaluate(poses, edges)
    res, grad, cost_scale = _deviation(poses, edges, dev, ref)
    cost = abs(dev[0] - ref[0])
    print(f"evaluate {name}: V={V} E={len(edges)} residual deviation {res:.3e} "
          f"gradient deviation {grad:.3e} cost difference {cost:.3e} of {ref[0]:.6e}, "
          f"cost scale {cost_scale:.3e}")
    assert res <= EVAL_MARGIN * EVAL_RESIDUAL_DEVIATION
    assert grad <= EVAL_MARGIN * EVAL_GRADIENT_DEVIATION
    # First order in the residual deviation, plus the rounding of two sums of E
    # positive terms in different orders.
    assert cost <= EVAL_MARGIN * EVAL_RESIDUAL_DEVIATION * cost_scale + \
        len(edges) * 2.0 ** -52 * ref[0]


def test_evaluate_meets_the_reference_spa_numbers(csm, mod):
    """spa_cost_function_2d_test.cc:109-126 at its own 1e-5: the residuals, and
    the gradient J'r from the recorded Jacobian blocks."""
    poses, edges, g = sup.golden_spa()
    cost, r, grad = mod.pose_graph2d_evaluate(poses, edges)
    print("golden residuals", r[0].tolist(), "gradient", grad.reshape(-1).tolist())
    assert np.abs(r[0] - g["residuals"]).max() <= g["tolerance"]
    want = np.asarray(g["residuals"])
    js = np.asarray(g["jacobian_start"]).reshape(3, 3)
    je = np.asarray(g["jacobian_end"]).reshape(3, 3)
    # Every recorded number is within 1e-5, so a gradient entry sum_i J_ij r_i is
    # within 1e-5 (sum |J_ij| + sum |r_i|) + 3e-10.
    bound = 1e-5 * (np.abs(np.concatenate([js, je], 1)).sum(0) + np.abs(want).sum()) + 3e-10
    got = grad.reshape(-1)
    assert np.all(np.abs(got - np.concatenate([js.T @ want, je.T @ want])) <= bound)
    assert cost == pytest.approx(0.5 * float(want @ want), abs=1e-5 * np.abs(want).sum() + 1e-9)


def test_one_edge_ends_at_submap_times_observation(csm, mod):
    """One constant submap, one node, one exact-able edge: the node ends at
    submap * zbar. A second node without edges comes back as it went in."""
    submap, z = (1.5, -2.0, 0.7), (0.8, 0.3, -0.4)
    poses = np.array([submap, (0.0, 0.0, 0.0), (4.0, 5.0, 6.0)])
    edges = sup.edges_array([(0, 1, z, *sup.LOOP_WEIGHTS, 1)])
    out, s = mod.pose_graph2d_solve(poses, [1, 0, 0], edges)
    want = sup.compose(submap, z)
    dt, da = sup.pose_distance(out[1], want)
    print("one edge:", out[1].tolist(), "want", want, "distance", dt, da, "iterations",
          s.num_iterations, "termination", s.termination, "final cost", s.final_cost)
    # The solve stops once a step is below 1e-8 (|x| + 1e-8), |x| about 2: what
    # is left is that step at most, and the damping's share of the step before.
    assert dt <= 1e-6 and da <= 1e-6
    # The cost those distances allow: 1/2 (wt^2 (dx^2 + dy^2) + wr^2 da^2).
    assert s.final_cost <= 0.5 * (sup.LOOP_WEIGHTS[0] ** 2 + sup.LOOP_WEIGHTS[1] ** 2) * 1e-12
    assert s.termination in mod.CONVERGED and s.initial_cost > 1.0
    assert out[0].tobytes() == poses[0].tobytes()
    assert out[2].tobytes() == poses[2].tobytes() and np.all(np.isfinite(out))


def test_ring_loop_closure_returns_the_truth(csm, mod, ring):
    graph, a, truth, ref_poses, ref_summary = ring
    assert ref_summary["termination"] in (0, 1, 2) and ref_summary["num_iterations"] < 50
    ref_dt, ref_da = sup.pose_distance(ref_poses, truth)
    out, s = mod.pose_graph2d_solve(a.poses, a.constant, a.edges)
    dt, da = sup.pose_distance(out, truth)
    print(f"ring: device distance {dt:.3e} m {da:.3e} rad, checker {ref_dt:.3e} m {ref_da:.3e} rad; "
          f"device cost {s.initial_cost:.6e} -> {s.final_cost:.3e} in {s.num_iterations} iterations "
          f"({s.num_successful_steps} accepted, {s.num_cg_iterations} CG iterations, "
          f"{s.num_cg_capped_steps} capped), termination {s.termination}; checker {ref_summary}")
    assert dt <= RING_MARGIN * ref_dt and da <= RING_MARGIN * ref_da
    assert s.termination in mod.CONVERGED
    # The cost is quadratic in the distance from the truth, where it is zero.
    assert s.final_cost <= RING_MARGIN ** 2 * ref_summary["final_cost"]
    assert s.initial_cost == pytest.approx(ref_summary["initial_cost"], rel=1e-12)
    assert out[0].tobytes() == a.poses[0].tobytes()


def test_noisy_graph_with_outliers_agrees_with_the_checker(csm, mod, noisy):
    a, ref_poses, ref_summary = noisy
    assert ref_summary["termination"] in (0, 1, 2)
    out, s = mod.pose_graph2d_solve(a.poses, a.constant, a.edges)
    cost_dev, _, g_dev = sup.ref_evaluate(out, a.edges)
    cost_ref, _, g_ref = sup.ref_evaluate(ref_poses, a.edges)
    free = a.constant == 0
    gmax_dev, gmax_ref = np.abs(g_dev[free]).max(), np.abs(g_ref[free]).max()
    rel = abs(cost_dev - cost_ref) / cost_ref
    print(f"noisy: checker cost at device poses {cost_dev!r}, at checker poses {cost_ref!r}, "
          f"relative difference {rel:.3e}; max |gradient| device {gmax_dev:.6e} checker "
          f"{gmax_ref:.6e} ratio {gmax_dev / gmax_ref:.6f}; device summary cost "
          f"{s.initial_cost!r} -> {s.final_cost!r}, {s.num_iterations} iterations, "
          f"{s.num_cg_iterations} CG iterations, termination {s.termination}; checker {ref_summary}")
    assert rel <= min(NOISY_COST_CAP, 8 * NOISY_COST_DIFFERENCE + 2 * len(a.edges) * 2.0 ** -52)
    assert gmax_dev <= (NOISY_GRADIENT_RATIO + 0.1) * gmax_ref
    assert s.termination in mod.CONVERGED
    assert s.final_cost == pytest.approx(cost_dev, rel=1e-9)


def test_constant_vertices_keep_their_bits(csm, mod, noisy):
    a = noisy[0]
    constant = a.constant.copy()
    constant[[3, 17, 40]] = 1
    out, _ = mod.pose_graph2d_solve(a.poses, constant, a.edges)
    held = constant == 1
    assert out[held].tobytes() == a.poses[held].tobytes()
    assert not np.array_equal(out[~held], a.poses[~held])


def test_edge_between_constant_vertices_adds_cost_only(csm, mod, ring):
    _, a, _, _, _ = ring
    constant = a.constant.copy()
    constant[1] = 1  # a second submap held: vertices 0 and 1 are constant
    extra = sup.edges_array([(0, 1, (9.0, -9.0, 1.0), 3.0, 4.0, 0)])
    base, s0 = mod.pose_graph2d_solve(a.poses, constant, a.edges)
    more, s1 = mod.pose_graph2d_solve(a.poses, constant, np.concatenate([a.edges, extra]))
    only = sup.ref_evaluate(a.poses, extra)[0]
    print("constant edge: cost", only, "final", s0.final_cost, s1.final_cost)
    assert more.tobytes() == base.tobytes()
    assert (s1.num_iterations, s1.termination) == (s0.num_iterations, s0.termination)
    assert s1.initial_cost - s0.initial_cost == pytest.approx(only, rel=1e-9)
    assert s1.final_cost - s0.final_cost == pytest.approx(only, rel=1e-9)


def test_frozen_trajectory_stays_put(csm, mod, cb):
    """Trajectory 1, frozen, holds the ring's truth; trajectory 0 a drifted
    copy of three nodes tied to trajectory 1's submap. Solve() moves
    trajectory 0 only."""
    ring = sup.ring_graph()
    problem = mod.OptimizationProblem2D()
    problem.InsertSubmap((0, 0), (0.0, 0.0, 0.0))
    for s, pose in ring.truth_submaps.items():
        problem.InsertSubmap((1, s[1]), pose)
    for n, pose in ring.truth_nodes.items():
        problem.InsertTrajectoryNode((1, n[1]), mod.NodeSpec2D(float(n[1]), pose, pose))
    constraints = []
    for i in range(3):
        truth = ring.truth_nodes[(0, i)]
        problem.InsertTrajectoryNode((0, i), mod.NodeSpec2D(
            float(i), truth, sup.compose(truth, (0.05 * i, 0.02, 0.01 * i))))
        constraints.append(cb.Constraint((1, 0), (0, i), sup.between(ring.truth_submaps[(0, 0)], truth),
                                         *sup.LOOP_WEIGHTS, "INTER_SUBMAP"))
    before_nodes = {n: d.global_pose_2d for n, d in problem.node_data().items()}
    before_submaps = {s: d.global_pose for s, d in problem.submap_data().items()}
    summary = problem.Solve(constraints, {1: mod.FROZEN})
    assert summary.termination in mod.CONVERGED
    for n, d in problem.node_data().items():
        if n[0] == 1:
            assert d.global_pose_2d == before_nodes[n]
        else:
            dt, da = sup.pose_distance(d.global_pose_2d, ring.truth_nodes[(0, n[1])])
            assert dt <= 1e-6 and da <= 1e-6
    assert {s: d.global_pose for s, d in problem.submap_data().items()} == before_submaps


def test_one_iteration_reports_no_convergence(csm, mod, ring):
    _, a, _, _, _ = ring
    out, s = mod.pose_graph2d_solve(a.poses, a.constant, a.edges, max_num_iterations=1)
    assert (s.num_iterations, s.termination) == (1, mod.NO_CONVERGENCE)
    assert s.final_cost < s.initial_cost and s.num_successful_steps == 1


def test_two_cg_iterations_still_return(csm, mod, ring):
    _, a, _, _, _ = ring
    out, s = mod.pose_graph2d_solve(a.poses, a.constant, a.edges, max_cg_iterations=2)
    print("cg cap 2:", s.initial_cost, "->", s.final_cost, s.num_iterations, "iterations",
          s.num_cg_iterations, "CG iterations", s.num_cg_capped_steps, "capped, termination",
          s.termination)
    assert s.num_cg_capped_steps >= 1 and s.num_cg_iterations <= 2 * s.num_iterations
    assert s.final_cost <= s.initial_cost and np.all(np.isfinite(out))
    assert sup.ref_evaluate(out, a.edges)[0] == pytest.approx(s.final_cost, rel=1e-9)


def test_component_without_a_constant_vertex_terminates(csm, mod, ring):
    """The ring, and a second copy of its nodes shifted away with no constant
    vertex: that copy can move as a whole (gauge freedom)."""
    _, a, _, _, _ = ring
    V = len(a.poses)
    poses = np.concatenate([a.poses, a.poses[4:] + (50.0, 0.0, 0.0)])
    chain = a.edges[(a.edges["start"] >= 4) & (a.edges["end"] >= 4)].copy()
    chain["start"] += V - 4
    chain["end"] += V - 4
    constant = np.concatenate([a.constant, np.zeros(V - 4, np.uint8)])
    edges = np.concatenate([a.edges, chain])
    out, s = mod.pose_graph2d_solve(poses, constant, edges)
    print("gauge:", s.initial_cost, "->", s.final_cost, s.num_iterations, "iterations, termination",
          s.termination)
    assert np.all(np.isfinite(out)) and s.final_cost <= s.initial_cost
    assert s.termination in (mod.CONVERGED + (mod.NO_CONVERGENCE, mod.FAILURE))
    assert s.num_iterations <= 50


def test_nonmonotonic_steps_return_the_cheapest_point(csm, mod, noisy, ring):
    """use_nonmonotonic_steps: the reported final cost is the cost of the poses
    that come back (the checker's evaluation of them), never above the start."""
    for a in (noisy[0], ring[1]):
        out, s = mod.pose_graph2d_solve(a.poses, a.constant, a.edges, use_nonmonotonic_steps=True)
        print("nonmonotonic:", s.initial_cost, "->", s.final_cost, s.num_iterations, "iterations",
              s.num_successful_steps, "accepted, termination", s.termination)
        assert s.termination in mod.CONVERGED and s.final_cost <= s.initial_cost
        # Absolute: the ring ends at a cost near 1e-7 whose residuals are what
        # cancellation leaves, each uncertain by about eps w (|z| + |dx| + |dy|)
        # = 1e-9; against sum |r| <= sqrt(E 2 cost) = 5e-3 that moves the cost
        # by 5e-12 at most.
        assert sup.ref_evaluate(out, a.edges)[0] == pytest.approx(s.final_cost, rel=1e-9, abs=1e-11)


def test_two_solves_return_identical_bytes(csm, mod, noisy):
    a = noisy[0]
    first, s1 = mod.pose_graph2d_solve(a.poses, a.constant, a.edges)
    second, s2 = mod.pose_graph2d_solve(a.poses, a.constant, a.edges)
    assert first.tobytes() == second.tobytes()
    assert bytes(s1) == bytes(s2)


def test_errors_and_empty_problems(csm, mod, ring):
    _, a, _, _, _ = ring
    bad = a.poses.copy()
    bad[5, 1] = np.nan
    with pytest.raises(csm.CsmError, match=r"\(-1\)"):
        mod.pose_graph2d_solve(bad, a.constant, a.edges)
    with pytest.raises(csm.CsmError, match=r"\(-1\)"):
        mod.pose_graph2d_evaluate(bad, a.edges)
    for field, value in (("start", len(a.poses)), ("end", -1)):
        edges = a.edges.copy()
        edges[7][field] = value
        with pytest.raises(csm.CsmError, match=r"\(-1\)"):
            mod.pose_graph2d_solve(a.poses, a.constant, edges)
    edges = a.edges.copy()
    edges[7]["end"] = edges[7]["start"]
    with pytest.raises(csm.CsmError, match=r"\(-1\)"):
        mod.pose_graph2d_solve(a.poses, a.constant, edges)
    edges = a.edges.copy()
    edges[2]["rotation_weight"] = math.inf
    with pytest.raises(csm.CsmError, match=r"\(-1\)"):
        mod.pose_graph2d_solve(a.poses, a.constant, edges)
    with pytest.raises(csm.CsmError, match=r"\(-4\)"):
        mod.pose_graph2d_solve(np.zeros(((1 << 22) + 1, 3)), None, a.edges)
    # No edges, and every vertex constant: the poses stay, nothing is solved.
    out, s = mod.pose_graph2d_solve(a.poses, a.constant, a.edges[:0])
    assert out.tobytes() == a.poses.tobytes() and s.num_iterations == 0
    assert s.termination in mod.CONVERGED
    out, s = mod.pose_graph2d_solve(a.poses, np.ones(len(a.poses), np.uint8), a.edges)
    assert out.tobytes() == a.poses.tobytes() and s.num_iterations == 0
    assert s.termination in mod.CONVERGED


def test_cpp_solve_and_python_mirror_return_the_same_bits(csm, mod, cb, ring):
    graph, a, truth, _, _ = ring
    problem = mod.OptimizationProblem2D()
    constraints = graph.fill(problem, mod, cb.Constraint)
    summary = problem.Solve(constraints, {})
    text = sup.run_cpp("solve", graph.script())
    seen = 0
    for line in text.splitlines():
        f = line.split()
        if f[0] in ("S", "N"):
            pose = tuple(float.fromhex(v) for v in f[3:6])
            key = (int(f[1]), int(f[2]))
            mine = problem.submap_data()[key].global_pose if f[0] == "S" else \
                problem.node_data()[key].global_pose_2d
            assert pose == mine, (f[0], key)
            seen += 1
        elif f[0] == "SUMMARY":
            assert float.fromhex(f[1]) == summary.initial_cost
            assert float.fromhex(f[2]) == summary.final_cost
            assert [int(v) for v in f[3:8]] == [
                summary.num_iterations, summary.num_successful_steps, summary.num_cg_iterations,
                summary.num_cg_capped_steps, summary.termination]
            seen += 1
    assert seen == len(a.poses) + 1
    solved = np.array([problem.submap_data()[s].global_pose for s in a.submap_ids] +
                      [problem.node_data()[n].global_pose_2d for n in a.node_ids])
    dt, da = sup.pose_distance(solved, truth)
    assert dt <= 1e-6 and da <= 1e-6
