"""CPU: the pose-graph solve's checker (tests/cpp/pose_graph2d_ref.cc) against
the reference's recorded SPA numbers and on the loop-closure ring, and the
bookkeeping of OptimizationProblem2D.Assemble() in the Python mirror and the
C++ header (tests/cpp/optimization_problem_2d_test.cc). No GPU: Assemble()
makes no device call."""
import importlib

import numpy as np
import pytest

import pose_graph2d_support as sup


@pytest.fixture(scope="module")
def mod(csm):
    return sup.op2d()


@pytest.fixture(scope="module")
def cb(csm):
    return importlib.import_module("cartographer_amd.constraint_builder")


def test_checker_meets_the_reference_spa_numbers(csm):
    """spa_cost_function_2d_test.cc:109-126, at its own 1e-5."""
    poses, edges, g = sup.golden_spa()
    cost, r, grad, j = sup.ref_evaluate(poses, edges, jacobians=True)
    tol = g["tolerance"]
    assert np.abs(r[0] - g["residuals"]).max() <= tol
    assert np.abs(j[0, :9] - g["jacobian_start"]).max() <= tol
    assert np.abs(j[0, 9:] - g["jacobian_end"]).max() <= tol
    assert cost == pytest.approx(0.5 * float(np.dot(r[0], r[0])), rel=1e-15)
    # The gradient is J'r: the checker's two outputs agree with each other.
    want = np.concatenate([j[0, :9].reshape(3, 3).T @ r[0], j[0, 9:].reshape(3, 3).T @ r[0]])
    assert np.allclose(grad.reshape(-1), want, rtol=1e-14, atol=0)


def test_checker_gradient_is_the_cost_derivative(csm):
    """Central differences of the checker's cost, Huber edges included."""
    poses, edges = sup.evaluate_fixture(3, 24)
    _, _, grad = sup.ref_evaluate(poses, edges)
    rng = np.random.RandomState(0)
    for _ in range(12):
        v, k = int(rng.randint(len(poses) - 1)), int(rng.randint(3))
        h = 1e-6
        hi, lo = poses.copy(), poses.copy()
        hi[v, k] += h
        lo[v, k] -= h
        d = (sup.ref_evaluate(hi, edges)[0] - sup.ref_evaluate(lo, edges)[0]) / (2 * h)
        # Second-order error of the difference plus rounding of costs near 1e9.
        assert d == pytest.approx(grad[v, k], rel=1e-5, abs=5e-1)


def test_checker_closes_the_ring(csm):
    """The dense solve recovers the truth from drifted poses within 50
    iterations and reports a convergence."""
    ring = sup.ring_graph()
    a = sup.assemble(ring)
    truth = sup.truth_array(ring, a)
    before = sup.pose_distance(a.poses, truth)
    assert before[0] > 0.5 and before[1] > 0.1  # the drift is real
    p, s = sup.ref_solve(a.poses, a.constant, a.edges)
    assert s["termination"] in (0, 1, 2) and s["num_iterations"] < 50
    dt, da = sup.pose_distance(p, truth)
    assert dt < 1e-6 and da < 1e-6
    assert s["final_cost"] < 1e-6 < s["initial_cost"]
    assert np.array_equal(p[0], a.poses[0])  # the constant first submap


def test_checker_converges_on_the_noisy_graph(csm):
    """The seed the GPU test uses: a convergence, with Huber edges on both
    sides of the scale at the solution."""
    a = sup.assemble(sup.noisy_graph())
    p, s = sup.ref_solve(a.poses, a.constant, a.edges)
    assert s["termination"] in (0, 1, 2), s
    _, r, _ = sup.ref_evaluate(p, a.edges)
    sq = (r ** 2).sum(1)[a.edges["loss"] == 1]
    assert (sq > sup.HUBER_SCALE ** 2).sum() >= 4 and (sq < sup.HUBER_SCALE ** 2).sum() >= 20


def _two_trajectories(mod, cb):
    """Two trajectories, ids inserted out of order, with a gap in trajectory
    1's node indices."""
    p = mod.OptimizationProblem2D()
    p.InsertSubmap((1, 0), (10.0, 0.0, 0.1))
    p.InsertSubmap((0, 1), (2.0, 0.0, 0.2))
    p.InsertSubmap((0, 0), (0.0, 0.0, 0.3))
    for t, i in [(1, 3), (0, 2), (0, 0), (1, 0), (0, 1), (1, 1)]:
        x = 10.0 * t + i
        p.InsertTrajectoryNode((t, i), mod.NodeSpec2D(float(i), (x, 1.0, 0.01 * i),
                                                      (x + 0.5, 1.5, 0.02 * i)))
    constraints = [cb.Constraint((0, 1), (1, 3), (1.0, 2.0, 0.3), 11.0, 12.0, "INTER_SUBMAP"),
                   cb.Constraint((1, 0), (0, 0), (-1.0, 0.5, -0.2), 5.0, 6.0, "INTRA_SUBMAP")]
    return p, constraints


def test_assemble_orders_submaps_then_nodes_by_id(mod, cb):
    p, constraints = _two_trajectories(mod, cb)
    a = p.Assemble(constraints)
    assert a.submap_ids == [(0, 0), (0, 1), (1, 0)]
    assert a.node_ids == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 3)]
    assert a.poses.shape == (9, 3) and a.poses.dtype == np.float64
    assert a.poses[0].tolist() == [0.0, 0.0, 0.3] and a.poses[2].tolist() == [10.0, 0.0, 0.1]
    assert a.poses[3].tolist() == [0.5, 1.5, 0.0] and a.poses[8].tolist() == [13.5, 1.5, 0.06]


def test_assemble_constraint_edges_and_tags(mod, cb):
    p, constraints = _two_trajectories(mod, cb)
    e = p.Assemble(constraints).edges
    # Submap -> node, in the constraints' order; INTER_SUBMAP takes the Huber loss.
    assert (e[0]["start"], e[0]["end"], e[0]["loss"]) == (1, 8, mod.LOSS_HUBER)
    assert e[0]["zbar"].tolist() == [1.0, 2.0, 0.3]
    assert (e[0]["translation_weight"], e[0]["rotation_weight"]) == (11.0, 12.0)
    assert (e[1]["start"], e[1]["end"], e[1]["loss"]) == (2, 3, mod.LOSS_NONE)


def test_assemble_chain_terms_only_for_consecutive_indices(mod, cb):
    p, constraints = _two_trajectories(mod, cb)
    e = p.Assemble(constraints).edges[len(constraints):]
    # (0,0)-(0,1), (0,1)-(0,2), (1,0)-(1,1); not (0,2)-(1,0) nor (1,1)-(1,3).
    assert [(int(x["start"]), int(x["end"])) for x in e] == [(3, 4), (4, 5), (6, 7)]
    assert all(x["loss"] == mod.LOSS_NONE for x in e)
    assert all(x["translation_weight"] == 1e5 and x["rotation_weight"] == 1e5 for x in e)
    # local_pose(first).inverse() * local_pose(second) (:338-340).
    want = sup.between((0.0, 1.0, 0.0), (1.0, 1.0, 0.01))
    assert e[0]["zbar"].tolist() == list(want)


def test_assemble_constant_first_submap_and_frozen_trajectories(mod, cb):
    p, constraints = _two_trajectories(mod, cb)
    a = p.Assemble(constraints)
    assert a.constant.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    a = p.Assemble(constraints, {1: mod.FROZEN, 0: mod.ACTIVE})
    assert a.constant.tolist() == [1, 0, 1, 0, 0, 0, 1, 1, 1]
    # A frozen trajectory gets no chain terms (:307-310); its constraints stay.
    chain = a.edges[len(constraints):]
    assert [(int(x["start"]), int(x["end"])) for x in chain] == [(3, 4), (4, 5)]
    a = p.Assemble(constraints, {0: mod.FROZEN})
    assert a.constant.tolist() == [1, 1, 0, 1, 1, 1, 0, 0, 0]


def test_assemble_survives_trim_and_add(mod, cb):
    p, constraints = _two_trajectories(mod, cb)
    p.TrimTrajectoryNode((0, 1))
    p.TrimSubmap((0, 0))
    # Append goes one past the trajectory's last index.
    assert p.AddTrajectoryNode(1, mod.NodeSpec2D(4.0, (14.0, 1.0, 0.0), (14.0, 1.0, 0.0))) == (1, 4)
    assert p.AddSubmap(0, (3.0, 0.0, 0.0)) == (0, 2)
    assert p.AddSubmap(5, (0.0, 0.0, 0.0)) == (5, 0)
    a = p.Assemble(constraints)
    assert a.submap_ids == [(0, 1), (0, 2), (1, 0), (5, 0)]
    assert a.node_ids == [(0, 0), (0, 2), (1, 0), (1, 1), (1, 3), (1, 4)]
    assert a.constant.tolist() == [1] + [0] * 9  # the first submap is now (0, 1)
    chain = a.edges[len(constraints):]
    # (0,0)-(0,2) is no longer consecutive; (1,3)-(1,4) is new.
    assert [(int(x["start"]), int(x["end"])) for x in chain] == [(6, 7), (8, 9)]
    assert (int(a.edges[0]["start"]), int(a.edges[0]["end"])) == (0, 8)
    assert set(p.node_data()) == set(a.node_ids) and set(p.submap_data()) == set(a.submap_ids)


def test_options_carry_the_reference_defaults(mod):
    o = mod.OptimizationProblem2D().options
    assert (o.huber_scale, o.local_slam_pose_translation_weight,
            o.local_slam_pose_rotation_weight, o.max_num_iterations) == (10.0, 1e5, 1e5, 50)
    p = mod.OptimizationProblem2D()
    p.SetMaxNumIterations(7)
    assert p.options.max_num_iterations == 7


def _script_of(ops):
    return "\n".join(ops) + "\n"


def test_cpp_header_assembles_the_same_problem(mod, cb):
    """The C++ header against the mirror, in bits, on the ring, on the noisy
    graph and on a script with trims, appends and a frozen trajectory."""
    for graph in (sup.ring_graph(), sup.noisy_graph()):
        a = sup.assemble(graph)
        poses, constant, rows, sids, nids = sup.parse_assembled(
            sup.run_cpp("assemble", graph.script()))
        assert sids == a.submap_ids and nids == a.node_ids
        assert np.array_equal(poses, a.poses) and np.array_equal(constant, a.constant)
        assert sup.edges_array(rows).tobytes() == a.edges.tobytes()

    p, constraints = _two_trajectories(mod, cb)
    p.TrimTrajectoryNode((0, 1))
    p.TrimSubmap((0, 0))
    p.AddTrajectoryNode(1, mod.NodeSpec2D(4.0, (14.0, 1.0, 0.0), (14.0, 1.0, 0.0)))
    p.AddSubmap(0, (3.0, 0.0, 0.0))
    a = p.Assemble(constraints, {1: mod.FROZEN})
    ops = ["S 1 0 10.0 0.0 0.1", "S 0 1 2.0 0.0 0.2", "S 0 0 0.0 0.0 0.3"]
    for t, i in [(1, 3), (0, 2), (0, 0), (1, 0), (0, 1), (1, 1)]:
        x = 10.0 * t + i
        ops.append("N %d %d %r %r 1.0 %r %r 1.5 %r" % (t, i, float(i), x, 0.01 * i, x + 0.5,
                                                      0.02 * i))
    ops += ["C 0 1 1 3 1.0 2.0 0.3 11.0 12.0 1", "C 1 0 0 0 -1.0 0.5 -0.2 5.0 6.0 0",
            "TN 0 1", "TS 0 0", "AN 1 4.0 14.0 1.0 0.0 14.0 1.0 0.0", "AS 0 3.0 0.0 0.0", "F 1"]
    poses, constant, rows, sids, nids = sup.parse_assembled(
        sup.run_cpp("assemble", _script_of(ops)))
    assert sids == a.submap_ids and nids == a.node_ids
    assert np.array_equal(poses, a.poses) and np.array_equal(constant, a.constant)
    assert sup.edges_array(rows).tobytes() == a.edges.tobytes()
