"""The constraint builders' shared host skeleton, on the CPU: flush timing,
slot order and counters, DeleteScanMatcher between enqueue and flush, the cut
into sub-batches under a matcher budget and sharding alone.

A stub dimension drives it: its matcher is a byte size and its search records
the pairs it was given and returns scripted statuses, so no device is touched.
tests/cpp/constraint_builder_skeleton_test.cc does this for
ConstraintBuilderBase (its in-process checks make the exit code; the stderr
lines are checked here), and ``_Stub`` below runs the same scripts through the
Python base.
"""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT

CPP_TEST = os.path.join(ROOT, "tests", "cpp", "constraint_builder_skeleton_test.cc")
CPP_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "constraint_builder_skeleton_test")

SKIP_TEXT = "input exceeds the device path's index limits"  # csm_strerror(CSM_ERANGE)
ORDER_STDERR = [f"StubBuilder: 1 of 4 pairs skipped ({SKIP_TEXT})",
                f"StubBuilder: 2 of 4 pairs skipped ({SKIP_TEXT})"]
DELETE_STDERR = ["StubBuilder: DeleteScanMatcher dropped 2 pending pairs of a deleted submap"]


@pytest.fixture(scope="module")
def cpp_bin(csm):
    os.makedirs(os.path.dirname(CPP_BIN), exist_ok=True)
    libdir = os.path.join(ROOT, "cartographer-1_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "include"), CPP_TEST, "-o", CPP_BIN,
                           "-L", libdir, "-lcsm_amd", "-Wl,-rpath," + libdir])
    return CPP_BIN


@pytest.mark.parametrize("case,stderr", [
    ("flush_every_node", []), ("flush_at_five", []), ("order_and_counters", ORDER_STDERR),
    ("delete_before_flush", DELETE_STDERR), ("budget", []), ("sharding_alone", [])])
def test_cpp_skeleton(cpp_bin, case, stderr):
    out = subprocess.run([cpp_bin, case], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout == "OK\n"
    assert out.stderr.splitlines() == stderr


# ------------------------------------------------------- the Python base --
@pytest.fixture(scope="module")
def cb(csm):
    return importlib.import_module("cartographer_amd.constraint_builder")


class _Matcher:
    def __init__(self, nbytes):
        self.nbytes = nbytes

    def device_bytes(self):
        return self.nbytes

    def close(self):
        pass


class _Pair:
    def __init__(self, ident, submap, node, full, status, nbytes):
        self.id, self.submap_id, self.node_id, self.full = ident, (0, submap), (0, node), full
        self.status, self.nbytes, self.slot = status, nbytes, -1


def _stub(cb, flush_pairs, sampling_ratio=1.0, matcher_cache_bytes=0):
    class _Stub(cb._ConstraintBuilderBase):
        _name = "StubBuilder"
        _metrics = cb._BuilderMetrics(False)

        def __init__(self, options):
            super().__init__(options, context=object())  # a placeholder: never used
            self.batches, self.held_bytes, self.log = [], [], []
            self.log_sink = self.log.append

        def add(self, ident, submap, node, full, status=0, nbytes=10):
            if not full and not self._sample((0, submap)):
                return
            self._enqueue(_Pair(ident, submap, node, full, status, nbytes))

        def _make_matcher(self, p):
            return _Matcher(p.nbytes)

        def _log_when_done(self, computations, constraints):
            self.log_sink(f"done {computations} {constraints}")

        def _run_batch(self, pending, held):
            assert all(p.submap_id in held for p in pending)
            self.batches.append([p.id for p in pending])
            self.held_bytes.append(sum(m.device_bytes() for m in held.values()))
            assert len(held) == len({p.submap_id for p in pending})
            return [(p.status, (0.5,), p.id, f"match {p.id}") for p in pending]

        def done(self):
            got = []
            self.WhenDone(got.append)
            assert len(got) == 1
            return got[0]

    # matcher_cache_bytes 0: one batch per flush, in submission order
    return _Stub(cb.ConstraintBuilderOptions(flush_pairs=flush_pairs,
                                             sampling_ratio=sampling_ratio,
                                             matcher_cache_bytes=matcher_cache_bytes))


def test_flush_every_node(cb):
    b = _stub(cb, 0)
    assert b.GetNumFinishedNodes() == 0
    for node in range(3):
        b.add(2 * node, 0, node, False)
        b.add(2 * node + 1, 1, node, True)
        assert len(b.batches) == node
        b.NotifyEndOfNode()
        assert b.batches[node:] == [[2 * node, 2 * node + 1]]
        assert b.GetNumFinishedNodes() == node + 1
    b.NotifyEndOfNode()  # a node without pairs finishes at once
    assert len(b.batches) == 3 and b.GetNumFinishedNodes() == 4
    assert b.done() == [0, 1, 2, 3, 4, 5]
    assert len(b.batches) == 3


def test_flush_at_five(cb):
    b = _stub(cb, 5)
    for node, finished in enumerate((0, 0, 3, 3)):
        b.add(2 * node, 0, node, False)
        b.add(2 * node + 1, 1, node, True)
        b.NotifyEndOfNode()
        assert b.GetNumFinishedNodes() == finished
        assert b.batches == ([] if node < 2 else [[0, 1, 2, 3, 4, 5]])
    assert b.done() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert b.batches == [[0, 1, 2, 3, 4, 5], [6, 7]]
    assert b.GetNumFinishedNodes() == 4


def test_order_and_counters(cb, csm, capsys):
    """The script of OrderAndCounters in the C++ test: local searched 0 3 4 9,
    found 0 3 9; global searched 1 5 8, found 5 8; failed 2 6 7."""
    ok, no_match, erange = csm.CSM_OK, csm.CSM_NO_MATCH, csm.CSM_ERANGE
    b = _stub(cb, 0)
    script = [[(0, 0, False, ok), (1, 1, True, no_match), (2, 0, True, erange), (3, 1, False, ok)],
              [(4, 0, False, no_match), (5, 1, True, ok), (6, 1, False, erange),
               (7, 0, False, erange)],
              [(8, 0, True, ok), (9, 1, False, ok)]]
    for node, pairs in enumerate(script):
        for ident, submap, full, status in pairs:
            b.add(ident, submap, node, full, status)
        b.NotifyEndOfNode()
        if node == 0:
            assert (b.last_error, b.constraints_failed) == (erange, 1)
    assert b.done() == [0, 3, 5, 8, 9]
    assert (b.constraints_searched, b.constraints_found) == (4, 3)
    assert (b.global_constraints_searched, b.global_constraints_found) == (3, 2)
    assert (b.constraints_failed, b.last_error) == (3, erange)
    assert len(b.constraint_scores) == 3 and len(b.global_constraint_scores) == 2
    # "computations" counts the slots, not the results.
    assert b.log == ["match 0", "match 3", "match 5", "match 8", "match 9", "done 10 5"]
    assert capsys.readouterr().err.splitlines() == ORDER_STDERR
    assert b.done() == [] and b.log[-1] == "done 0 0"


def test_delete_before_flush(cb, capsys):
    """0 A local (taken), 1 B local (taken), 2 A global, 3 B global, delete A,
    4 A local (taken only by a fresh sampler), 5 B local (dropped)."""
    b = _stub(cb, 100, sampling_ratio=0.5)
    b.add(0, 0, 0, False)
    b.add(1, 1, 0, False)
    b.add(2, 0, 0, True)
    b.add(3, 1, 0, True)
    b.NotifyEndOfNode()
    assert (b.num_submap_scan_matchers, b._matchers.builds) == (2, 2)
    b.DeleteScanMatcher((0, 0))
    assert (b.num_submap_scan_matchers, b._matchers.bytes) == (1, 10)
    b.add(4, 0, 1, False)
    b.add(5, 1, 1, False)
    b.NotifyEndOfNode()
    assert (b.num_submap_scan_matchers, b._matchers.builds) == (2, 3)
    assert b.batches == [] and b.GetNumFinishedNodes() == 0
    assert b.done() == [1, 3, 4]
    assert b.batches == [[1, 3, 4]]
    assert b.log[-1] == "done 5 3"  # the dropped pairs' slots still count
    assert (b.constraints_searched, b.global_constraints_searched) == (2, 1)
    assert b.GetNumFinishedNodes() == 2
    assert capsys.readouterr().err.splitlines() == DELETE_STDERR


SUBMAP_OF = (3, 0, 4, 1, 3, 2, 0, 4, 1, 2)  # five submaps of 10 bytes, interleaved


def test_budget(cb):
    """Budget 25. Every enqueue builds the pair's matcher, unpins it and trims,
    so from the third on the oldest one goes: 10 builds, 8 evictions, {1, 2}
    cached. The flush takes the submaps in id order and rebuilds each (15
    builds). 0 and 1 each push out an unpinned matcher (10 evictions); 2 finds
    all pinned and does not fit beside 0 and 1, which are searched, then 0 is
    unpinned and goes (11); 3 pushes out 1 (12); 4 does not fit beside 2 and 3,
    which are searched, then 2 goes (13); 4 is searched alone."""
    b = _stub(cb, 100, matcher_cache_bytes=25)
    for k, submap in enumerate(SUBMAP_OF):
        b.add(k, submap, k // 4, k % 2 == 0)
    assert (b._matchers.builds, b._matchers.evictions) == (10, 8)
    assert b.done() == list(range(10))
    assert b.batches == [[1, 6, 3, 8], [5, 9, 0, 4], [2, 7]]
    assert b.held_bytes == [20, 20, 10]
    # Whole submaps: each is in one batch only.
    submaps = [s for batch in b.batches for s in sorted({SUBMAP_OF[k] for k in batch})]
    assert sorted(submaps) == [0, 1, 2, 3, 4]
    assert (b._matchers.builds, b._matchers.evictions) == (15, 13)
    assert (b.num_submap_scan_matchers, b._matchers.bytes) == (2, 20)
    assert not b._matchers.pinned

    big = _stub(cb, 100, matcher_cache_bytes=25)  # a submap past the budget goes alone
    big.add(0, 0, 0, True)
    big.add(1, 1, 0, True, nbytes=30)
    big.add(2, 2, 0, True)
    assert big.done() == [0, 1, 2]
    assert big.batches == [[0], [1], [2]] and big.held_bytes == [10, 30, 10]

    u = _stub(cb, 100, matcher_cache_bytes=0)  # unbounded: one batch, submission order
    for k, submap in enumerate(SUBMAP_OF):
        u.add(k, submap, k // 4, k % 2 == 0)
    assert u.done() == list(range(10))
    assert u.batches == [list(range(10))]
    assert (u._matchers.builds, u._matchers.evictions) == (5, 0)
    assert (u.num_submap_scan_matchers, u._matchers.bytes) == (5, 50)
