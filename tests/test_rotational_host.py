"""CPU: pins the oracle's RotationalScanMatcher (oracle/match3d.cc RotateHistogram,
MatchHistograms, ReduxSumSse) before test_rotational_gpu.py trusts it bit for
bit: against a numpy restatement with float64 sums, against a float32
restatement of Eigen's packet-order reduction written separately from the
oracle's, and on the reference's two RotationalScanMatcher3DTest cases
(rotational_scan_matcher_test.cc:28-67) stated in the argument conventions of
csm_rotational_scores_batch (rotational_support.py).

Bound of the float64 comparison, 1e-6: every term of the three sums is
non-negative, so nothing cancels; a float32 sum of n <= 512 such terms, the
float32 interpolation, two square roots and the division stay within a few
float32 ulps of the float64 value. The worst deviation seen over the cases
below is 2.7e-7 (printed per window); 1e-6 is about four times that."""
import math

import numpy as np
import pytest
from rotational_support import (F32, normalization_edge, oracle_scores, packet_sum_f32,
                                restated_scores, step_for, unit)

SIZES = list(range(1, 18)) + [23, 24, 119, 120, 121, 127, 128, 129, 511, 512]
WINDOWS = [0, 31, 32, 127, 128, 400]
YAW0S = [0.0, 3.1, -3.14159]


@pytest.mark.parametrize("window", WINDOWS)
def test_oracle_scores_match_float64_restatement(oracle, window):
    rng = np.random.default_rng(1000 + window)
    worst = 0.0
    for n in SIZES:
        for yaw0 in YAW0S:
            submap = rng.uniform(0, 5, n).astype(F32)
            node = rng.uniform(0, 5, n).astype(F32)
            got = oracle_scores(oracle, submap, node, yaw0, window, step_for(window))
            want = restated_scores(submap, node, yaw0, window, step_for(window))
            worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want))))
    print(f"window {window}: worst |oracle - float64 restatement| = {worst:.3g}")
    assert worst <= 1e-6


def test_oracle_empty_histogram_scores_one(oracle):
    got = oracle_scores(oracle, np.zeros(0, F32), np.zeros(0, F32), 0.3, 5, 0.1)
    assert np.array_equal(got, np.ones(11, F32))
    assert np.array_equal(restated_scores([], [], 0.3, 5, 0.1), np.ones(11))


def test_oracle_packet_sum_is_eigens_order(oracle):
    rng = np.random.default_rng(7)
    for n in list(range(0, 34)) + list(range(119, 130)) + [511, 512]:
        for _ in range(4):
            v = rng.uniform(0, 5, n).astype(F32)
            a, b = oracle.redux_sum(v), packet_sum_f32(v)
            assert a.view(np.int32) == b.view(np.int32), (n, a, b)
    # The order matters: a plain left-to-right float32 sum differs somewhere.
    v = rng.uniform(0, 5, 512).astype(F32)
    serial = F32(0)
    for x in v:
        serial = F32(serial + x)
    assert serial != packet_sum_f32(v)


def test_only_same_histogram_is_score_one(oracle):
    """RotationalScanMatcher3DTest.OnlySameHistogramIsScoreOne: angles {0, 1}
    are yaws k = 1, 2 of a record with window 1 and step 1."""
    h = np.array([1, 43, 0.5, 0.3123, 23, 42, 0], F32)
    scores = oracle_scores(oracle, h, h, 0.0, 1, 1.0)
    assert len(scores) == 3
    assert abs(1.0 - scores[1]) <= 1e-6
    assert scores[2] < 1.0 and scores[0] < 1.0
    want = restated_scores(h, h, 0.0, 1, 1.0)
    assert np.max(np.abs(scores - want)) <= 1e-6


def test_interpolates_as_expected(oracle):
    """RotationalScanMatcher3DTest.InterpolatesAsExpected: each angle is a
    record of window 0 whose yaw0 is the angle (initial_angle 0.f + angle is
    the angle itself)."""
    buckets = 10
    per_bucket = F32(math.pi / buckets)
    submap = unit(buckets, 3)
    t = F32(0)
    while t < 1:
        expected = float(t) / math.hypot(float(t), 1 - float(t))
        for node, angle in [(unit(buckets, 2), t * per_bucket),
                            (unit(buckets, 2), (2 - t) * per_bucket),
                            (unit(buckets, 4), -t * per_bucket),
                            (unit(buckets, 4), (t - 2) * per_bucket)]:
            score = oracle_scores(oracle, submap, node, F32(angle), 0, 1.0)
            assert len(score) == 1
            assert abs(expected - float(score[0])) <= 1e-6, (t, angle)
            assert abs(restated_scores(submap, node, F32(angle), 0, 1.0)[0] - expected) <= 1e-6
        t = F32(t + F32(0.1))


def test_normalization_edge_values(oracle):
    """The two inputs test_rotational_gpu.py uses around normalization < 1e-3f:
    adjacent floats, exactly 1 below and the true score (2 / sqrt(5)) above."""
    v0, v1, yaw0 = normalization_edge(oracle)
    assert np.nextafter(v0, F32(1)) == v1
    below = oracle_scores(oracle, unit(4, 0, v0), unit(4, 0, v0), yaw0, 0, 0.1)[0]
    above = oracle_scores(oracle, unit(4, 0, v1), unit(4, 0, v1), yaw0, 0, 0.1)[0]
    assert below == 1.0
    assert abs(float(above) - 2 / math.sqrt(5)) <= 1e-6
