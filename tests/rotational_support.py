"""Shared by test_rotational_host.py and test_rotational_gpu.py: a numpy
restatement of RotationalScanMatcher::Match (rotational_scan_matcher.cc:
119-185) that is independent of the oracle's C++, a float32 restatement of
Eigen's packet-order sum, and the inputs both files use.

Conventions of csm_rotational_scores_batch: a record scores the angles
yaw0 + (k - window) * step, k = 0..2 * window, all in float32; the oracle
takes the same angles as Match(histogram, initial_angle = yaw0, angles[k] =
float(k - window) * step)."""
import math

import numpy as np

F32 = np.float32
K_MIN_NORMALIZATION = float(F32(1e-3))  # MatchHistograms: normalization < 1e-3f -> 1.f


def angles_of(window, step):
    """angles[k] = float(k - window) * step, as GenerateDiscreteScans builds them."""
    return (np.arange(-window, window + 1).astype(F32) * F32(step)).astype(F32)


def step_for(window):
    return F32(0.999 * math.pi / max(window, 1))


def lround(x):
    """std::lround: halves away from zero."""
    x = float(x)
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def rotation_of(angle, n):
    """RotateHistogram's bucket arithmetic in float32, as the reference:
    (full_buckets mod n, fraction)."""
    rotate_by_buckets = F32(np.float64(F32(-F32(angle)) * F32(n)) / math.pi)
    full = lround(F32(rotate_by_buckets - F32(0.5)))
    fraction = F32(rotate_by_buckets - F32(full))
    return full % n, fraction


def restated_scores(submap_histogram, histogram, yaw0, window, step):
    """Every yaw's score with the sums, norms and the division in float64."""
    s = np.asarray(submap_histogram, np.float64)
    h = np.asarray(histogram, np.float64)
    n = len(h)
    count = 2 * window + 1
    if n == 0:
        return np.ones(count)
    out = np.empty(count)
    index = np.arange(n)
    submap_norm = math.sqrt(float(s @ s))
    for k, a in enumerate(angles_of(window, step)):
        full, fraction = rotation_of(F32(yaw0) + a, n)
        f = float(fraction)
        rotated = f * h[(index + 1 + full) % n] + (1.0 - f) * h[(index + full) % n]
        normalization = math.sqrt(float(rotated @ rotated)) * submap_norm
        out[k] = 1.0 if normalization < K_MIN_NORMALIZATION else float(s @ rotated) / normalization
    return out


def packet_sum_f32(values):
    """Eigen's aligned 4-wide linear reduction (Redux.h) in float32, by lanes:
    two packet accumulators over the 8-strided part, a third packet when a
    whole one is left, the lanes folded (0 + 2) + (1 + 3), then the scalar
    tail."""
    v = np.asarray(values, F32)
    n = len(v)
    whole4, whole8 = n - n % 4, n - n % 8
    if whole4 == 0:
        r = F32(0)
        for i, x in enumerate(v):
            r = x if i == 0 else F32(r + x)
        return r
    lanes = v[:whole4].reshape(-1, 4)  # packet j = lanes[j]
    acc = lanes[0].copy()
    if whole4 > 4:
        even, odd = lanes[0].copy(), lanes[1].copy()
        for j in range(2, whole8 // 4, 2):
            even = (even + lanes[j]).astype(F32)
            odd = (odd + lanes[j + 1]).astype(F32)
        acc = (even + odd).astype(F32)
        if whole4 > whole8:
            acc = (acc + lanes[whole8 // 4]).astype(F32)
    r = F32(F32(acc[0] + acc[2]) + F32(acc[1] + acc[3]))
    for x in v[whole4:]:
        r = F32(r + x)
    return r


def oracle_scores(oracle, submap_histogram, histogram, yaw0, window, step):
    return oracle.rotational_match(submap_histogram, histogram, F32(yaw0), angles_of(window, step))


def unit(n, i, value=1.0):
    h = np.zeros(n, F32)
    h[i] = value
    return h


def rounding_margins(window, step):
    """yaw_build keeps its own float rounding of sin(|angle| / 2) / |angle|
    and cos(|angle| / 2) only when the double value lies farther than 2^-40
    (relative) from a float rounding boundary; closer yaws are flagged and
    rebuilt on the host. Returns, per yaw k, the smaller relative distance of
    the two values from such a boundary (inf where the angle is too small for
    the branch), computed here with libm."""
    def margin(v):
        f = F32(v)
        up, down = float(np.nextafter(f, F32(np.inf))), float(np.nextafter(f, F32(-np.inf)))
        return min(abs(v - 0.5 * (float(f) + up)), abs(v - 0.5 * (float(f) + down))) / v

    out = np.full(2 * window + 1, np.inf)
    for k, angle in enumerate(angles_of(window, step)):
        sq = F32(angle * angle)
        if float(sq) > 1e-8:
            norm = float(F32(np.sqrt(sq)))
            out[k] = min(margin(abs(math.sin(norm / 2) / norm)), margin(abs(math.cos(norm / 2))))
    return out


def normalization_edge(oracle):
    """Two adjacent float32 values v0 < v1 for which MatchHistograms' norm
    product of unit(4, 0, v) against itself, rotated by a third of a bucket,
    lies below 1e-3f at v0 (the oracle returns exactly 1) and not at v1 (it
    returns the true score, about 0.894). Found by bisection on the float32
    bit pattern: the product is monotonic in v."""
    yaw0 = F32(-math.pi / 12)  # -angle * 4 / pi = 1 / 3 of a bucket

    def score(v):
        return oracle_scores(oracle, unit(4, 0, v), unit(4, 0, v), yaw0, 0, F32(0.1))[0]

    lo, hi = F32(0.01), F32(0.1)
    assert score(lo) == 1 and score(hi) != 1
    lo_bits, hi_bits = int(lo.view(np.int32)), int(hi.view(np.int32))
    while hi_bits - lo_bits > 1:
        mid = (lo_bits + hi_bits) // 2
        if score(np.int32(mid).view(F32)) == 1:
            lo_bits = mid
        else:
            hi_bits = mid
    return np.int32(lo_bits).view(F32), np.int32(hi_bits).view(F32), yaw0
