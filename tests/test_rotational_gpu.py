"""GPU: the three device stages that run before FastCorrelativeScanMatcher3D
searches anything (kernels3d.hip rot_scores, yaw_compact, yaw_build with the
host's flag patches), every yaw checked, against the oracle
(test_rotational_host.py pins it first).

Raw entry (csm_rotational_scores_batch): every score of every record is the
oracle's float32 bit for bit and within 1e-6 of the float64 restatement
(rotational_support.py; the bound is derived in test_rotational_host.py).
Histogram sizes by the branch of PacketSum / PacketSum2 they take:
  n = 0: 0 | n < 4: 1, 2, 3 | 4 <= n < 8: 4, 5, 7 |
  n % 8 == 0: 8, 16, 120, 512 | n % 8 in 1..3 (tail only): 9, 11, 17, 121 |
  n % 8 == 4 (third packet, no tail): 12, 124 |
  n % 8 in 5..7 (third packet and tail): 13, 15, 127, 511.
Windows put 2A + 1 on both sides of rot_scores' 64-yaw blocks (64, 128, 512,
768) and yaw_compact's 256-yaw chunks; the angles span [-2 pi, 2 pi], so
`while (full < 0)` and `full %= n` both run, and yaw0 = 0 has angle == 0.

Matcher entry (csm_fast3d_discrete_scans): k, score, q, n and t of every kept
yaw are the bits of the oracle's own GenerateDiscreteScans, under the three
yaw-build modes."""
import ctypes as C
import math

import numpy as np
import pytest
from rotational_support import (F32, normalization_edge, oracle_scores, restated_scores,
                                rounding_margins, step_for, unit)
from test_fast3d_gpu import (TEST_CLOUD, assert_same_result, gpu_grid, opt_tuple, options, quat_z,
                             transform)

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, 120, 121, 124, 127, 511, 512]
WINDOWS = [0, 1, 31, 32, 63, 64, 127, 128, 255, 256, 383, 384]
YAW0S = [0.0, 3.1, -3.14159, 1e-3]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class Records:
    """Histograms packed into one array (shared where records share them) and
    the records over them, with the oracle's scores per record."""

    def __init__(self):
        self.floats = []
        self.size = 0
        self.rows = []       # (node offset, submap offset, size, window, step, yaw0)
        self.inputs = []     # (submap histogram, node histogram)

    def add_histogram(self, h):
        h = np.asarray(h, F32)
        self.floats.append(h)
        self.size += len(h)
        return self.size - len(h), h

    def add(self, node, submap, window, step, yaw0):
        (node_at, node_h), (submap_at, submap_h) = node, submap
        assert len(node_h) == len(submap_h)
        self.rows.append((node_at, submap_at, len(node_h), window, F32(step), F32(yaw0)))
        self.inputs.append((submap_h, node_h))

    def histograms(self):
        return np.concatenate(self.floats + [np.zeros(0, F32)])

    def pairs(self, min_scores):
        return [row + (float(m),) for row, m in zip(self.rows, min_scores)]

    def oracle_scores(self, oracle):
        return [oracle_scores(oracle, s, h, row[5], row[3], row[4])
                for (s, h), row in zip(self.inputs, self.rows)]

    def restated_scores(self):
        return [restated_scores(s, h, row[5], row[3], row[4])
                for (s, h), row in zip(self.inputs, self.rows)]


def build_mixed():
    """Every size with every window in one batch; per size the windows cycle
    through the four kinds of data and the yaw0 values."""
    rng = np.random.default_rng(2024)
    rec = Records()
    for si, n in enumerate(SIZES):
        for wi, window in enumerate(WINDOWS):
            kind = wi % 4
            yaw0 = YAW0S[(wi // 4 + si) % 4]
            random = rec.add_histogram(rng.uniform(0, 5, n))
            if kind == 0:    # two random histograms
                node, submap = random, rec.add_histogram(rng.uniform(0, 5, n))
            elif kind == 1:  # the only non-zero bucket is the first
                node, submap = rec.add_histogram(unit(n, 0, 2.5) if n else []), random
            elif kind == 2:  # ... is the last: read through the wrap at full = 0
                node, submap = rec.add_histogram(unit(n, n - 1, 3.0) if n else []), random
            else:            # the same histogram on both sides
                node = submap = random
            rec.add(node, submap, window, step_for(window), yaw0)
    return rec


@pytest.fixture(scope="module")
def mixed(oracle):
    rec = build_mixed()
    return rec, rec.oracle_scores(oracle), rec.restated_scores()


def check_kept(pairs, want_scores, ranges, kept_k, kept_s):
    """yaw_compact's contract for one call: per record the kept k, in
    increasing order, are those with not (double(score) < min_score), with
    their scores' bits; the ranges tile [0, sum of counts) whatever their
    order (the cursor is atomic)."""
    for p, (pair, want) in enumerate(zip(pairs, want_scores)):
        keep = np.nonzero(~(want.astype(np.float64) < pair[6]))[0]
        at, count = ranges[p]
        assert count == len(keep), (p, pair)
        assert np.array_equal(kept_k[at:at + count], keep), (p, pair)
        assert np.array_equal(bits(kept_s[at:at + count]), bits(want[keep])), (p, pair)
    order = np.argsort(ranges[:, 0], kind="stable")
    starts, counts = ranges[order, 0], ranges[order, 1]
    live = counts > 0
    assert np.array_equal(starts[live], (np.cumsum(counts[live]) - counts[live]))
    assert int(counts.sum()) == len(kept_k) == len(kept_s)


def test_every_score_is_the_oracles(csm, mixed):
    rec, want, restated = mixed
    pairs = rec.pairs([0.5] * len(rec.rows))
    scores, ranges, kept_k, kept_s = csm.rotational_scores_batch(rec.histograms(), pairs)
    worst = 0.0
    for p, (got, ref, f64) in enumerate(zip(scores, want, restated)):
        assert len(got) == 2 * pairs[p][3] + 1
        bad = np.nonzero(bits(got) != bits(ref))[0]
        assert len(bad) == 0, (pairs[p], bad[:8], got[bad[:8]], ref[bad[:8]])
        worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - f64))))
    print(f"worst |kernel - float64 restatement| over {sum(map(len, scores))} yaws: {worst:.3g}")
    assert worst <= 1e-6
    check_kept(pairs, want, ranges, kept_k, kept_s)


def test_shared_histograms_over_many_pairs(csm, oracle):
    """300 records: one node histogram against three submap histograms."""
    rng = np.random.default_rng(5)
    rec = Records()
    node = rec.add_histogram(rng.uniform(0, 5, 121))
    submaps = [rec.add_histogram(rng.uniform(0, 5, 121)) for _ in range(3)]
    for i in range(300):
        rec.add(node, submaps[i % 3], 40, step_for(40), -3.0 + 0.02 * i)
    want = rec.oracle_scores(oracle)
    pairs = rec.pairs([0.7 + 0.0005 * i for i in range(300)])
    scores, ranges, kept_k, kept_s = csm.rotational_scores_batch(rec.histograms(), pairs)
    for got, ref in zip(scores, want):
        assert np.array_equal(bits(got), bits(ref))
    check_kept(pairs, want, ranges, kept_k, kept_s)
    assert 0 < len(kept_k) < 300 * 81


def test_normalization_edge(csm, oracle):
    """normalization < 1e-3f returns 1: an all-zero node histogram, an
    all-zero submap histogram, and one non-zero bucket of adjacent float
    values whose norm product lies on either side of the threshold."""
    rng = np.random.default_rng(6)
    v0, v1, yaw0 = normalization_edge(oracle)
    rec = Records()
    zero, random = rec.add_histogram(np.zeros(9)), rec.add_histogram(rng.uniform(0, 5, 9))
    rec.add(zero, random, 2, 0.3, 0.1)
    rec.add(random, zero, 2, 0.3, 0.1)
    below, above = rec.add_histogram(unit(4, 0, v0)), rec.add_histogram(unit(4, 0, v1))
    rec.add(below, below, 0, 0.1, yaw0)
    rec.add(above, above, 0, 0.1, yaw0)
    want = rec.oracle_scores(oracle)
    assert np.all(want[0] == 1) and np.all(want[1] == 1) and want[2][0] == 1 and want[3][0] < 0.9
    scores, _, _, _ = csm.rotational_scores_batch(rec.histograms(), rec.pairs([0.5] * 4))
    for got, ref in zip(scores, want):
        assert np.array_equal(bits(got), bits(ref)), (got, ref)


def test_reference_cases(csm, oracle):
    """rotational_scan_matcher_test.cc:28-67 through the kernels."""
    rec = Records()
    h = rec.add_histogram([1, 43, 0.5, 0.3123, 23, 42, 0])
    rec.add(h, h, 1, 1.0, 0.0)  # angles {-1, 0, 1}
    submap = rec.add_histogram(unit(10, 3))
    two, four = rec.add_histogram(unit(10, 2)), rec.add_histogram(unit(10, 4))
    per_bucket = F32(math.pi / 10)
    expected = [None]
    t = F32(0)
    while t < 1:
        e = float(t) / math.hypot(float(t), 1 - float(t))
        for node, angle in [(two, t * per_bucket), (two, (2 - t) * per_bucket),
                            (four, -t * per_bucket), (four, (t - 2) * per_bucket)]:
            rec.add(node, submap, 0, 1.0, F32(angle))
            expected.append(e)
        t = F32(t + F32(0.1))
    scores, _, _, _ = csm.rotational_scores_batch(rec.histograms(), rec.pairs([0.0] * len(rec.rows)))
    for got, ref in zip(scores, rec.oracle_scores(oracle)):
        assert np.array_equal(bits(got), bits(ref))
    assert abs(1.0 - scores[0][1]) <= 1e-6 and scores[0][2] < 1.0
    for got, e in zip(scores[1:], expected[1:]):
        assert abs(float(got[0]) - e) <= 1e-6


def test_filter_at_equality_and_bounds(csm, mixed):
    """Each record of the mixed batch four times over the same histograms:
    min_score at one of its own scores s (that yaw, and every yaw of equal
    score, is kept), at the next double above s (they are dropped), at -1
    (all kept) and at 2 (none)."""
    rec, want, _ = mixed
    pairs, scores, chosen = [], [], []
    for row, ref in zip(rec.rows, want):
        s = np.float64(ref[len(ref) // 3])
        for m in (s, np.nextafter(s, np.inf), -1.0, 2.0):
            pairs.append(row + (float(m),))
            scores.append(ref)
        chosen.append(s)
    got, ranges, kept_k, kept_s = csm.rotational_scores_batch(rec.histograms(), pairs)
    check_kept(pairs, scores, ranges, kept_k, kept_s)
    for i, (ref, s) in enumerate(zip(want, chosen)):
        equal = np.nonzero(ref.astype(np.float64) == s)[0]
        assert len(equal) > 0
        at, count = ranges[4 * i]
        assert np.all(np.isin(equal, kept_k[at:at + count]))
        at, count = ranges[4 * i + 1]
        assert not np.any(np.isin(equal, kept_k[at:at + count]))
        assert ranges[4 * i + 2][1] == len(ref)
        assert ranges[4 * i + 3][1] == 0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, scores))


def test_rejections(csm):
    """Every CSM_EINVAL of csm_rotational_scores_batch: null pointers, sizes,
    windows and histogram offsets out of range, non-finite step, yaw0 and
    min_score (a bad record after a good one rejects the call)."""
    ctx = csm.default_context()
    lib = ctx._lib
    hists = np.arange(600, dtype=np.float32)
    good = (0, 10, 8, 3, 0.1, 0.2, 0.5)

    def call(rows, **nulls):
        arr = np.array(rows, csm.ROT_PAIR3_DTYPE)
        n = int((2 * arr["window"].astype(np.int64) + 1).clip(min=1).sum())
        scores, ks = np.zeros(n, np.float32), np.zeros(n, np.float32)
        ranges, kk = np.zeros((len(arr), 2), np.int32), np.zeros(n, np.int32)
        kept = C.c_int64()
        a = dict(ctx=ctx.handle, hists=hists.ctypes.data_as(C.POINTER(C.c_float)),
                 pairs=arr.ctypes.data_as(C.POINTER(csm.RotPair3D)),
                 scores=scores.ctypes.data_as(C.POINTER(C.c_float)),
                 ranges=ranges.ctypes.data_as(C.POINTER(C.c_int32)),
                 kk=kk.ctypes.data_as(C.POINTER(C.c_int32)),
                 ks=ks.ctypes.data_as(C.POINTER(C.c_float)), kept=C.byref(kept))
        a.update(nulls)
        return lib.csm_rotational_scores_batch(a["ctx"], a["hists"], len(hists), a["pairs"],
                                               len(arr), a["scores"], a["ranges"], a["kk"],
                                               a["ks"], a["kept"])

    assert call([good]) == csm.CSM_OK
    assert call([(0, 0, 512, 3, 0.1, 0.2, 0.5)]) == csm.CSM_OK       # kMaxHistogram itself
    for null in ("ctx", "hists", "pairs", "scores", "ranges", "kk", "ks", "kept"):
        assert call([good], **{null: None}) == csm.CSM_EINVAL, null
    inf, nan = math.inf, math.nan
    for bad in [(0, 10, -1, 3, 0.1, 0.2, 0.5), (0, 0, 513, 3, 0.1, 0.2, 0.5),
                (0, 10, 8, -1, 0.1, 0.2, 0.5), (0, 10, 8, 32769, 0.1, 0.2, 0.5),
                (0, 10, 8, 3, nan, 0.2, 0.5), (0, 10, 8, 3, inf, 0.2, 0.5),
                (0, 10, 8, 3, 0.1, nan, 0.5), (0, 10, 8, 3, 0.1, -inf, 0.5),
                (0, 10, 8, 3, 0.1, 0.2, nan), (0, 10, 8, 3, 0.1, 0.2, inf),
                (-1, 10, 8, 3, 0.1, 0.2, 0.5), (0, 593, 8, 3, 0.1, 0.2, 0.5)]:
        assert call([good, bad]) == csm.CSM_EINVAL, bad


# ------------------------------------------------------------ matcher entry --
YAW_BUILDS = {"device": None, "host": "CSM_YAW_HOST_BUILD", "retry": "CSM_YAW_FORCE_RETRY"}
IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))


def quat_x(theta):
    return (math.cos(0.5 * theta), math.sin(0.5 * theta), 0.0, 0.0)


def qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])


def compose(a, b):
    """Rigid transform a * b, each ((t), (w, x, y, z))."""
    t = transform(np.asarray([b[0]], np.float64), a[0], a[1])[0]
    return tuple(float(v) for v in t), qmul(a[1], b[1])


# (node pose, submap pose, gravity alignment). The submap holds the cloud at
# ((0.2, 0.1, 0), yaw 0.15); each node pose is the submap pose times a guess
# near that, so a match exists inside Match's window. "yaw": global poses
# about z; "tilt": a submap pose (and with it the node pose) tilted about x,
# and a gravity alignment tilted about x and y; "full+" / "full-": node yaw
# 3.1 and -3.1 for MatchFullSubmap, the latter over a slightly tilted submap.
TILTED_GRAVITY = (math.cos(0.02), 0.6 * math.sin(0.02), 0.8 * math.sin(0.02), 0.0)
GUESS = ((0.25, 0.05, 0.05), quat_z(0.1))
SUBMAP_YAW = ((-0.1, 0.1, 0.0), quat_z(-0.05))
SUBMAP_TILT = ((-0.1, 0.1, 0.02), qmul(quat_x(0.03), quat_z(-0.05)))
SUBMAP_FULL_TILT = ((0.0, 0.0, 0.0), quat_x(0.003))
POSES = {
    "yaw": (compose(SUBMAP_YAW, GUESS), SUBMAP_YAW, (math.cos(0.01), math.sin(0.01), 0.0, 0.0)),
    "tilt": (compose(SUBMAP_TILT, GUESS), SUBMAP_TILT, TILTED_GRAVITY),
    "full+": (((0.0, 0.0, 0.0), quat_z(3.1)), IDENTITY,
              (math.cos(0.01), math.sin(0.01), 0.0, 0.0)),
    "full-": (compose(SUBMAP_FULL_TILT, ((0.0, 0.0, 0.0), quat_z(-3.1))), SUBMAP_FULL_TILT,
              TILTED_GRAVITY),
}
# (histogram size, Match's angular window in steps or None for MatchFullSubmap,
# poses): 2A + 1 = 63, 65, 255 and 257 for Match; the full-submap window is
# round(pi / astep) for this cloud.
CASES = [(7, 31, "yaw"), (13, 32, "tilt"), (120, 127, "tilt"), (127, 128, "yaw"),
         (13, None, "full+"), (127, None, "full-"), (7, None, "full-")]
CASE_IDS = [f"{n}-{'full' if a is None else a}-{p}" for n, a, p in CASES]


class World:
    """The grid and cloud of test_fast3d_gpu.py's test_rotational_filter_and_poses
    and, built once each, the matchers and the oracle's discrete scans of
    every case."""

    def __init__(self, csm, oracle):
        self.csm, self.oracle = csm, oracle
        rng = np.random.default_rng(3)
        cloud = np.concatenate([TEST_CLOUD,
                                rng.uniform(-6, 6, (200, 3)).astype(np.float32) * [1, 1, 0.3]])
        self.cloud = cloud.astype(np.float32)
        placed = transform(self.cloud, (0.2, 0.1, 0.0), quat_z(0.15))
        self.og = oracle.hybrid_grid(0.05)
        self.og.insert((0.2, 0.1, 0.0), placed, 0.7, 0.4, 5)
        self.g = gpu_grid(csm, self.og)
        self.hists = {n: (oracle.histogram(placed, n), oracle.histogram(self.cloud, n))
                      for n in (7, 13, 120, 127)}
        self.matchers, self.refs = {}, {}
        probe = self.matcher(7, 0.3, 0.0)[1]
        self.astep = F32(csm.discrete_scans_3d(probe, self.node(7, "yaw"), *POSES["yaw"][:2])[2])

    def node(self, size, poses):
        return self.csm.NodeData3D(self.cloud, self.cloud[::3], self.hists[size][1], POSES[poses][2])

    def matcher(self, size, angular_search_window, min_rotational_score):
        key = (size, angular_search_window, min_rotational_score)
        if key not in self.matchers:
            o = options(self.csm, 7, 3, min_rotational_score=min_rotational_score,
                        linear_xy_search_window=0.4, linear_z_search_window=0.2,
                        angular_search_window=angular_search_window)
            om = self.oracle.fast3d(self.og, self.og, self.hists[size][0], opt_tuple(o))
            gm = self.csm.FastCorrelativeScanMatcher3D(self.g, self.g, self.hists[size][0], o)
            self.matchers[key] = (om, gm)
        return self.matchers[key]

    def case(self, size, steps, poses, equality):
        """(gpu matcher, oracle matcher, node, poses, full_submap, oracle's
        discrete scans, min_rotational_score): the last is 0 or, for
        `equality`, one of the oracle's own unfiltered scores."""
        full = steps is None
        ang = 0.3 if full else (steps + 0.25) * float(self.astep)
        node = self.node(size, poses)
        node_pose, submap_pose = POSES[poses][:2]
        min_rot = 0.0
        if equality:
            scores = self.case(size, steps, poses, False)[5]["scores"]
            min_rot = float(np.float64(np.sort(scores)[3 * len(scores) // 4]))  # the top quarter
        om, gm = self.matcher(size, ang, min_rot)
        key = (size, steps, poses, equality)
        if key not in self.refs:
            self.refs[key] = om.discrete_scans(node_pose, submap_pose, node, full)
        return gm, om, node, (node_pose, submap_pose), full, self.refs[key], min_rot


@pytest.fixture(scope="module")
def world(csm, oracle):
    return World(csm, oracle)


@pytest.mark.parametrize("yaw_build", list(YAW_BUILDS))
@pytest.mark.parametrize("equality", [False, True], ids=["min0", "equal"])
@pytest.mark.parametrize("size,steps,poses", CASES, ids=CASE_IDS)
def test_discrete_scans_are_the_oracles(world, size, steps, poses, equality, yaw_build,
                                        monkeypatch):
    if YAW_BUILDS[yaw_build]:
        monkeypatch.setenv(YAW_BUILDS[yaw_build], "1")
    gm, om, node, (node_pose, submap_pose), full, ref, min_rot = world.case(size, steps, poses,
                                                                           equality)
    scans, window, astep, yaw0 = world.csm.discrete_scans_3d(gm, node, node_pose, submap_pose, full)
    assert bits(F32(astep)) == bits(ref["step"]) == bits(world.astep)
    assert window == ref["window"]
    if not full:
        assert window == steps
    else:
        assert 2 * window + 1 > 768
    if equality:  # the chosen score itself passes, and some yaw does not
        assert 0 < len(ref["k"]) < 2 * window + 1
        assert np.float64(ref["score"].min()) == min_rot
    else:
        assert len(ref["k"]) == 2 * window + 1
    assert len(scans) == len(ref["k"])
    assert np.array_equal(scans["k"], ref["k"])
    assert np.array_equal(bits(scans["rotational_score"]), bits(ref["score"]))
    for field in ("q", "n", "t"):
        bad = np.nonzero(np.any(bits(scans[field]) != bits(ref[field]), axis=1))[0]
        assert len(bad) == 0, (field, scans["k"][bad[:4]], scans[field][bad[:4]], ref[field][bad[:4]])
    # The unfiltered scores behind the filter: the raw entry on the same inputs.
    raw, _, _, _ = world.csm.rotational_scores_batch(
        np.concatenate([world.hists[size][1], world.hists[size][0]]),
        [(0, size, size, window, astep, yaw0, 0.0)])
    assert np.array_equal(bits(raw[0]), bits(ref["scores"]))


@pytest.mark.parametrize("yaw_build", list(YAW_BUILDS))
def test_undecided_rounding_is_patched(world, yaw_build, monkeypatch):
    """The cloud scaled by 1.22 has angular step 0.0048460593, and at yaw 415
    of MatchFullSubmap's 1297 a double sin or cos lies 2^-43 (relative) from
    a float rounding boundary: inside yaw_build's 2^-40 margin, so the device
    flags the yaw, the deferred pass runs again and the host patches that
    record in. Every record, the patched one included, is the oracle's."""
    if YAW_BUILDS[yaw_build]:
        monkeypatch.setenv(YAW_BUILDS[yaw_build], "1")
    om, gm = world.matcher(13, 0.3, 0.0)
    cloud = (world.cloud * F32(1.22)).astype(np.float32)
    node_pose, submap_pose, gravity = POSES["full+"]
    node = world.csm.NodeData3D(cloud, cloud[::3], world.hists[13][1], gravity)
    ref = om.discrete_scans(node_pose, submap_pose, node, True)
    margins = rounding_margins(ref["window"], ref["step"])
    assert ref["window"] == 648 and int(np.argmin(margins)) == 415
    assert margins[415] < 2.0 ** -42 and len(ref["k"]) == 1297
    scans, window, astep, _ = world.csm.discrete_scans_3d(gm, node, node_pose, submap_pose, True)
    assert window == 648 and bits(F32(astep)) == bits(ref["step"])
    assert np.array_equal(scans["k"], ref["k"])
    assert np.array_equal(bits(scans["rotational_score"]), bits(ref["score"]))
    for field in ("q", "n", "t"):
        bad = np.nonzero(np.any(bits(scans[field]) != bits(ref[field]), axis=1))[0]
        assert len(bad) == 0, (field, scans["k"][bad[:4]], scans[field][bad[:4]], ref[field][bad[:4]])


@pytest.mark.parametrize("size,steps,poses", [(7, 31, "yaw"), (13, 32, "tilt"), (127, 128, "yaw"),
                                              (13, None, "full+"), (127, None, "full-"),
                                              (7, None, "full-")],
                         ids=["7-match", "13-match", "127-match", "13-full", "127-full", "7-full"])
def test_whole_matches_at_other_histogram_sizes(world, size, steps, poses):
    """Match and MatchFullSubmap end to end with 7, 13 and 127 buckets."""
    gm, om, node, (node_pose, submap_pose), full, scans, _ = world.case(size, steps, poses, True)
    if full:
        ref = om.match_full_submap(node_pose[1], submap_pose[1], node, 0.3)
        gpu = gm.MatchFullSubmap(node_pose[1], submap_pose[1], node, 0.3)
    else:
        ref = om.match(node_pose, submap_pose, node, 0.3)
        gpu = gm.Match(node_pose, submap_pose, node, 0.3)
    assert ref["num_discrete_scans"] == len(scans["k"]) > 0
    assert_same_result(gpu, ref, om, full, node_pose, submap_pose, node)
