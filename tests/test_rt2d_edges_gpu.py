"""RealTimeCorrelativeScanMatcher2D at the edges of today's rt2d.hip, against
the oracle.

rt2d_score is a software-pipelined gather kernel: a workgroup is (rotation,
y offset, chunk of 64 x offsets), a lane is one x offset, and the points are
summed in batches of kDepth (32; 8 or 16 by CSM_RT2D_DEPTH), two batches in
flight, with two partial tails. The host keeps the converted, padded grid of
the previous call (EnsureGrid) and reduces one key per workgroup. The cases
(rt2d_edges_support.py) sit where that can go wrong:

1. cloud sizes at and next to multiples of 32 and 64, on non-square grids
   with the cloud straddling every border;
2. the winner on the first and the last lane, in a last chunk of one valid
   lane, in the first and the last rotation;
3. exact ties, where only the (scan, x, y) order decides;
4. every term of the cache's reuse test, one change at a time;
5. the kernels selected by CSM_RT2D_DEPTH and CSM_RT2D_HOSTKEYS, each in a
   fresh process;
6. the early refusals.

Comparison rule. With both cost weights 0 the penalty factor is exp(-0) = 1
on host and device and the sums run in point order: the float32 score and the
pose are equal. With weights, test_rt2d_gpu.py's rule: 1e-6 relative on the
score, the pose equal; such cases are used only where the oracle's runner-up
over the whole window is at least 1e-4 relative below its best, so a last-ulp
exp difference cannot move the argmax.

The test_sanity_* tests need no GPU: they show from the oracle alone that the
cases are what they claim to be.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rt2d_edges_support as S

gpu = pytest.mark.gpu

BATCH = {c.name: c for c in S.batch_cases()}
TIES = {c.name: c for c in S.tie_cases()}
EXTREME_IDS = [f"L{L}-x{sx:+d}-y{sy:+d}-r{sr:+d}" for L in S.EX_LS for sx, sy, sr in S.EX_CORNERS]
EXTREME_ARGS = [(L,) + c for L in S.EX_LS for c in S.EX_CORNERS]

_extremes = {}


def _extreme(oracle, args):
    if args not in _extremes:
        _extremes[args] = S.extreme_case(oracle, *args)
    return _extremes[args]


_cache_steps = []


def _steps(oracle):
    if not _cache_steps:
        _cache_steps.extend(S.cache_steps(oracle))
    return _cache_steps


def _margin(oracle, case, distinct=False):
    """Relative gap between the oracle's best candidate and its runner-up over
    the whole window (distinct: the best score strictly below the maximum).
    Checks on the way that ScoreCandidates over the window and Match agree."""
    scores, cands, (L, na, step) = S.window_scores(oracle, case)
    ref_score, ref_pose, _ = S.reference(oracle, case)
    first = int(np.argmax(scores))  # the first maximum, as std::max_element
    assert scores[first] == np.float32(ref_score)
    assert S.candidate_pose(case, cands[first], na, step) == ref_pose
    s = np.sort(scores.astype(np.float64))[::-1]
    runner_up = s[s < s[0]][0] if distinct else s[1]
    return (s[0] - runner_up) / s[0], scores


# ---- oracle-only sanity (no GPU) --------------------------------------------

def test_sanity_batch_clouds_straddle_the_limits():
    """From 31 points on, each section-1 cloud has points beyond each of the
    four borders at the initial pose, and points inside."""
    x0, y0, t0 = S.INITIAL
    for n in S.SIZES:
        for weighted in (False, True):
            p = S.straddling_cloud(n, (2000 if weighted else 1000) + n).astype(np.float64)
            wx = x0 + math.cos(t0) * p[:, 0] - math.sin(t0) * p[:, 1]
            wy = y0 + math.sin(t0) * p[:, 0] + math.cos(t0) * p[:, 1]
            lo_x, lo_y = S.LIMITS[1] - S.NY * S.RES, S.LIMITS[2] - S.NX * S.RES
            m = S.WINDOW[0]  # farther from the border than the linear window reaches
            sides = [np.sum(wx > S.LIMITS[1] + m), np.sum(wx < lo_x - m),
                     np.sum(wy > S.LIMITS[2] + m), np.sum(wy < lo_y - m)]
            inside = np.sum((wx > lo_x + m) & (wx < S.LIMITS[1] - m) &
                            (wy > lo_y + m) & (wy < S.LIMITS[2] - m))
            if n >= 31:
                assert min(sides) >= 1 and inside >= 3, (n, sides, inside)
    assert {len(c.cloud) for c in BATCH.values()} == set(S.SIZES)


def test_sanity_weighted_cases_have_a_margin(oracle):
    """The weighted cases' runner-up is at least 1e-4 relative below the best."""
    weighted = [c for c in BATCH.values() if not c.exact]
    assert len(weighted) == len(S.KINDS) * len(S.WEIGHTED_SIZES)
    for case in weighted:
        margin, _ = _margin(oracle, case)
        print(case.name, "margin", margin)
        assert margin >= 1e-4, (case.name, margin)


@pytest.mark.parametrize("args", EXTREME_ARGS, ids=EXTREME_IDS)
def test_sanity_extreme_winners(oracle, args):
    """The oracle's winner is the intended corner of the window in the first
    or last rotation: pose - initial == (-yo * res, -xo * res, -+na * step)."""
    L = args[0]
    case, (r, xo, yo), na, step = _extreme(oracle, args)
    score, pose, ncand = S.reference(oracle, case)
    assert na >= 1 and ncand == (2 * na + 1) * (2 * L + 1) ** 2  # L as intended
    assert (abs(xo), abs(yo)) == (L, L) and r in (0, 2 * na)
    assert len(case.cloud) <= 65
    assert pose[0] - case.initial[0] == -yo * S.EX_RES
    assert pose[1] - case.initial[1] == -xo * S.EX_RES
    assert pose[2] == case.initial[2] + (r - na) * step
    assert abs(score - 0.9) < 1e-6  # every point on the wall


def test_sanity_tie_poses(oracle):
    """The tie cases' winners, derived by hand, are the oracle's."""
    step, na = S.tie_step()
    assert na == 3
    for case in TIES.values():
        score, pose, ncand = S.reference(oracle, case)
        L = math.ceil(case.opts[0] / S.RES)
        assert ncand == (2 * na + 1) * (2 * L + 1) ** 2, case.name
        if case.name.endswith("-small"):
            continue
        assert pose == S.tie_expected_pose(case), case.name
        if L > 3:
            assert L == 32  # two chunks of x offsets
            continue
        scores = S.window_scores(oracle, case)[0]
        tied = int(np.sum(scores == scores.max()))
        wt, wr = case.opts[2:]
        if case.exact:
            assert tied == ncand
        else:
            # Offset (0, 0) of every scan, or every offset of the centre scan.
            assert tied == (2 * na + 1 if wt > 0 else (2 * L + 1) ** 2), case.name
            assert _margin(oracle, case, distinct=True)[0] >= 1e-4, case.name
    # The issue's numbers for x and y at this window, resolution and initial pose.
    assert S.tie_expected_pose(TIES["tie-prob-0-0"])[:2] == (0.55, 0.85)
    assert S.tie_expected_pose(TIES["tie-prob-1-0"])[:2] == (0.4, 0.7)
    assert S.tie_expected_pose(TIES["tie-prob-0-1"]) == (0.55, 0.85, 0.1)
    # Grid smaller than the window: the first candidates read the outside
    # value, and the winner is a later one that keeps every point inside.
    small, full = TIES["tie-prob-0-0-small"], TIES["tie-prob-0-0"]
    scores, cands, (L, na_, step_) = S.window_scores(oracle, small)
    first_all_inside = int(np.argmax(scores == np.float32(S.reference(oracle, full)[0])))
    assert first_all_inside > 0 and scores[0] < scores[first_all_inside] == scores.max()
    assert S.reference(oracle, small)[1] == S.candidate_pose(small, cands[first_all_inside],
                                                             na_, step_)


def test_sanity_cache_steps_differ(oracle):
    """Consecutive steps of the cache sequence differ in the oracle's result
    (score bits or pose): a converted grid reused by mistake cannot pass."""
    steps = _steps(oracle)
    assert len(steps) == 12
    for (la, a, _), (lb, b, _) in zip(steps, steps[1:]):
        ra, rb = S.reference(oracle, a), S.reference(oracle, b)
        assert np.float32(ra[0]) != np.float32(rb[0]) or ra[1] != rb[1], (la, lb)
    assert all(case.exact for _, case, _ in steps)


# ---- 1. batch boundaries ----------------------------------------------------

@gpu
@pytest.mark.parametrize("name", list(BATCH))
def test_batch_boundaries(csm, oracle, name):
    """n at and next to multiples of 32 and 64: nfull changes parity, and each
    of the two tails is empty, partial, full or has a negative count."""
    case = BATCH[name]
    S.check(case, *case.match(csm), S.reference(oracle, case))


# ---- 2. the winner at the extremes of the mapping ---------------------------

@gpu
@pytest.mark.parametrize("args", EXTREME_ARGS, ids=EXTREME_IDS)
def test_winner_at_extremes(csm, oracle, args):
    """Sides 63, 65 and 129: the winner on lane 0 of the first chunk or on the
    last valid lane (alone in its chunk for 65 and 129), on the first or the
    last y row, in the first or the last rotation."""
    case = _extreme(oracle, args)[0]
    sp = csm.SearchParameters(case.opts[0], case.opts[1], case.cloud, case.limits[0])
    assert sp._c.num_linear_perturbations == args[0]
    S.check(case, *case.match(csm), S.reference(oracle, case))


# ---- 3. exact ties ----------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", list(TIES))
def test_ties(csm, oracle, name):
    """Uniform grids: the first maximum in (scan, x, y) order wins, within a
    wave, across the workgroups' keys, and across chunks and rows at L = 32."""
    case = TIES[name]
    score, pose = case.match(csm)
    S.check(case, score, pose, S.reference(oracle, case))
    if not name.endswith("-small"):
        assert pose == S.tie_expected_pose(case)


# ---- 4. the converted-grid cache --------------------------------------------

@gpu
def test_cache_sequence(csm, oracle):
    """One Context, one cloud and initial pose; each Match differs from the
    one before in one term of EnsureGrid's reuse test (cells, P, prob/TSDF,
    weight cells, truncation, max_weight, device id, dims). The window is a
    matcher option, so the wider window is a second matcher on the Context."""
    ctx = csm.Context(0)
    matchers, device_grids = {}, []
    try:
        for label, case, on_device in _steps(oracle):
            grid = case.grid(csm)
            if on_device:
                grid = csm.DeviceProbabilityGrid.from_host(grid, ctx)
                device_grids.append(grid)
            if case.opts not in matchers:
                matchers[case.opts] = csm.RealTimeCorrelativeScanMatcher2D(
                    csm.RealTimeCorrelativeScanMatcherOptions(*case.opts), ctx)
            print(label)
            score, pose = matchers[case.opts].Match(case.initial, case.cloud, grid)
            S.check(case, score, pose, S.reference(oracle, case))
        assert len(matchers) == 2
    finally:
        for g in device_grids:
            g.close()
        ctx.close()


@gpu
def test_score_candidates_after_a_wide_match(csm, oracle):
    """ScoreCandidates keeps the cached padding P: right after a wide-window
    Match and on a fresh Context it gives the same scores, the oracle's."""
    case = _steps(oracle)[0][1]
    opts = S.CACHE_WINDOW + (0.1, 0.1)
    grid = case.grid(csm)
    sp = csm.SearchParameters(opts[0], opts[1], case.cloud, S.RES)
    d = csm.DiscretizeScans(grid.limits(), csm.GenerateRotatedScans(case.cloud, sp),
                            case.initial[:2])
    rng = np.random.RandomState(17)
    # Offsets reach past the window, the padding and the grid.
    cands = [(int(rng.randint(0, sp.num_scans)), int(rng.randint(-45, 46)),
              int(rng.randint(-45, 46))) for _ in range(500)]
    ref = oracle.rt2d_score_candidates(
        case.limits + (grid.num_x_cells, grid.num_y_cells), case.cells, opts[2], opts[3], d,
        sp.num_angular_perturbations, sp.angular_perturbation_step_size, cands)
    got = []
    for wide_first in (True, False):
        ctx = csm.Context(0)
        try:
            if wide_first:
                csm.RealTimeCorrelativeScanMatcher2D(
                    csm.RealTimeCorrelativeScanMatcherOptions(*S.CACHE_WIDE, 0.0, 0.0),
                    ctx).Match(case.initial, case.cloud, grid)
            m = csm.RealTimeCorrelativeScanMatcher2D(
                csm.RealTimeCorrelativeScanMatcherOptions(*opts), ctx)
            got.append(m.ScoreCandidates(grid, d, sp, [csm.Candidate2D(*c, sp) for c in cands]))
        finally:
            ctx.close()
    assert np.array_equal(got[0], got[1])
    # The rule of test_search_space.py.
    assert np.allclose(got[0], ref, rtol=1e-6, atol=0.0)
    assert np.mean(got[0] == ref) > 0.99
    assert 50 < np.sum(ref > np.float32(0.1)) < 500  # inside and outside lookups


# ---- 5. environment variants ------------------------------------------------

@gpu
def test_environment_variants(oracle):
    """rt2d_score<., 8>, rt2d_score<., 16> and the device atomicMax path: the
    variables are read once per process, so each runs in a fresh child, one
    after another; a child that fails or times out ends the test."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rt2d_edges_child.py")
    cases = S.child_cases()
    for var, value in (("CSM_RT2D_DEPTH", "8"), ("CSM_RT2D_DEPTH", "16"),
                       ("CSM_RT2D_HOSTKEYS", "0")):
        env = {k: v for k, v in os.environ.items()
               if k not in ("CSM_RT2D_DEPTH", "CSM_RT2D_HOSTKEYS")}
        env[var] = value
        p = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, f"{var}={value}: exit {p.returncode}\n{p.stderr[-2000:]}"
        out = json.loads(p.stdout.strip().splitlines()[-1])
        assert [o["name"] for o in out] == [c.name for c in cases]
        print(f"{var}={value}")
        for case, o in zip(cases, out):
            score = float(np.array(o["bits"], np.uint32).view(np.float32))
            S.check(case, score, tuple(o["pose"]), S.reference(oracle, case))


# ---- 6. refusals ------------------------------------------------------------

@gpu
def test_refusals(csm):
    """Returned before any GPU work: L > 4096 and a padded grid above 2^27
    cells are CSM_ERANGE, an empty cloud CSM_EINVAL."""
    cloud = S.tie_cloud()

    def match(lin, shape, pts):
        m = csm.RealTimeCorrelativeScanMatcher2D(
            csm.RealTimeCorrelativeScanMatcherOptions(lin, 0.1, 0.0, 0.0))
        grid = csm.ProbabilityGrid(0.5, 10.0, 10.0, np.full(shape, 100, np.uint16))
        return m.Match((5.0, 5.0, 0.0), pts, grid)

    assert match(1.0, (23, 37), cloud)[0] > 0.0  # the same call within range
    with pytest.raises(csm.CsmError, match=rf"\({csm.CSM_ERANGE}\)"):
        match(4097 * 0.5, (23, 37), cloud)  # L = 4097
    with pytest.raises(csm.CsmError, match=rf"\({csm.CSM_ERANGE}\)"):
        match(4000 * 0.5, (200, 200), cloud)  # (200 + 2 * 8001)^2 > 2^27
    with pytest.raises(csm.CsmError, match=rf"\({csm.CSM_EINVAL}\)"):
        match(1.0, (23, 37), np.zeros((0, 3), np.float32))
