"""Cases of tests/test_rt2d_edges_gpu.py and its child script: small grids,
clouds and windows placed at the batch, lane, chunk, rotation and cache edges
of the real-time 2D matcher (csrc/rt2d.hip).

Everything here is deterministic. The section-1 and tie cases are plain numpy,
so the child process can rebuild them without the oracle; the cases that plant
a winner (extremes, cache sequence) ask the oracle for the angular step and
for the cells the winning candidate reads.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

# Section 1: a non-square grid (23 rows x 37 columns) around the initial pose.
RES = 0.05
LIMITS = (RES, 1.0, 1.6)  # x in (-0.15, 1.0], y in (-0.25, 1.6]
NX, NY = 37, 23
INITIAL = (0.4, 0.7, 0.1)
WINDOW = (0.15, 0.2)  # +-3 cells, +-0.2 rad
TRUNCATION, MAX_WEIGHT = 0.3, 10.0
# At and next to every multiple of the pipeline batch (32) and of the two
# batches in flight (64); 31..33 and 63..65 are also next to multiples of the
# optional batches of 8 and 16.
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129)
WEIGHTED_SIZES = (33, 96, 129)
KINDS = ("prob", "tsdf")


@dataclass
class Case:
    name: str
    kind: str                       # "prob" or "tsdf"
    limits: Tuple[float, float, float]
    cells: np.ndarray               # (ny, nx) uint16; the TSD cells of a TSDF
    opts: Tuple[float, float, float, float]  # lin, ang, wt, wr
    initial: Tuple[float, float, float]
    cloud: np.ndarray
    weights: Optional[np.ndarray] = None
    truncation: float = TRUNCATION
    max_weight: float = MAX_WEIGHT

    @property
    def exact(self):
        """Both cost weights 0: exp(-0) = 1 on host and device, scores equal."""
        return self.opts[2] == 0.0 and self.opts[3] == 0.0

    def grid(self, csm):
        if self.kind == "tsdf":
            return csm.TSDF2D(*self.limits, self.cells, self.weights, self.truncation,
                              self.max_weight)
        return csm.ProbabilityGrid(*self.limits, self.cells)

    def match(self, csm, context=None):
        m = csm.RealTimeCorrelativeScanMatcher2D(
            csm.RealTimeCorrelativeScanMatcherOptions(*self.opts), context)
        return m.Match(self.initial, self.cloud, self.grid(csm))


_refs = {}


def reference(oracle, case):
    """(score, pose, num_candidates) of the oracle, computed once per case."""
    if case.name not in _refs:
        if case.kind == "tsdf":
            _refs[case.name] = oracle.rt2d_match_tsdf(
                case.limits, case.cells, case.weights, case.truncation, case.max_weight,
                case.opts, case.initial, case.cloud)
        else:
            _refs[case.name] = oracle.rt2d_match(case.limits, case.cells, case.opts,
                                                 case.initial, case.cloud)
    return _refs[case.name]


def check(case, score, pose, ref):
    """The comparison rule: an equal float32 score without cost weights, the
    project's 1e-6 relative with them (double exp on OCML against glibc); the
    pose equal in both."""
    ref_score, ref_pose, _ = ref
    print(f"{case.name}: score {score!r} ref {ref_score!r} pose {pose} ref {ref_pose}")
    if case.exact:
        assert np.float32(score) == np.float32(ref_score), case.name
    else:
        assert abs(score - ref_score) <= 1e-6 * abs(ref_score), case.name
    assert tuple(pose) == tuple(ref_pose), case.name


def window_scores(oracle, case):
    """Every candidate of the case's window scored by the oracle's
    ScoreCandidates, in (scan, x, y) order: (scores, candidates (k, 3),
    (L, num_angular, step)). L is read back from the oracle's candidate count."""
    _, _, ncand = reference(oracle, case)
    ns, _, d, step = oracle.discretize(case.limits, case.cells, case.initial, case.opts[0],
                                       case.opts[1], case.cloud, rotated_sp=True)
    side = math.isqrt(ncand // ns)
    assert ns * side * side == ncand and side % 2 == 1 and ns % 2 == 1
    L, na = (side - 1) // 2, (ns - 1) // 2
    offs = np.arange(-L, L + 1)
    cands = np.stack(np.meshgrid(np.arange(ns), offs, offs, indexing="ij"), -1).reshape(-1, 3)
    ny, nx = case.cells.shape
    scores = oracle.rt2d_score_candidates(
        case.limits + (nx, ny), case.cells, case.opts[2], case.opts[3], d, na, step, cands,
        tsdf=None if case.kind == "prob" else (case.weights, case.truncation, case.max_weight))
    return scores, cands, (L, na, step)


def candidate_pose(case, cand, na, step):
    """Candidate2D and the pose update of Match, in its double arithmetic."""
    r, xo, yo = (int(v) for v in cand)
    res = case.limits[0]
    return (case.initial[0] + -yo * res, case.initial[1] + -xo * res,
            case.initial[2] + (r - na) * step)


def winner_cells(oracle, case):
    """Cells (x, y) inside the limits that the oracle's winning candidate reads."""
    scores, cands, _ = window_scores(oracle, case)
    r, xo, yo = (int(v) for v in cands[int(np.argmax(scores))])
    _, _, d, _ = oracle.discretize(case.limits, case.cells, case.initial, case.opts[0],
                                   case.opts[1], case.cloud, rotated_sp=True)
    ny, nx = case.cells.shape
    hit = d[r] + np.array([xo, yo])
    return [(int(x), int(y)) for x, y in hit if 0 <= x < nx and 0 <= y < ny]


# ---- section 1: batch boundaries -------------------------------------------

def prob_cells(seed, nx=NX, ny=NY):
    """Random cells in 1..32767, about a fifth unknown (0)."""
    rng = np.random.RandomState(seed)
    cells = rng.randint(1, 32768, (ny, nx)).astype(np.uint16)
    cells[rng.uniform(size=(ny, nx)) < 0.2] = 0
    return cells


def tsdf_planes(seed, nx=NX, ny=NY):
    """Random TSD and weight planes; about a fifth of the weights 0."""
    rng = np.random.RandomState(seed)
    tsd = rng.randint(1, 32768, (ny, nx)).astype(np.uint16)
    wgt = rng.randint(1, 32768, (ny, nx)).astype(np.uint16)
    wgt[rng.uniform(size=(ny, nx)) < 0.2] = 0
    return tsd, wgt


def straddling_cloud(n, seed):
    """n points spread past the limits of the section-1 grid on every side
    when placed at INITIAL: from 8 points on, four of them are put beyond the
    four borders, at shuffled positions of the list."""
    rng = np.random.RandomState(seed)
    xy = rng.uniform([-0.8, -1.2], [0.8, 1.2], (n, 2))
    if n >= 8:
        xy[:4] = np.array([[0.85, 0.1], [-0.85, -0.1], [0.05, 1.25], [-0.05, -1.25]]) + \
            rng.uniform(-0.03, 0.03, (4, 2))
        xy = xy[rng.permutation(n)]
    elif n == 2:
        xy[0], xy[1] = (0.1, -0.2), (0.05, 1.25)  # one inside, one outside
    return np.concatenate([xy, np.zeros((n, 1))], 1).astype(np.float32)


def batch_case(kind, n, weighted=False):
    seed = (2000 if weighted else 1000) + n
    cloud = straddling_cloud(n, seed)
    opts = WINDOW + ((0.1, 0.1) if weighted else (0.0, 0.0))
    name = f"batch-{kind}-{n}" + ("-weighted" if weighted else "")
    if kind == "tsdf":
        tsd, wgt = tsdf_planes(7)
        return Case(name, kind, LIMITS, tsd, opts, INITIAL, cloud, wgt)
    return Case(name, kind, LIMITS, prob_cells(5), opts, INITIAL, cloud)


def batch_cases():
    return [batch_case(k, n) for k in KINDS for n in SIZES] + \
        [batch_case(k, n, weighted=True) for k in KINDS for n in WEIGHTED_SIZES]


# ---- section 3: exact ties --------------------------------------------------

TIE_ANGULAR_WINDOW = 0.7
TIE_VALUE, TIE_WEIGHT = 12345, 23456


def tie_cloud():
    """40 points within 0.14 m of the origin: below the 3 * resolution floor
    of SearchParameters' max range, so the angular step follows from the
    resolution alone (tie_step)."""
    rng = np.random.RandomState(40)
    r, a = rng.uniform(0.01, 0.14, 40), rng.uniform(-math.pi, math.pi, 40)
    return np.stack([r * np.cos(a), r * np.sin(a), np.zeros(40)], 1).astype(np.float32)


def tie_step(res=RES):
    """SearchParameters (correlative_scan_matcher_2d.cc:27-47) for a cloud
    whose ranges stay under max_scan_range = 3.f * resolution."""
    max_range = np.float32(3.0 * res)  # a float, and so is its square
    step = (1. - 1e-3) * math.acos(1. - res * res / (2. * float(max_range * max_range)))
    return step, math.ceil(TIE_ANGULAR_WINDOW / step)


def tie_case(kind, wt, wr, lin=0.15, shape=(NY, NX), limits=LIMITS, initial=INITIAL, tag=""):
    """A uniform grid: every candidate of a window reads the same values."""
    name = f"tie-{kind}-{wt:g}-{wr:g}{tag}"
    opts = (lin, TIE_ANGULAR_WINDOW, wt, wr)
    cells = np.full(shape, TIE_VALUE, np.uint16)
    wgt = np.full(shape, TIE_WEIGHT, np.uint16) if kind == "tsdf" else None
    return Case(name, kind, limits, cells, opts, initial, tie_cloud(), wgt)


TIE_WEIGHTS = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
# 31.5 cells: rounds up to L = 32 whatever 1.575 / 0.05 gives in its last bit.
TIE_WIDE = dict(lin=1.575, shape=(83, 97), limits=(RES, 2.5, 3.1), tag="-L32")
# 9 x 7 cells around the initial pose under a +-8-cell window.
TIE_SMALL = dict(lin=0.4, shape=(7, 9), limits=(RES, 0.6, 0.9), tag="-small")


def tie_cases():
    return [tie_case(k, wt, wr) for k in KINDS for wt, wr in TIE_WEIGHTS] + \
        [tie_case("prob", 0.0, 0.0, **TIE_WIDE), tie_case("prob", 0.0, 0.0, **TIE_SMALL)]


def tie_expected_pose(case):
    """By hand: without weights the first candidate (scan 0, x offset -L,
    y offset -L); with a translation weight offset (0, 0) of the first scan;
    with a rotation weight offset (-L, -L) of the centre scan."""
    res = case.limits[0]
    L = math.ceil(case.opts[0] / res)
    step, na = tie_step(res)
    x0, y0, t0 = case.initial
    wt, wr = case.opts[2:]
    x, y = (x0, y0) if wt > 0 else (x0 + L * res, y0 + L * res)
    return (x, y, t0 if wr > 0 else t0 + (0 - na) * step)


# ---- section 2: the winner at the extremes of the mapping -------------------

EX_RES = 0.5
EX_NX, EX_NY = 41, 29
EX_LIMITS = (EX_RES, EX_NY * EX_RES, EX_NX * EX_RES)
EX_ANGULAR_WINDOW = 0.4
EX_THETA0 = 0.3
EX_TRUTH = (8.0, 12.0)
# An L-shaped wall, legs of 7 and 6 cells, as (x, y) cell indices.
EX_WALL = [(x, 10) for x in range(14, 21)] + [(14, y) for y in range(11, 17)]
EX_LS = (31, 32, 64)  # sides 63, 65, 129: one, two and three chunks of 64
EX_CORNERS = [(sx, sy, sr) for sx in (-1, 1) for sy in (-1, 1) for sr in (-1, 1)]


def extreme_case(oracle, L, sx, sy, sr):
    """The wall's cells hold probability 0.9 on an unknown grid, and the cloud
    is the wall seen from the true pose. The initial pose is displaced so that
    the true pose is candidate (x offset sx * L, y offset sy * L) of the first
    (sr = -1) or last (sr = +1) rotation. Returns (case, winner (r, xo, yo),
    num_angular, step)."""
    cells = np.zeros((EX_NY, EX_NX), np.uint16)
    wall = np.array(EX_WALL)
    cells[wall[:, 1], wall[:, 0]] = 1
    # Cell centres in the world: x runs against the y index, y against x.
    world = np.stack([EX_LIMITS[1] - (wall[:, 1] + 0.5) * EX_RES,
                      EX_LIMITS[2] - (wall[:, 0] + 0.5) * EX_RES], 1)
    xo, yo = sx * L, sy * L
    initial = (EX_TRUTH[0] + yo * EX_RES, EX_TRUTH[1] + xo * EX_RES, EX_THETA0)
    opts = (L * EX_RES, EX_ANGULAR_WINDOW, 0.0, 0.0)
    # The step depends on the cloud's largest float range and the cloud on the
    # true angle, initial + (r - num_angular) * step: two rounds settle it.
    theta, na, step = EX_THETA0, 0, 0.0
    for _ in range(3):
        c, s = math.cos(-theta), math.sin(-theta)
        rel = world - np.array(EX_TRUTH)
        local = np.stack([c * rel[:, 0] - s * rel[:, 1], s * rel[:, 0] + c * rel[:, 1],
                          np.zeros(len(rel))], 1).astype(np.float32)
        ns, _, _, step = oracle.discretize(EX_LIMITS, cells, initial, opts[0], opts[1], local,
                                           rotated_sp=True)
        na = (ns - 1) // 2
        theta = EX_THETA0 + sr * na * step
    name = f"extreme-L{L}-x{sx:+d}-y{sy:+d}-r{sr:+d}"
    case = Case(name, "prob", EX_LIMITS, cells, opts, initial, local)
    return case, (na + sr * na, xo, yo), na, step


def extreme_cases(oracle):
    return [extreme_case(oracle, L, *c) for L in EX_LS for c in EX_CORNERS]


# ---- section 4: the converted-grid cache ------------------------------------

CACHE_WINDOW = (0.1, 0.2)  # +-2 cells
CACHE_WIDE = (0.3, 0.2)  # +-6 cells: another padding P, and another winner


def cache_steps(oracle):
    """The Match sequence on one Context: [(label, case, on_device)], built so
    that consecutive steps differ in one term of EnsureGrid's reuse test."""
    cloud = straddling_cloud(40, 1040)
    zero = (0.0, 0.0)

    def prob(label, cells, window=CACHE_WINDOW, limits=LIMITS):
        return Case("cache-" + label, "prob", limits, cells, window + zero, INITIAL, cloud)

    def tsdf(label, tsd, wgt, truncation=TRUNCATION, max_weight=MAX_WEIGHT):
        return Case("cache-" + label, "tsdf", LIMITS, tsd, CACHE_WINDOW + zero, INITIAL, cloud, wgt,
                    truncation, max_weight)

    g1 = prob("G1", prob_cells(5))
    # One cell that G1's winner reads, moved to the other end of the scale.
    x, y = winner_cells(oracle, g1)[0]
    cells2 = g1.cells.copy()
    cells2[y, x] = 1 if (cells2[y, x] == 0 or cells2[y, x] > 16000) else 32767
    tsd, wgt = tsdf_planes(7)
    t1 = tsdf("T1", tsd, wgt)
    seen = [c for c in winner_cells(oracle, t1) if wgt[c[1], c[0]] != 0]
    x, y = seen[0]
    wgt2 = wgt.copy()
    wgt2[y, x] = 0
    return [
        ("G1", g1, False),
        ("G2: one cell changed", prob("G2", cells2), False),
        ("G2, wider window", prob("G2-wide", cells2, CACHE_WIDE), False),
        ("G2, first window", prob("G2", cells2), False),
        ("T1", t1, False),
        ("T1, one weight changed", tsdf("T1-w", tsd, wgt2), False),
        ("T1 cells, truncation 0.25", tsdf("T1-w-t", tsd, wgt2, 0.25), False),
        ("T1 cells, max weight 7", tsdf("T1-w-t-m", tsd, wgt2, 0.25, 7.0), False),
        ("G1 again", g1, False),
        ("device grid, other cells", prob("G3", prob_cells(6)), True),
        ("G1 from host cells", g1, False),
        ("G1 transposed: nx and ny exchanged", prob("G1-T", np.ascontiguousarray(g1.cells.T)),
         False),
    ]


# ---- section 5: the cases run under the environment variants ----------------

def child_cases():
    """No oracle needed to build them: the child process has none."""
    return batch_cases() + tie_cases()
