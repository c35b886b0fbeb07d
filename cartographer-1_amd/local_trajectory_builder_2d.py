"""LocalTrajectoryBuilder2D on device-resident data (reference
mapping/internal/2d/local_trajectory_builder_2d.{h,cc},
mapping/internal/motion_filter.{h,cc}): the Python mirror of
include/cartographer_amd/local_trajectory_builder_2d.h.

The per-point work of a sweep (each point by its own extrapolated pose, the
range test, the gravity alignment, the crop and the voxel filters) is one
``range_data2d_prepare`` call; the scan match and the insertion go through
RealTimeCorrelativeScanMatcher2D, CeresScanMatcher2D and ActiveSubmaps2D on
either grid type. Poses are ``(t, q)``: translation (3,) and rotation
(w, x, y, z), in double; 2D poses are ``(x, y, angle)``. Times are seconds
(pose_graph_2d_search.h's time type). The caller supplies the pose
extrapolator; PoseExtrapolator, ImuTracker and RangeDataCollator are not
part of this."""
from __future__ import annotations

import abc
import ctypes as C
import ctypes.util
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import (AdaptiveVoxelFilterOptions, CeresOptions2D, CeresScanMatcher2D, Context,
               RangeData2DOptions, RealTimeCorrelativeScanMatcher2D,
               RealTimeCorrelativeScanMatcherOptions, default_context, range_data2d_prepare,
               range_data_transform)
from .submap_2d import (PROBABILITY_GRID, ActiveSubmaps2D,
                        ProbabilityGridRangeDataInserterOptions2D, RangeData, Submap2D,
                        TSDFRangeDataInserterOptions2D)

Rigid3 = Tuple[Sequence[float], Sequence[float]]

# The C library's sinf and cosf: what std::sin(float) is in the C++ header and
# in the reference, so Embed3D in float gives the same bits here.
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.sinf, _libm.cosf):
    _f.restype = C.c_float
    _f.argtypes = [C.c_float]
_F = np.float32


# ---- transform/rigid_transform.h and transform.h in Eigen's operation order ----

def _cross(a, b):
    """Eigen MatrixBase::cross, coefficient order kept."""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _rotate(q, v):
    """QuaternionBase::_transformVector; q = (w, x, y, z). Works in the type of
    its arguments (float or np.float32)."""
    uv = _cross(q[1:], v)
    uv = tuple(c + c for c in uv)
    c = _cross(q[1:], uv)
    return tuple((v[a] + q[0] * uv[a]) + c[a] for a in range(3))


def _quat_mul(a, b):
    """Eigen's quaternion product (generic path)."""
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def _quat_normalized(q, sqrt):
    """QuaternionBase::normalized: coeffs / coeffs.norm(), the squared norm
    summed as the packet reduction does over (x, y, z, w) storage."""
    w, x, y, z = q
    n = sqrt((x * x + z * z) + (y * y + w * w))
    if n > 0:
        return (w / n, x / n, y / n, z / n)
    return q


def _apply(r, p):
    """Rigid3::operator*(vector) (rigid_transform.h:190-196)."""
    v = _rotate(r[1], p)
    return tuple(v[a] + r[0][a] for a in range(3))


def _mul(a, b, sqrt):
    """Rigid3 * Rigid3 (rigid_transform.h:181-188): the product's rotation is normalized."""
    return (_apply(a, b[0]), _quat_normalized(_quat_mul(a[1], b[1]), sqrt))


def _inverse(r):
    """Rigid3::inverse (rigid_transform.h:150-154)."""
    c = (r[1][0], -r[1][1], -r[1][2], -r[1][3])
    t = _rotate(c, r[0])
    return (tuple(-x for x in t), c)


def _norm3(v, sqrt):
    """Eigen's redux of a 3-vector: x0 + (x1 + x2)."""
    return sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]))


def _rigid3d(pose: Rigid3):
    return (tuple(float(x) for x in pose[0]), tuple(float(x) for x in pose[1]))


def _cast_f(pose):
    """Rigid3d::cast<float>()."""
    return (tuple(_F(x) for x in pose[0]), tuple(_F(x) for x in pose[1]))


def _tq(pose) -> np.ndarray:
    return np.array(list(pose[0]) + list(pose[1]), np.float32)


def GetAngle(pose: Rigid3) -> float:
    """transform::GetAngle (transform.h:34-37)."""
    q = pose[1]
    return 2.0 * math.atan2(_norm3(q[1:], math.sqrt), abs(q[0]))


def Project2D(pose: Rigid3) -> Tuple[float, float, float]:
    """transform::Project2D (transform.h:103-106) with GetYaw (:43-47)."""
    d = _rotate(pose[1], (1.0, 0.0, 0.0))
    return (pose[0][0], pose[0][1], math.atan2(d[1], d[0]))


def Embed3D(pose2d) -> Rigid3:
    """transform::Embed3D (transform.h:110-115) in double: AngleAxis about z."""
    ha = 0.5 * float(pose2d[2])
    s = math.sin(ha)
    return ((float(pose2d[0]), float(pose2d[1]), 0.0), (math.cos(ha), s * 0.0, s * 0.0, s * 1.0))


def Embed3DF(pose2d):
    """Embed3D(pose.cast<float>()) (local_trajectory_builder_2d.cc:248), in float."""
    ha = _F(0.5) * _F(pose2d[2])
    s = _F(_libm.sinf(float(ha)))
    zero = s * _F(0.0)
    return ((_F(pose2d[0]), _F(pose2d[1]), _F(0.0)),
            (_F(_libm.cosf(float(ha))), zero, zero, s * _F(1.0)))


# ---- MotionFilter ----------------------------------------------------------------

@dataclass
class MotionFilterOptions:
    """proto::MotionFilterOptions; defaults from
    configuration_files/trajectory_builder_2d.lua:56-60."""
    max_time_seconds: float = 5.0
    max_distance_meters: float = 0.2
    max_angle_radians: float = math.radians(1.0)


class MotionFilter:
    """motion_filter.h:34-49, .cc:40-58, in double, without the log line."""

    def __init__(self, options: Optional[MotionFilterOptions] = None):
        self.options = options or MotionFilterOptions()
        self.num_total = 0
        self.num_different = 0
        self.last_time = 0.0
        self.last_pose: Rigid3 = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0))

    def IsSimilar(self, time: float, pose: Rigid3) -> bool:
        """True when the pose is close, in time, distance and angle, to the
        last one that was not."""
        o = self.options
        pose = _rigid3d(pose)
        self.num_total += 1
        if (self.num_total > 1 and time - self.last_time <= o.max_time_seconds and
                _norm3(tuple(pose[0][a] - self.last_pose[0][a] for a in range(3)), math.sqrt)
                <= o.max_distance_meters and
                GetAngle(_mul(_inverse(pose), self.last_pose, math.sqrt)) <= o.max_angle_radians):
            return True
        self.last_time = time
        self.last_pose = pose
        self.num_different += 1
        return False


# ---- options and the extrapolator ------------------------------------------------

@dataclass
class SubmapsOptions2D:
    """proto::SubmapsOptions2D, the fields ActiveSubmaps2D reads; defaults from
    configuration_files/trajectory_builder_2d.lua:87-114."""
    num_range_data: int = 90
    resolution: float = 0.05
    grid_type: str = PROBABILITY_GRID
    range_data_inserter_options: ProbabilityGridRangeDataInserterOptions2D = field(
        default_factory=ProbabilityGridRangeDataInserterOptions2D)
    tsdf_range_data_inserter_options: TSDFRangeDataInserterOptions2D = field(
        default_factory=TSDFRangeDataInserterOptions2D)


@dataclass
class CeresScanMatcherOptions2D:
    """proto::CeresScanMatcherOptions2D; defaults from
    configuration_files/trajectory_builder_2d.lua:45-54."""
    occupied_space_weight: float = 1.0
    translation_weight: float = 10.0
    rotation_weight: float = 40.0
    max_num_iterations: int = 20
    use_nonmonotonic_steps: bool = False


@dataclass
class LocalTrajectoryBuilderOptions2D:
    """proto::LocalTrajectoryBuilderOptions2D, the fields this builder reads;
    defaults from configuration_files/trajectory_builder_2d.lua:17-60."""
    min_range: float = 0.0
    max_range: float = 30.0
    min_z: float = -0.8
    max_z: float = 2.0
    missing_data_ray_length: float = 5.0
    num_accumulated_range_data: int = 1
    voxel_filter_size: float = 0.025
    adaptive_voxel_filter_options: AdaptiveVoxelFilterOptions = field(
        default_factory=AdaptiveVoxelFilterOptions.make)
    use_online_correlative_scan_matching: bool = False
    real_time_correlative_scan_matcher_options: RealTimeCorrelativeScanMatcherOptions = field(
        default_factory=RealTimeCorrelativeScanMatcherOptions)
    ceres_scan_matcher_options: CeresScanMatcherOptions2D = field(
        default_factory=CeresScanMatcherOptions2D)
    motion_filter_options: MotionFilterOptions = field(default_factory=MotionFilterOptions)
    submaps_options: SubmapsOptions2D = field(default_factory=SubmapsOptions2D)

    def range_data_options(self) -> RangeData2DOptions:
        a = self.adaptive_voxel_filter_options
        return RangeData2DOptions.make(
            self.min_range, self.max_range, self.missing_data_ray_length, self.min_z, self.max_z,
            self.voxel_filter_size,
            AdaptiveVoxelFilterOptions(a.max_length, a.min_num_points, a.max_range))


class PoseExtrapolatorInterface(abc.ABC):
    """mapping/pose_extrapolator_interface.h:36-78, the methods the 2D builder
    calls. Poses are (t, q) in double; times are seconds."""

    @abc.abstractmethod
    def GetLastPoseTime(self) -> float: ...

    @abc.abstractmethod
    def GetLastExtrapolatedTime(self) -> float: ...

    @abc.abstractmethod
    def ExtrapolatePose(self, time: float) -> Rigid3: ...

    @abc.abstractmethod
    def EstimateGravityOrientation(self, time: float) -> Sequence[float]:
        """The rotation (w, x, y, z) to the gravity-aligned frame."""

    @abc.abstractmethod
    def AddPose(self, time: float, pose: Rigid3) -> None: ...


# ---- results (local_trajectory_builder_2d.h:49-62) ---------------------------------

@dataclass
class TrajectoryNodeData:
    """TrajectoryNode::Data (trajectory_node.h:45-63), the fields the 2D builder fills."""
    time: float
    gravity_alignment: Tuple[float, float, float, float]
    filtered_gravity_aligned_point_cloud: np.ndarray
    local_pose: Rigid3


@dataclass
class InsertionResult:
    constant_data: TrajectoryNodeData
    insertion_submaps: List[Submap2D]


@dataclass
class MatchingResult:
    time: float
    local_pose: Rigid3
    range_data_in_local: RangeData
    insertion_result: Optional[InsertionResult]  # None if dropped by the motion filter


class LocalTrajectoryBuilder2D:
    """local_trajectory_builder_2d.h:45-124, without the collator, the IMU and
    odometry inputs and the metrics."""

    def __init__(self, options: Optional[LocalTrajectoryBuilderOptions2D] = None,
                 extrapolator: Optional[PoseExtrapolatorInterface] = None,
                 context: Optional[Context] = None):
        self.options = options or LocalTrajectoryBuilderOptions2D()
        self.context = context or default_context()
        self.extrapolator = extrapolator
        s = self.options.submaps_options
        self.active_submaps = ActiveSubmaps2D(
            s.num_range_data, s.resolution, s.range_data_inserter_options, self.context,
            s.grid_type, s.tsdf_range_data_inserter_options)
        self.motion_filter = MotionFilter(self.options.motion_filter_options)
        self.real_time_correlative_scan_matcher = RealTimeCorrelativeScanMatcher2D(
            self.options.real_time_correlative_scan_matcher_options, self.context)
        c = self.options.ceres_scan_matcher_options
        self.ceres_scan_matcher = CeresScanMatcher2D(
            CeresOptions2D.make(c.occupied_space_weight, c.translation_weight, c.rotation_weight,
                                c.max_num_iterations, c.use_nonmonotonic_steps), self.context)
        self._range_data_options = self.options.range_data_options()
        self._num_accumulated = 0
        self._reset_accumulation()

    def _reset_accumulation(self):
        self._hits: List[np.ndarray] = []
        self._index: List[np.ndarray] = []
        self._poses: List[np.ndarray] = []
        self._origins: List[np.ndarray] = []
        self._num_origins = 0

    def AddRangeData(self, time: float, origins, ranges) -> Optional[MatchingResult]:
        """local_trajectory_builder_2d.cc:104-209 on synchronized data: ``origins``
        (k, 3); ``ranges`` = (point_time (n, 4) as x, y, z, relative time;
        origin_index (n,)). The raw points and their poses are kept until
        num_accumulated_range_data calls have come; then one device call."""
        point_time = np.asarray(ranges[0], np.float32).reshape(-1, 4)
        origin_index = np.asarray(ranges[1], np.int32).reshape(-1)
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        if len(point_time) == 0 or self.extrapolator is None:  # :110-113, :121-126
            return None
        assert len(origin_index) == len(point_time)
        assert point_time[-1, 3] <= 0.0  # :130
        ex = self.extrapolator
        if time + float(point_time[0, 3]) < ex.GetLastPoseTime():  # :131-137
            return None
        poses = np.zeros((len(point_time), 7), np.float32)
        for i in range(len(point_time)):
            time_point = time + float(point_time[i, 3])
            if time_point < ex.GetLastExtrapolatedTime():  # :144-152
                time_point = ex.GetLastExtrapolatedTime()
            poses[i] = _tq(_cast_f(_rigid3d(ex.ExtrapolatePose(time_point))))
        if self._num_accumulated == 0:
            self._reset_accumulation()
        self._hits.append(point_time[:, :3])
        self._index.append(origin_index + self._num_origins)
        self._poses.append(poses)
        self._origins.append(origins)
        self._num_origins += len(origins)
        self._num_accumulated += 1
        if self._num_accumulated < self.options.num_accumulated_range_data:
            return None
        self._num_accumulated = 0
        gravity_q = tuple(float(x) for x in ex.EstimateGravityOrientation(time))
        gravity_alignment = ((0.0, 0.0, 0.0), gravity_q)
        last = (tuple(poses[-1, :3]), tuple(poses[-1, 3:]))  # range_data_poses.back()
        gravity_from_local = _mul(_cast_f(gravity_alignment), _inverse(last), np.sqrt)
        origin, returns, misses, filtered = range_data2d_prepare(
            self._range_data_options, np.concatenate(self._hits), np.concatenate(self._index),
            np.concatenate(self._poses), np.concatenate(self._origins), _tq(gravity_from_local),
            poses[-1, :3], self.context)
        self._reset_accumulation()
        return self.AddAccumulatedRangeData(time, RangeData(origin, returns, misses),
                                            gravity_alignment, filtered)

    def AddAccumulatedRangeData(self, time: float, gravity_aligned_range_data: RangeData,
                                gravity_alignment: Rigid3,
                                filtered_gravity_aligned_point_cloud) -> Optional[MatchingResult]:
        """:211-277 without the wall-clock metrics; the adaptive voxel filter of
        :228-231 has already run on the device."""
        if len(gravity_aligned_range_data.returns) == 0:
            return None
        gravity_alignment = _rigid3d(gravity_alignment)
        non_gravity_aligned_pose_prediction = _rigid3d(self.extrapolator.ExtrapolatePose(time))
        pose_prediction = Project2D(_mul(non_gravity_aligned_pose_prediction,
                                         _inverse(gravity_alignment), math.sqrt))
        if len(filtered_gravity_aligned_point_cloud) == 0:
            return None
        pose_estimate_2d = self.ScanMatch(time, pose_prediction,
                                          filtered_gravity_aligned_point_cloud)
        if pose_estimate_2d is None:
            return None
        pose_estimate = _mul(Embed3D(pose_estimate_2d), gravity_alignment, math.sqrt)
        self.extrapolator.AddPose(time, pose_estimate)
        g = gravity_aligned_range_data
        origin, returns, misses = range_data_transform(_tq(Embed3DF(pose_estimate_2d)), g.origin,
                                                       g.returns, g.misses, self.context)
        range_data_in_local = RangeData(origin, returns, misses)
        insertion_result = self.InsertIntoSubmap(
            time, range_data_in_local, filtered_gravity_aligned_point_cloud, pose_estimate,
            gravity_alignment[1])
        return MatchingResult(time, pose_estimate, range_data_in_local, insertion_result)

    def ScanMatch(self, time: float, pose_prediction, filtered_gravity_aligned_point_cloud):
        """:65-102 -> the pose observation (x, y, angle)."""
        submaps = self.active_submaps.submaps()
        if not submaps:
            return tuple(pose_prediction)
        matching_submap = submaps[0]
        grid = matching_submap.grid() or matching_submap.tsdf()
        initial_ceres_pose = tuple(pose_prediction)
        if self.options.use_online_correlative_scan_matching:
            _, initial_ceres_pose = self.real_time_correlative_scan_matcher.Match(
                pose_prediction, filtered_gravity_aligned_point_cloud, grid)
        pose_observation, _ = self.ceres_scan_matcher.Match(
            pose_prediction[:2], initial_ceres_pose, filtered_gravity_aligned_point_cloud, grid)
        return pose_observation

    def InsertIntoSubmap(self, time: float, range_data_in_local: RangeData,
                         filtered_gravity_aligned_point_cloud, pose_estimate: Rigid3,
                         gravity_alignment) -> Optional[InsertionResult]:
        """:279-300."""
        if self.motion_filter.IsSimilar(time, pose_estimate):
            return None
        insertion_submaps = self.active_submaps.InsertRangeData(range_data_in_local)
        return InsertionResult(
            TrajectoryNodeData(time, tuple(gravity_alignment),
                               filtered_gravity_aligned_point_cloud, pose_estimate),
            insertion_submaps)
