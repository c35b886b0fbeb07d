"""LocalTrajectoryBuilder3D on device-resident data (reference
mapping/internal/3d/local_trajectory_builder_3d.{h,cc}): the Python mirror of
include/cartographer_amd/local_trajectory_builder_3d.h.

The per-point work of a sweep (each point by its own extrapolated pose, the
range test, both voxel filters, the move to the tracking frame and both
adaptive voxel filters) is one ``range_data3d_prepare`` call; the scan match
and the insertion go through RealTimeCorrelativeScanMatcher3D,
CeresScanMatcher3D and ActiveSubmaps3D. The rotational histogram is
``compute_histogram`` on the host. Poses are ``(t, q)``: translation (3,) and
rotation (w, x, y, z), in double. Times are seconds. The caller supplies the
pose extrapolator; PoseExtrapolator, ImuTracker and RangeDataCollator are not
part of this.

Left out, all of them the fork's additions to upstream's builder:
scanmatch_mode 3 and 4 (PCL ICP / NDT), use_edge_filter and VoxelFilterEdge,
the IMU-acceleration gate of AddAccumulatedRangeData (:714-719), the PCD dumps
and logs, and the metrics gauges."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import (AdaptiveVoxelFilterOptions, Context, RangeData3DOptions,
               RealTimeCorrelativeScanMatcher3D, compute_histogram, default_context,
               range_data3d_prepare, range_data_transform, voxel_filter_large_mask)
from .local_trajectory_builder_2d import (MotionFilter, MotionFilterOptions,
                                          PoseExtrapolatorInterface, Rigid3, _cast_f, _inverse,
                                          _mul, _quat_mul, _rigid3d, _tq)
from .submap_2d import RangeData
from .submap_3d import (ActiveSubmaps3D, CeresScanMatcher3D, CeresScanMatcherOptions3D,
                        IntensityCostFunctionOptions, RangeDataInserterOptions3D, Submap3D,
                        SubmapsOptions3D)

_F = np.float32


@dataclass
class RealTimeCorrelativeScanMatcherOptions3D:
    """proto::RealTimeCorrelativeScanMatcherOptions; defaults from
    configuration_files/trajectory_builder_3d.lua:37-42."""
    linear_search_window: float = 0.15
    angular_search_window: float = math.radians(1.0)
    translation_delta_cost_weight: float = 1e-1
    rotation_delta_cost_weight: float = 1e-1


def _motion_filter_3d() -> MotionFilterOptions:
    """trajectory_builder_3d.lua:62-66."""
    return MotionFilterOptions(0.5, 0.1, 0.004)


def _ceres_3d() -> CeresScanMatcherOptions3D:
    """trajectory_builder_3d.lua:44-60, with intensity_cost_function_options_0."""
    return CeresScanMatcherOptions3D(
        intensity_cost_function_options_0=IntensityCostFunctionOptions())


def _submaps_3d() -> SubmapsOptions3D:
    return SubmapsOptions3D(range_data_inserter_options=RangeDataInserterOptions3D())


@dataclass
class LocalTrajectoryBuilderOptions3D:
    """proto::LocalTrajectoryBuilderOptions3D, the fields this builder reads;
    defaults from configuration_files/trajectory_builder_3d.lua:18-112."""
    min_range: float = 1.0
    max_range: float = 60.0
    num_accumulated_range_data: int = 1
    voxel_filter_size: float = 0.15
    high_resolution_adaptive_voxel_filter_options: AdaptiveVoxelFilterOptions = field(
        default_factory=lambda: AdaptiveVoxelFilterOptions.make(2.0, 150, 15.0))
    low_resolution_adaptive_voxel_filter_options: AdaptiveVoxelFilterOptions = field(
        default_factory=lambda: AdaptiveVoxelFilterOptions.make(4.0, 200, 60.0))
    use_online_correlative_scan_matching: bool = False
    real_time_correlative_scan_matcher_options: RealTimeCorrelativeScanMatcherOptions3D = field(
        default_factory=RealTimeCorrelativeScanMatcherOptions3D)
    ceres_scan_matcher_options: CeresScanMatcherOptions3D = field(default_factory=_ceres_3d)
    motion_filter_options: MotionFilterOptions = field(default_factory=_motion_filter_3d)
    rotational_histogram_size: int = 120
    submaps_options: SubmapsOptions3D = field(default_factory=_submaps_3d)
    use_intensities: bool = False

    def range_data_options(self) -> RangeData3DOptions:
        h = self.high_resolution_adaptive_voxel_filter_options
        l = self.low_resolution_adaptive_voxel_filter_options
        return RangeData3DOptions.make(
            self.min_range, self.max_range, self.voxel_filter_size,
            AdaptiveVoxelFilterOptions(h.max_length, h.min_num_points, h.max_range),
            AdaptiveVoxelFilterOptions(l.max_length, l.min_num_points, l.max_range))


@dataclass
class RangeMeasurement3D:
    """sensor::TimedPointCloudOriginData::RangeMeasurement
    (sensor/timed_point_cloud_data.h:40-44) as the 3D builder reads it."""
    position: Tuple[float, float, float]
    time: float
    intensity: float
    origin_index: int


@dataclass
class ExtrapolationResult:
    """PoseExtrapolatorInterface::ExtrapolationResult
    (pose_extrapolator_interface.h:38-46), the fields the 3D builder reads."""
    previous_poses: np.ndarray  # (n - 1, 7) float32, (t, q) per time but the last
    current_pose: Rigid3        # double
    gravity_from_tracking: Tuple[float, float, float, float]


class PoseExtrapolatorInterface3D(PoseExtrapolatorInterface):
    """The 2D builder's interface plus ExtrapolatePosesWithGravity, whose default
    body is PoseExtrapolator's (pose_extrapolator.cc:266-279)."""

    def ExtrapolatePosesWithGravity(self, times: Sequence[float]) -> ExtrapolationResult:
        times = [float(t) for t in times]
        previous = np.zeros((len(times) - 1, 7), np.float32)
        for i, t in enumerate(times[:-1]):
            previous[i] = _tq(_cast_f(_rigid3d(self.ExtrapolatePose(t))))
        current = _rigid3d(self.ExtrapolatePose(times[-1]))
        gravity = tuple(float(v) for v in self.EstimateGravityOrientation(times[-1]))
        return ExtrapolationResult(previous, current, gravity)


def extrapolate_poses_with_gravity(extrapolator, times) -> ExtrapolationResult:
    """The extrapolator's own ExtrapolatePosesWithGravity, else the default body
    over its ExtrapolatePose and EstimateGravityOrientation."""
    own = getattr(extrapolator, "ExtrapolatePosesWithGravity", None)
    if own is not None:
        return own(times)
    return PoseExtrapolatorInterface3D.ExtrapolatePosesWithGravity(extrapolator, times)


def local_from_gravity_aligned(pose_rotation, gravity_alignment):
    """pose_estimate.rotation() * gravity_alignment.inverse()
    (local_trajectory_builder_3d.cc:908-909): Eigen's inverse is the conjugate
    over the squared norm, summed as its packet reduction does."""
    w, x, y, z = (float(v) for v in gravity_alignment)
    n2 = (x * x + z * z) + (y * y + w * w)
    inv = (w / n2, -x / n2, -y / n2, -z / n2)
    return _quat_mul(tuple(float(v) for v in pose_rotation), inv)


# ---- results (local_trajectory_builder_3d.h:51-63) ----------------------------------

@dataclass
class TrajectoryNodeData3D:
    """TrajectoryNode::Data (trajectory_node.h:45-63), the fields the 3D builder fills."""
    time: float
    gravity_alignment: Tuple[float, float, float, float]
    high_resolution_point_cloud: np.ndarray
    low_resolution_point_cloud: np.ndarray
    rotational_scan_matcher_histogram: np.ndarray
    local_pose: Rigid3
    high_resolution_intensities: Optional[np.ndarray] = None
    low_resolution_intensities: Optional[np.ndarray] = None


@dataclass
class InsertionResult3D:
    constant_data: TrajectoryNodeData3D
    insertion_submaps: List[Submap3D]


@dataclass
class MatchingResult3D:
    time: float
    local_pose: Rigid3
    range_data_in_local: RangeData
    insertion_result: Optional[InsertionResult3D]  # None if dropped by the motion filter


@dataclass
class PreparedRangeData3D:
    """What one range_data3d_prepare call leaves: the range data in the
    tracking frame and the two filtered clouds, with their intensities."""
    range_data: RangeData
    high: np.ndarray
    low: np.ndarray
    high_intensities: Optional[np.ndarray]
    low_intensities: Optional[np.ndarray]


class LocalTrajectoryBuilder3D:
    """local_trajectory_builder_3d.h:47-126, without the collator, the IMU and
    odometry inputs and the metrics."""

    def __init__(self, options: Optional[LocalTrajectoryBuilderOptions3D] = None,
                 extrapolator=None, context: Optional[Context] = None):
        self.options = options or LocalTrajectoryBuilderOptions3D()
        self.context = context or default_context()
        self.extrapolator = extrapolator
        o = self.options
        s = o.submaps_options
        self.active_submaps = ActiveSubmaps3D(
            SubmapsOptions3D(s.high_resolution, s.high_resolution_max_range, s.low_resolution,
                             s.num_range_data, s.range_data_inserter_options, o.use_intensities),
            self.context)
        self.motion_filter = MotionFilter(o.motion_filter_options)
        self.real_time_correlative_scan_matcher = RealTimeCorrelativeScanMatcher3D(
            o.real_time_correlative_scan_matcher_options, self.context)
        self.ceres_scan_matcher = CeresScanMatcher3D(o.ceres_scan_matcher_options)
        self._range_data_options = o.range_data_options()
        self._num_accumulated = 0
        self._accumulated: List[dict] = []
        self.last_prepared: Optional[PreparedRangeData3D] = None  # test-visible

    def AddRangeData(self, time: float, origins, ranges: Sequence[RangeMeasurement3D],
                     intensities=None) -> Optional[MatchingResult3D]:
        """local_trajectory_builder_3d.cc:544-700 on synchronized data: ``origins``
        (k, 3); ``ranges`` a sequence of RangeMeasurement3D, or a tuple
        (positions (n, 3), times (n,), intensities (n,), origin_index (n,)).
        ``intensities``: the unsynchronized message's, for the size check."""
        if isinstance(ranges, tuple):
            position = np.asarray(ranges[0], np.float32).reshape(-1, 3)
            point_time = np.asarray(ranges[1], np.float32).reshape(-1)
            intensity = np.asarray(ranges[2], np.float32).reshape(-1)
            origin_index = np.asarray(ranges[3], np.int32).reshape(-1)
        else:
            position = np.array([r.position for r in ranges], np.float32).reshape(-1, 3)
            point_time = np.array([r.time for r in ranges], np.float32)
            intensity = np.array([r.intensity for r in ranges], np.float32)
            origin_index = np.array([r.origin_index for r in ranges], np.int32)
        o = self.options
        if o.use_intensities and intensities is not None:  # :544-549
            assert len(intensities) == len(position), \
                "Passed point cloud has inconsistent number of intensities and ranges."
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        if len(position) == 0:  # :552-555
            return None
        if self.extrapolator is None:  # :557-562
            return None
        assert len(point_time) == len(position) == len(intensity) == len(origin_index)
        assert point_time[-1] <= 0.0  # :565
        ex = self.extrapolator
        if time + float(point_time[0]) < ex.GetLastPoseTime():  # :566-572
            return None
        if self._num_accumulated == 0:
            self._accumulated = []
        # The per-message VoxelFilter (:584-585), on the sensor-frame positions.
        keep, _ = voxel_filter_large_mask(position, float(_F(0.5) * _F(o.voxel_filter_size)),
                                          self.context)
        self._accumulated.append({
            "time": float(time), "origins": origins, "position": position[keep],
            "point_time": point_time[keep], "intensity": intensity[keep],
            "origin_index": origin_index[keep]})
        self._num_accumulated += 1
        if self._num_accumulated < o.num_accumulated_range_data:  # :593-595
            return None
        self._num_accumulated = 0

        hit_times: List[float] = []
        prev_time_point = ex.GetLastExtrapolatedTime()
        for data in self._accumulated:  # :598-620
            for dt in data["point_time"]:
                time_point = data["time"] + float(dt)
                if time_point < prev_time_point:
                    time_point = prev_time_point
                hit_times.append(time_point)
                prev_time_point = time_point
        hit_times.append(self._accumulated[-1]["time"])
        result = extrapolate_poses_with_gravity(ex, hit_times)
        poses = np.asarray(result.previous_poses, np.float32).reshape(-1, 7)
        assert len(poses) + 1 == len(hit_times)  # :627

        hits = np.concatenate([d["position"] for d in self._accumulated])
        index, base = [], 0
        for d in self._accumulated:
            index.append(d["origin_index"] + base)
            base += len(d["origins"])
        current_pose = _rigid3d(result.current_pose)
        tracking_from_local = _tq(_cast_f(_inverse(current_pose)))  # :698
        local_origin = np.array([_F(v) for v in current_pose[0]], np.float32)  # :681
        prepared = range_data3d_prepare(
            self._range_data_options, hits, np.concatenate(index), poses,
            np.concatenate([d["origins"] for d in self._accumulated]), tracking_from_local,
            local_origin,
            intensities=(np.concatenate([d["intensity"] for d in self._accumulated])
                         if o.use_intensities else None),
            context=self.context)
        self._accumulated = []
        current_time = hit_times[-1]  # :678
        self.last_prepared = PreparedRangeData3D(
            RangeData(prepared["origin"], prepared["returns"], prepared["misses"],
                      prepared["returns_intensities"]),
            prepared["high"], prepared["low"], prepared["high_intensities"],
            prepared["low_intensities"])
        return self.AddAccumulatedRangeData(current_time, self.last_prepared, current_pose,
                                            result.gravity_from_tracking)

    def AddAccumulatedRangeData(self, time: float, prepared: PreparedRangeData3D,
                                pose_prediction: Rigid3,
                                gravity_alignment) -> Optional[MatchingResult3D]:
        """:705-874 without the fork's additions and the wall-clock metrics; the
        adaptive voxel filters of :734-745 have already run on the device."""
        filtered_range_data_in_tracking = prepared.range_data
        if len(filtered_range_data_in_tracking.returns) == 0:  # :722-725
            return None
        if len(prepared.high) == 0:  # :738-741
            return None
        if len(prepared.low) == 0:  # :746-749
            return None
        pose_estimate = self.ScanMatch(pose_prediction, prepared.low, prepared.high,
                                       prepared.high_intensities)
        if pose_estimate is None:  # :785-788
            return None
        self.extrapolator.AddPose(time, pose_estimate)  # :799
        g = filtered_range_data_in_tracking
        origin, returns, misses = range_data_transform(_tq(_cast_f(pose_estimate)), g.origin,
                                                       g.returns, g.misses, self.context)
        filtered_range_data_in_local = RangeData(origin, returns, misses, g.intensities)
        insertion_result = self.InsertIntoSubmap(
            time, filtered_range_data_in_local, filtered_range_data_in_tracking, prepared,
            pose_estimate, gravity_alignment)
        return MatchingResult3D(time, pose_estimate, filtered_range_data_in_local,
                                insertion_result)

    def ScanMatch(self, pose_prediction: Rigid3, low_resolution_point_cloud_in_tracking,
                  high_resolution_point_cloud_in_tracking, high_resolution_intensities=None):
        """:451-515 (the upstream path) -> the pose estimate in the local frame."""
        pose_prediction = _rigid3d(pose_prediction)
        submaps = self.active_submaps.submaps()
        if not submaps:  # :456-458
            return pose_prediction
        matching_submap = submaps[0]
        local_pose = _rigid3d(matching_submap.local_pose())
        initial_ceres_pose = _mul(_inverse(local_pose), pose_prediction, math.sqrt)
        target_translation = initial_ceres_pose[0]  # :494, the same product
        if self.options.use_online_correlative_scan_matching:  # :478-485
            _, initial_ceres_pose = self.real_time_correlative_scan_matcher.Match(
                initial_ceres_pose, high_resolution_point_cloud_in_tracking,
                matching_submap.high_resolution_hybrid_grid())
        intensity_grid = (matching_submap.high_resolution_intensity_hybrid_grid()
                          if self.options.use_intensities else None)
        self.last_scan_match_inputs = (target_translation, initial_ceres_pose)  # test-visible
        pose_observation_in_submap, _ = self.ceres_scan_matcher.Match(
            target_translation, initial_ceres_pose,
            [(high_resolution_point_cloud_in_tracking,
              matching_submap.high_resolution_hybrid_grid(), intensity_grid),
             (low_resolution_point_cloud_in_tracking,
              matching_submap.low_resolution_hybrid_grid(), None)],
            intensities=high_resolution_intensities if intensity_grid is not None else None)
        return _mul(local_pose, _rigid3d(pose_observation_in_submap), math.sqrt)  # :513-514

    def InsertIntoSubmap(self, time: float, filtered_range_data_in_local: RangeData,
                         filtered_range_data_in_tracking: RangeData,
                         prepared: PreparedRangeData3D, pose_estimate: Rigid3,
                         gravity_alignment) -> Optional[InsertionResult3D]:
        """:886-925. The returns are rotated into the gravity frame by
        csm_range_data_transform with a zero translation (the device kernel, as
        TransformPointCloud by Rigid3f::Rotation is the same arithmetic)."""
        if self.motion_filter.IsSimilar(time, pose_estimate):
            return None
        gravity_alignment = tuple(float(v) for v in gravity_alignment)
        rotation = ((_F(0.0), _F(0.0), _F(0.0)), tuple(_F(v) for v in gravity_alignment))
        _, in_gravity, _ = range_data_transform(_tq(rotation), np.zeros(3, np.float32),
                                                filtered_range_data_in_tracking.returns, None,
                                                self.context)
        histogram = compute_histogram(in_gravity, self.options.rotational_histogram_size)
        lfga = local_from_gravity_aligned(_rigid3d(pose_estimate)[1], gravity_alignment)
        self.last_insertion_inputs = (histogram, lfga)  # test-visible
        insertion_submaps = self.active_submaps.InsertData(filtered_range_data_in_local, lfga,
                                                           histogram)
        return InsertionResult3D(
            TrajectoryNodeData3D(time, gravity_alignment, prepared.high, prepared.low, histogram,
                                 pose_estimate, prepared.high_intensities,
                                 prepared.low_intensities),
            insertion_submaps)
