"""Submap2D, ActiveSubmaps2D and the two 2D range-data inserters on
device-resident grids (reference mapping/2d/submap_2d.{h,cc},
probability_grid_range_data_inserter_2d.{h,cc},
mapping/internal/2d/tsdf_range_data_inserter_2d.{h,cc}): the Python mirror of
include/cartographer_amd/submap_2d.h."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Union

import numpy as np

from . import (Context, DeviceProbabilityGrid, DeviceTSDF2D, FastCorrelativeScanMatcher2D,
               FastCorrelativeScanMatcherOptions2D, TSDFInserterOptions, default_context)

# proto::GridOptions2D::GridType (grid_2d_options.proto:20-24).
PROBABILITY_GRID = "PROBABILITY_GRID"
TSDF = "TSDF"


def FastMatcherFor(grid: Union[DeviceProbabilityGrid, DeviceTSDF2D],
                   options: FastCorrelativeScanMatcherOptions2D) -> FastCorrelativeScanMatcher2D:
    """FastCorrelativeScanMatcher2D(grid, options) for a device-resident grid,
    on the grid's context and without a host copy (submap_2d.h's
    FastMatcherFor): a DeviceTSDF2D gives a TSDF matcher, which
    ceres_refine_batch refines with the TSDF match cost."""
    return FastCorrelativeScanMatcher2D(grid, options, grid.context)


@dataclass
class RangeData:
    """sensor::RangeData (sensor/range_data.h:31-35), in the grid's frame."""
    origin: np.ndarray                       # (3,)
    returns: np.ndarray                      # (n, 3)
    misses: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float32))
    # returns.intensities() (sensor/point_cloud.h:46-58): None, or (n,). Read by
    # the 3D inserter only.
    intensities: Optional[np.ndarray] = None


@dataclass
class ProbabilityGridRangeDataInserterOptions2D:
    """proto::ProbabilityGridRangeDataInserterOptions2D; defaults from
    configuration_files/trajectory_builder_2d.lua:81-87."""
    hit_probability: float = 0.55
    miss_probability: float = 0.49
    insert_free_space: bool = True


class ProbabilityGridRangeDataInserter2D:
    """probability_grid_range_data_inserter_2d.h:37-56."""

    def __init__(self, options: Optional[ProbabilityGridRangeDataInserterOptions2D] = None):
        self.options = options or ProbabilityGridRangeDataInserterOptions2D()

    def Insert(self, range_data: RangeData, grid: DeviceProbabilityGrid) -> None:
        o = self.options
        grid.insert(range_data.origin, range_data.returns, range_data.misses, o.hit_probability,
                    o.miss_probability, o.insert_free_space)

    def InsertBatch(self, range_data: RangeData, grids: List[DeviceProbabilityGrid]) -> None:
        """The same scan into several grids in one call (ActiveSubmaps2D)."""
        o = self.options
        scan = (range_data.origin, range_data.returns, range_data.misses)
        DeviceProbabilityGrid.insert_batch(grids, list(range(len(grids))), [scan] * len(grids),
                                           o.hit_probability, o.miss_probability,
                                           o.insert_free_space)


@dataclass
class TSDFRangeDataInserterOptions2D:
    """proto::TSDFRangeDataInserterOptions2D; defaults from
    configuration_files/trajectory_builder_2d.lua:100-112."""
    truncation_distance: float = 0.3
    maximum_weight: float = 10.0
    update_free_space: bool = False
    num_normal_samples: int = 4
    sample_radius: float = 0.5
    project_sdf_distance_to_scan_normal: bool = True
    update_weight_range_exponent: int = 0
    update_weight_angle_scan_normal_to_ray_kernel_bandwidth: float = 0.5
    update_weight_distance_cell_to_hit_kernel_bandwidth: float = 0.5

    def as_struct(self) -> TSDFInserterOptions:
        return TSDFInserterOptions.make((
            self.truncation_distance, self.maximum_weight, int(self.update_free_space),
            self.num_normal_samples, self.sample_radius,
            int(self.project_sdf_distance_to_scan_normal), self.update_weight_range_exponent,
            self.update_weight_angle_scan_normal_to_ray_kernel_bandwidth,
            self.update_weight_distance_cell_to_hit_kernel_bandwidth))


class TSDFRangeDataInserter2D:
    """tsdf_range_data_inserter_2d.h:33-55 (the reference ignores misses)."""

    def __init__(self, options: Optional[TSDFRangeDataInserterOptions2D] = None):
        self.options = options or TSDFRangeDataInserterOptions2D()

    def Insert(self, range_data: RangeData, grid: DeviceTSDF2D) -> None:
        grid.insert(range_data.origin, range_data.returns, self.options.as_struct())

    def InsertBatch(self, range_data: RangeData, grids: List[DeviceTSDF2D]) -> None:
        """The same scan into several grids in one call (ActiveSubmaps2D)."""
        scan = (range_data.origin, range_data.returns)
        DeviceTSDF2D.insert_batch(grids, list(range(len(grids))), [scan] * len(grids),
                                  self.options.as_struct())


class Submap2D:
    """submap_2d.h:41-72 (the grid and the insertion counters; the local pose
    is the origin the submap was created at). The grid is a ProbabilityGrid
    (``grid()``) or a TSDF2D (``tsdf()``); the other accessor returns None."""

    def __init__(self, origin, grid: Union[DeviceProbabilityGrid, DeviceTSDF2D]):
        self.origin = np.asarray(origin, np.float32)[:2].copy()
        self._grid = grid
        self._num_range_data = 0
        self._insertion_finished = False

    def grid(self) -> Optional[DeviceProbabilityGrid]:
        return self._grid if isinstance(self._grid, DeviceProbabilityGrid) else None

    def tsdf(self) -> Optional[DeviceTSDF2D]:
        return self._grid if isinstance(self._grid, DeviceTSDF2D) else None

    def num_range_data(self) -> int:
        return self._num_range_data

    def insertion_finished(self) -> bool:
        return self._insertion_finished

    def InsertRangeData(self, range_data: RangeData,
                        inserter: Union[ProbabilityGridRangeDataInserter2D,
                                        TSDFRangeDataInserter2D]) -> None:
        assert not self._insertion_finished  # submap_2d.cc:141
        inserter.Insert(range_data, self._grid)
        self._num_range_data += 1

    def Finish(self) -> None:
        assert not self._insertion_finished  # submap_2d.cc:148
        self._grid.finish()
        self._insertion_finished = True


class ActiveSubmaps2D:
    """submap_2d.h:86-115, .cc:153-232: at most two submaps; a new 100 x 100 one
    centred on the scan origin when the newest holds num_range_data scans; every
    scan goes into all of them (one insert_batch call); the oldest is finished
    at 2 * num_range_data. ``grid_type`` selects the grid and its inserter
    (CreateGrid and CreateRangeDataInserter, .cc:176-222): PROBABILITY_GRID (the
    default) or TSDF, whose truncation distance and maximum weight come from
    ``tsdf_inserter_options``."""

    kInitialSubmapSize = 100

    def __init__(self, num_range_data: int, resolution: float = 0.05,
                 inserter_options: Optional[ProbabilityGridRangeDataInserterOptions2D] = None,
                 context: Optional[Context] = None, grid_type: str = PROBABILITY_GRID,
                 tsdf_inserter_options: Optional[TSDFRangeDataInserterOptions2D] = None):
        if grid_type not in (PROBABILITY_GRID, TSDF):
            raise ValueError("Unknown GridType.")  # :220
        self.num_range_data = int(num_range_data)
        self.resolution = float(np.float32(resolution))  # `float resolution` (:195)
        self.grid_type = grid_type
        if grid_type == TSDF:
            self.range_data_inserter = TSDFRangeDataInserter2D(tsdf_inserter_options)
        else:
            self.range_data_inserter = ProbabilityGridRangeDataInserter2D(inserter_options)
        self.context = context or default_context()
        self._submaps: List[Submap2D] = []

    def submaps(self) -> List[Submap2D]:
        return list(self._submaps)

    def _add_submap(self, origin) -> None:
        if len(self._submaps) >= 2:
            assert self._submaps[0].insertion_finished()  # :224
            self._submaps.pop(0)
        o = np.asarray(origin, np.float32)
        half = 0.5 * self.kInitialSubmapSize * self.resolution
        if self.grid_type == TSDF:
            t = self.range_data_inserter.options
            grid = DeviceTSDF2D(self.resolution, float(o[0]) + half, float(o[1]) + half,
                                self.kInitialSubmapSize, self.kInitialSubmapSize,
                                t.truncation_distance, t.maximum_weight, context=self.context)
        else:
            grid = DeviceProbabilityGrid(self.resolution, float(o[0]) + half, float(o[1]) + half,
                                         self.kInitialSubmapSize, self.kInitialSubmapSize,
                                         context=self.context)
        self._submaps.append(Submap2D(o, grid))

    def InsertRangeData(self, range_data: RangeData) -> List[Submap2D]:
        if not self._submaps or self._submaps[-1].num_range_data() == self.num_range_data:
            self._add_submap(range_data.origin)
        self.range_data_inserter.InsertBatch(range_data, [s._grid for s in self._submaps])
        for s in self._submaps:
            s._num_range_data += 1
        if self._submaps[0].num_range_data() == 2 * self.num_range_data:
            self._submaps[0].Finish()
        return self.submaps()
