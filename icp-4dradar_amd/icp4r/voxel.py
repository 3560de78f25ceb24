"""Voxel-grid downsampling on the device (include/icp4r/icp4r_voxel.h): pcl::VoxelGrid as the
reference's radar_odometry node uses it for its surround map (radar_odometry.cpp:426-429):

    pcl::VoxelGrid<pcl::PointXYZI> sor;
    sor.setInputCloud(RadarCloudMap);
    sor.setLeafSize(0.5f, 0.5f, 0.5f);
    sor.filter(*downSizeFilterMap);

Same method names; clouds are (N, >=3) float32 arrays (x, y, z[, intensity]), the result is (K, 4)
float32 in ascending leaf index.  GPU-only: there is no CPU fallback.  A map that is already resident
filters itself: KD_TREE.voxel_filter / voxel_filter_device (icp4r.mapstore).  VoxelAccumulator is the
incremental form (include/icp4r/icp4r_voxel_acc.h): add each scan once, then filter.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import Context, _check, _cloud, _ptr, default_context, load


class VoxelParams(C.Structure):
    """icp4r_voxel_params."""
    _fields_ = [("leaf", C.c_float * 3), ("downsample_all_data", C.c_int32), ("min_points_per_voxel", C.c_uint32)]


def voxel_params(leaf=None, downsample_all_data: bool = True, min_points_per_voxel: int = 0) -> VoxelParams:
    """PCL's defaults (icp4r_voxel_params_default) with the given fields; leaf: one float or three."""
    p = VoxelParams()
    _check(load().icp4r_voxel_params_default(C.byref(p)), "icp4r_voxel_params_default")
    if leaf is not None:
        lf = np.broadcast_to(np.asarray(leaf, np.float32).reshape(-1), (3,))
        p.leaf[0], p.leaf[1], p.leaf[2] = float(lf[0]), float(lf[1]), float(lf[2])
    p.downsample_all_data = 1 if downsample_all_data else 0
    p.min_points_per_voxel = int(min_points_per_voxel)
    return p


class VoxelGrid:
    """pcl::VoxelGrid<PointT> (PCL 1.8.1 applyFilter; the contract in include/icp4r/icp4r_voxel.h)."""

    def __init__(self, ctx: Context | None = None):
        self._ctx = ctx or default_context()
        self._lib = load()
        self._p = voxel_params()
        self._cloud = None

    # -- PCL's method names ----------------------------------------------------------------------
    def setInputCloud(self, cloud):  # noqa: N802
        self._cloud = cloud

    def setLeafSize(self, lx: float, ly: float | None = None, lz: float | None = None):  # noqa: N802
        ly = lx if ly is None else ly
        lz = lx if lz is None else lz
        self._p.leaf[0], self._p.leaf[1], self._p.leaf[2] = float(np.float32(lx)), float(np.float32(ly)), float(np.float32(lz))

    def getLeafSize(self):  # noqa: N802
        return tuple(self._p.leaf)

    def setDownsampleAllData(self, downsample: bool):  # noqa: N802
        self._p.downsample_all_data = 1 if downsample else 0

    def getDownsampleAllData(self) -> bool:  # noqa: N802
        return bool(self._p.downsample_all_data)

    def setMinimumPointsNumberPerVoxel(self, min_points: int):  # noqa: N802
        self._p.min_points_per_voxel = int(min_points)

    def getMinimumPointsNumberPerVoxel(self) -> int:  # noqa: N802
        return int(self._p.min_points_per_voxel)

    @property
    def params(self) -> VoxelParams:
        return self._p

    def filter(self, cloud=None) -> np.ndarray:
        """The voxel centroids, (K, 4) float32.  Raises ICP4RError (ICP4R_E_TOO_LARGE) on grid overflow,
        where PCL warns "Leaf size is too small for the input dataset" and copies its input."""
        cloud = self._cloud if cloud is None else cloud
        a, n, stride = _cloud(cloud)
        out = np.empty((max(n, 1), 4), np.float32)
        k = C.c_int64()
        _check(self._lib.icp4r_voxel_filter(self._ctx.handle, _ptr(a), n, stride, C.byref(self._p), _ptr(out), n,
                                            C.byref(k)), "icp4r_voxel_filter")
        return out[:k.value].copy()

    def filter_device(self, d_points: int, n: int, d_out: int, d_count: int, stream=None):
        """n float4 points at device address d_points -> the centroids (float4, room for n) at d_out and
        their int32 count at d_count (-1: grid overflow), asynchronously on stream."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        _check(self._lib.icp4r_voxel_filter_device(self._ctx.handle, vp(d_points), int(n), C.byref(self._p), vp(d_out),
                                                   vp(d_count), vp(stream)), "icp4r_voxel_filter_device")

    def time_ms(self) -> tuple[float, int]:
        """Mean HIP-event time of the context's filter launches since the last reset, and their number."""
        ms, k = C.c_double(), C.c_int32()
        _check(self._lib.icp4r_voxel_time_ms(self._ctx.handle, C.byref(ms), C.byref(k)), "icp4r_voxel_time_ms")
        return ms.value, k.value

    def reset_timers(self):
        _check(self._lib.icp4r_voxel_time_reset(self._ctx.handle), "icp4r_voxel_time_reset")


class VoxelAccumulator:
    """The incremental voxel grid (include/icp4r/icp4r_voxel_acc.h): hand over each scan once, get the
    downsampled map back.  After any sequence of adds, filter() equals VoxelGrid.filter of the
    concatenation of all added clouds, bit for bit.  The parameters are fixed for the accumulator's life."""

    def __init__(self, leaf, downsample_all_data: bool = True, min_points_per_voxel: int = 0, ctx: Context | None = None):
        self._ctx = ctx or default_context()
        self._lib = load()
        self._p = voxel_params(leaf, downsample_all_data, min_points_per_voxel)
        self._h = C.c_void_p()
        _check(self._lib.icp4r_voxel_acc_create(self._ctx.handle, C.byref(self._p), C.byref(self._h)),
               "icp4r_voxel_acc_create")

    def close(self):
        if self._h:
            self._lib.icp4r_voxel_acc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def params(self) -> VoxelParams:
        return self._p

    def add(self, cloud):
        """One scan, (N, >=3) float32.  Raises ICP4RError (ICP4R_E_TOO_LARGE) when the scan leaves the
        range of +-2^20 cells around the origin; the accumulator is then as it was."""
        a, n, stride = _cloud(cloud)
        _check(self._lib.icp4r_voxel_acc_add(self._h, _ptr(a), n, stride), "icp4r_voxel_acc_add")

    def add_device(self, d_points: int, n: int, stream=None):
        """n float4 points at device address d_points, asynchronously on stream.  A scan outside the range
        is skipped whole and makes filter_device store -2 (filter raise) until clear()."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        _check(self._lib.icp4r_voxel_acc_add_device(self._h, vp(d_points), int(n), vp(stream)), "icp4r_voxel_acc_add_device")

    def add_map(self, tree):
        """The points of a map store (icp4r.mapstore.KD_TREE) of the same context, as one add."""
        _check(self._lib.icp4r_voxel_acc_add_map(self._h, tree.handle), "icp4r_voxel_acc_add_map")

    def size(self) -> tuple[int, int]:
        """(stored voxels, points added)."""
        v, p = C.c_int64(), C.c_int64()
        _check(self._lib.icp4r_voxel_acc_size(self._h, C.byref(v), C.byref(p)), "icp4r_voxel_acc_size")
        return v.value, p.value

    def filter(self) -> np.ndarray:
        """The voxel centroids, (K, 4) float32, in ascending leaf index.  Raises ICP4RError
        (ICP4R_E_TOO_LARGE) on grid overflow and after a device add that left the range."""
        cap = self.size()[0]
        out = np.empty((max(cap, 1), 4), np.float32)
        k = C.c_int64()
        _check(self._lib.icp4r_voxel_acc_filter(self._h, _ptr(out), cap, C.byref(k)), "icp4r_voxel_acc_filter")
        return out[:k.value].copy()

    def filter_device(self, d_out: int, d_count: int, stream=None):
        """The centroids (float4, room for size()[0]) to d_out and their int32 count to d_count (-1: grid
        overflow, -2: a device add left the range), asynchronously on stream."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        _check(self._lib.icp4r_voxel_acc_filter_device(self._h, vp(d_out), vp(d_count), vp(stream)),
               "icp4r_voxel_acc_filter_device")

    def clear(self):
        _check(self._lib.icp4r_voxel_acc_clear(self._h), "icp4r_voxel_acc_clear")

    def reserve(self, voxels: int):
        _check(self._lib.icp4r_voxel_acc_reserve(self._h, int(voxels)), "icp4r_voxel_acc_reserve")
