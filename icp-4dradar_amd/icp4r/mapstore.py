"""Scan-to-map store and sector query (include/icp4r/icp4r_map.h), mirroring the ikd-Tree API the
reference's radar_odometry node uses:

    KD_TREE<PointXYZI> ikd_Tree(0.3, 0.6, 0.5);            radar_odometry.cpp:92
    ikd_Tree.Build(src->points);                            :347
    ikd_Tree.set_downsample_param(0.5);                     :348
    pointAssociateToMap(...); ikd_Tree.Add_Points(.., false) :382-390
    ikd_Tree.Sector_Search(p_now, RADAR_RADIUS, heading, SubMap->points)   :396

and ikd-Tree's map-maintenance calls (ikd_Tree.h:238-245): Nearest_Search, Delete_Point_Boxes,
Box_Search, Radius_Search and the downsampling Add_Points(points, True).

Same method names; clouds are (N, >=3) float32 arrays (x, y, z[, intensity]).  Device-resident and
GPU-only: there is no CPU fallback (the library raises if it is missing).  A tree may outlive its
context: once the context is closed every call on the tree raises and close() only frees the handle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import E_INVALID, Context, ICP4RError, _check, _cloud, _ptr, default_context, load
from .voxel import voxel_params

RADAR_RADIUS = 80.0  # radar_odometry.cpp:36
KNN_MAX_K = 32  # ICP4R_MAP_KNN_MAX_K
KNN_BRUTE = 1   # ICP4R_MAP_KNN_BRUTE: every stored point, no index
KNN_INDEX = 2   # ICP4R_MAP_KNN_INDEX: the index whatever the map's size


class KD_TREE:  # noqa: N801 — the reference's class name
    """ikd-Tree replacement for radar_odometry's map: a dense device store in insertion order with
    Sector_Search, Box_Search and Radius_Search as full filters, box deletion, the downsampling
    insert, and an exact batched Nearest_Search over a Morton-order index the store keeps of itself.  ikd-Tree's rebuild / rebalancing have no counterpart; the one result they touch is the
    reference's Sector_Search after a deletion or a downsampling add, which may also return lazily
    deleted points with |dh| > 300 until a rebuild drops them — this store never does
    (include/icp4r/icp4r_map.h)."""

    def __init__(self, delete_param: float = 0.5, balance_param: float = 0.6, box_length: float | None = None,
                 ctx: Context | None = None):
        # delete/balance parameters steer ikd-Tree's rebalancing, which has no counterpart here;
        # box_length is the downsample box of Add_Points(.., True) (the node adds with downsample_on = false).
        # A tree that was never given a box (constructor or set_downsample_param) shows ikd-Tree's default
        # of 0.2 but refuses Add_Points(.., True), as every tree did before the downsampling insert existed.
        self.delete_param, self.balance_param = delete_param, balance_param
        self.downsample_size = 0.2 if box_length is None else box_length
        self._box_given = box_length is not None
        self._ctx = ctx or default_context()
        self._lib = load()
        self._h = C.c_void_p()
        _check(self._lib.icp4r_map_create(self._ctx.handle, C.byref(self._h)), "icp4r_map_create")

    def close(self):
        if self._h:
            self._lib.icp4r_map_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- the reference's method names ------------------------------------------------------------
    def Build(self, points):  # noqa: N802
        a, n, stride = _cloud(points)
        _check(self._lib.icp4r_map_build(self._h, _ptr(a), n, stride), "icp4r_map_build")

    def set_downsample_param(self, box_length: float):
        self.downsample_size = box_length
        self._box_given = True

    def Add_Points(self, points, downsample_on: bool = False) -> int:  # noqa: N802
        """ikd-Tree's return value: the downsample counter, 0 without downsampling."""
        a, n, stride = _cloud(points)
        if downsample_on:
            if not self._box_given:
                raise ICP4RError(E_INVALID, "Add_Points(.., True): give the tree its downsample box first "
                                            "(box_length or set_downsample_param)")
            k = C.c_int64()
            _check(self._lib.icp4r_map_add_points_downsample(self._h, _ptr(a), n, stride, float(self.downsample_size),
                                                             C.byref(k)), "icp4r_map_add_points_downsample")
            return k.value
        _check(self._lib.icp4r_map_add_points(self._h, _ptr(a), n, stride, 0), "icp4r_map_add_points")
        return 0

    def Delete_Point_Boxes(self, boxes) -> int:  # noqa: N802
        """Removes the points inside any box ((nb, 6): min xyz, max xyz; min <= p < max); -> how many."""
        b = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 6))
        k = C.c_int64()
        _check(self._lib.icp4r_map_delete_boxes(self._h, _ptr(b) if len(b) else None, len(b), C.byref(k)),
               "icp4r_map_delete_boxes")
        return k.value

    def _search(self, fn, name, *args) -> np.ndarray:
        cap = self.size()
        out = np.empty((max(cap, 1), 4), np.float32)
        k = C.c_int64()
        _check(fn(self._h, *args, _ptr(out), cap, C.byref(k)), name)
        return out[:k.value].copy()

    def Box_Search(self, box) -> np.ndarray:  # noqa: N802
        """The stored points with min <= p < max, (K, 4) float32, insertion order.  box: 6 floats."""
        b = np.ascontiguousarray(np.asarray(box, np.float32).reshape(6))
        return self._search(self._lib.icp4r_map_box_search, "icp4r_map_box_search", _ptr(b))

    def Radius_Search(self, point, radius: float) -> np.ndarray:  # noqa: N802
        """The stored points with calc_dist(p, point) <= radius^2 (float), (K, 4) float32, insertion order."""
        c = np.ascontiguousarray(np.asarray(point, np.float32).reshape(-1)[:3])
        return self._search(self._lib.icp4r_map_radius_search, "icp4r_map_radius_search", _ptr(c), float(radius))

    def Sector_Search(self, point, radius: float, heading: float) -> np.ndarray:  # noqa: N802
        """The kept points, (K, 4) float32, insertion order (ikd-Tree: the same set, tree order)."""
        c = np.ascontiguousarray(np.asarray(point, np.float32).reshape(-1)[:3])
        cap = self.size()
        out = np.empty((max(cap, 1), 4), np.float32)
        k = C.c_int64()
        _check(self._lib.icp4r_map_sector_search(self._h, _ptr(c), float(radius), float(heading), _ptr(out), cap,
                                                 C.byref(k)), "icp4r_map_sector_search")
        return out[:k.value].copy()

    def Nearest_Search(self, point, k_nearest: int, max_dist: float = float("inf")):  # noqa: N802
        """The reference's call for one point: (points (K', 4), squared distances (K',)), nearest first,
        K' = min(k_nearest, stored points within max_dist).  One call pays a launch and a
        synchronisation: hand a whole scan to nearest_search instead."""
        q = np.asarray(point, np.float32).reshape(-1)[:3].reshape(1, 3)
        pts, dist, _, found = self.nearest_search(q, k_nearest, max_dist)
        return pts[0, :found[0]].copy(), dist[0, :found[0]].copy()

    def nearest_search(self, queries, k: int, max_dist: float = float("inf"), brute: bool = False, flags: int = 0):
        """Batched Nearest_Search: the k nearest stored points of every query (include/icp4r/icp4r_map.h).
        -> points (nq, k, 4) float32, squared distances (nq, k) float32, insertion positions (nq, k) int32
        and found (nq,) int32; a row's unused slots hold a zero point, +inf and -1.  brute: no index."""
        a, nq, stride = _cloud(queries)
        kk = max(int(k), 0)
        pts = np.empty((nq, kk, 4), np.float32)
        dist = np.empty((nq, kk), np.float32)
        idx = np.empty((nq, kk), np.int32)
        found = np.empty((nq,), np.int32)
        _check(self._lib.icp4r_map_nearest_search(self._h, _ptr(a), nq, stride, int(k), float(max_dist),
                                                  int(flags) | (KNN_BRUTE if brute else 0), _ptr(pts), _ptr(dist),
                                                  _ptr(idx), _ptr(found)), "icp4r_map_nearest_search")
        return pts, dist, idx, found

    def voxel_filter(self, leaf, downsample_all_data: bool = True, min_points_per_voxel: int = 0) -> np.ndarray:
        """pcl::VoxelGrid over the stored points (the node's surround map, radar_odometry.cpp:426-429;
        include/icp4r/icp4r_voxel.h): (K, 4) float32 centroids in ascending leaf index.  leaf: one float
        or three.  The store and its k-NN index are left as they are."""
        p = voxel_params(leaf, downsample_all_data, min_points_per_voxel)
        cap = self.size()
        out = np.empty((max(cap, 1), 4), np.float32)
        k = C.c_int64()
        _check(self._lib.icp4r_map_voxel_filter(self._h, C.byref(p), _ptr(out), cap, C.byref(k)), "icp4r_map_voxel_filter")
        return out[:k.value].copy()

    def index_build(self):
        """Brings the k-NN index up to date now (a search does so by itself when it has to)."""
        _check(self._lib.icp4r_map_index_build(self._h), "icp4r_map_index_build")

    def index_stats(self) -> dict:
        """indexed: points the index covers; tail: appended since; tail_limit: the tail past which the next
        search rebuilds; builds: index builds so far."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        _check(self._lib.icp4r_map_index_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)),
               "icp4r_map_index_stats")
        return {"indexed": a.value, "tail": b.value, "tail_limit": c.value, "builds": d.value}

    def size(self) -> int:
        n = C.c_int64()
        _check(self._lib.icp4r_map_size(self._h, C.byref(n)), "icp4r_map_size")
        return n.value

    # -- radar_odometry's insertion step ---------------------------------------------------------
    def add_scan(self, scan, R, t, want_world: bool = False):
        """pointAssociateToMap (p_w = R p + t in double, stored as float) + Add_Points(.., false)."""
        a, n, stride = _cloud(scan)
        Rd = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
        td = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
        out = np.empty((n, 4), np.float32) if want_world else None
        _check(self._lib.icp4r_map_add_scan(self._h, _ptr(a), n, stride, _ptr(Rd), _ptr(td),
                                            _ptr(out) if out is not None else None), "icp4r_map_add_scan")
        return out

    # -- device-resident pipeline ----------------------------------------------------------------
    def sector_search_device(self, point, radius: float, heading: float, d_out: int, d_count: int, stream=None):
        """Writes the kept points (float4) to device address d_out and their int32 count to d_count."""
        c = np.ascontiguousarray(np.asarray(point, np.float32).reshape(-1)[:3])
        _check(self._lib.icp4r_map_sector_search_device(self._h, _ptr(c), float(radius), float(heading),
                                                        C.c_void_p(d_out), C.c_void_p(d_count),
                                                        C.c_void_p(stream) if stream else None),
               "icp4r_map_sector_search_device")

    def box_search_device(self, box, d_out: int, d_count: int, stream=None):
        b = np.ascontiguousarray(np.asarray(box, np.float32).reshape(6))
        _check(self._lib.icp4r_map_box_search_device(self._h, _ptr(b), C.c_void_p(d_out), C.c_void_p(d_count),
                                                     C.c_void_p(stream) if stream else None),
               "icp4r_map_box_search_device")

    def radius_search_device(self, point, radius: float, d_out: int, d_count: int, stream=None):
        c = np.ascontiguousarray(np.asarray(point, np.float32).reshape(-1)[:3])
        _check(self._lib.icp4r_map_radius_search_device(self._h, _ptr(c), float(radius), C.c_void_p(d_out),
                                                        C.c_void_p(d_count), C.c_void_p(stream) if stream else None),
               "icp4r_map_radius_search_device")

    def nearest_search_device(self, d_queries: int, nq: int, k: int, max_dist: float = float("inf"), d_points: int = 0,
                              d_dist: int = 0, d_index: int = 0, d_found: int = 0, stream=None, flags: int = 0):
        """nq float4 queries at device address d_queries; any of the four device outputs may be 0."""
        vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        _check(self._lib.icp4r_map_nearest_search_device(self._h, vp(d_queries), nq, int(k), float(max_dist), int(flags),
                                                         vp(d_points), vp(d_dist), vp(d_index), vp(d_found),
                                                         vp(stream)), "icp4r_map_nearest_search_device")

    def voxel_filter_device(self, leaf, d_out: int, d_count: int, downsample_all_data: bool = True,
                            min_points_per_voxel: int = 0, stream=None):
        """The store's voxel centroids (float4, room for size() points) to device address d_out and their
        int32 count to d_count (-1: grid overflow); nothing leaves the device and the store is unchanged."""
        p = voxel_params(leaf, downsample_all_data, min_points_per_voxel)
        _check(self._lib.icp4r_map_voxel_filter_device(self._h, C.byref(p), C.c_void_p(d_out), C.c_void_p(d_count),
                                                       C.c_void_p(stream) if stream else None),
               "icp4r_map_voxel_filter_device")

    def points_device(self) -> tuple[int, int]:
        p, n = C.c_void_p(), C.c_int64()
        _check(self._lib.icp4r_map_points_device(self._h, C.byref(p), C.byref(n)), "icp4r_map_points_device")
        return p.value or 0, n.value

    def time_ms(self) -> tuple[float, int]:
        ms, k = C.c_double(), C.c_int32()
        _check(self._lib.icp4r_map_time_ms(self._h, C.byref(ms), C.byref(k)), "icp4r_map_time_ms")
        return ms.value, k.value

    def reset_timers(self):
        _check(self._lib.icp4r_map_time_reset(self._h), "icp4r_map_time_reset")
