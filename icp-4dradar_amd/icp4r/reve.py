"""3D Doppler ego velocity and inlier scans (include/icp4r/icp4r_reve.h): the first step of every
radar_odometry frame of the reference,

    radar_ego_velocity.estimate(radar_data_msg, v_r, sigma_v_r, inlier_radar_scan)   src/radar_odometry.cpp:328

restated from reve::RadarEgoVelocityEstimator with the settings of config_init (:574-611): the valid
filter, the standstill test, three-point least-squares RANSAC, the refit and its standard deviation.
GPU-only: there is no CPU fallback.  The inlier scans come back in the gate's packed layout
(icp4r_gate.h), so icp4r_align_batch_device and every other batch consumer take them as they are.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import REVE_EXPORTED_SYMBOLS, Context, _check, _ptr, default_context, load  # noqa: F401

MAX_ITERATIONS = 256   # ICP4R_REVE_MAX_ITERATIONS
MAX_POINTS = 262144    # ICP4R_REVE_MAX_POINTS

_DOUBLES = ["min_dist", "max_dist", "min_db", "elevation_thresh_deg", "azimuth_thresh_deg", "filter_min_z",
            "filter_max_z", "doppler_velocity_correction_factor", "thresh_zero_velocity",
            "allowed_outlier_percentage", "sigma_zero_velocity_x", "sigma_zero_velocity_y", "sigma_zero_velocity_z",
            "sigma_offset_radar_x", "sigma_offset_radar_y", "sigma_offset_radar_z", "max_sigma_x", "max_sigma_y",
            "max_sigma_z", "max_r_cond", "outlier_prob", "success_prob", "inlier_thresh", "sigma_v_d", "min_speed_odr",
            "model_noise_offset_deg", "model_noise_scale_deg"]
_INTS = ["use_cholesky_instead_of_bdcsvd", "use_ransac", "N_ransac_points", "use_odr"]


class ReveParams(C.Structure):
    _fields_ = ([(k, C.c_double) for k in _DOUBLES] + [(k, C.c_int32) for k in _INTS] +
                [("seed", C.c_uint64), ("use_z_filter", C.c_int32), ("reserved", C.c_int32 * 7)])

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k in _DOUBLES + _INTS + ["seed", "use_z_filter"]}


class ReveResult(C.Structure):
    _fields_ = [("v", C.c_double * 3), ("sigma", C.c_double * 3), ("n", C.c_int32), ("n_valid", C.c_int32),
                ("n_inliers", C.c_int32), ("iterations", C.c_int32), ("accepted", C.c_int32), ("best", C.c_int32),
                ("zero_velocity", C.c_int32), ("success", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]

    def velocity(self) -> np.ndarray:
        return np.array(self.v, np.float64)

    def stddev(self) -> np.ndarray:
        return np.array(self.sigma, np.float64)


assert C.sizeof(ReveParams) == 272 and C.sizeof(ReveResult) == 88
REVE_RESULT_DTYPE = np.dtype([("v", np.float64, 3), ("sigma", np.float64, 3), ("n", np.int32), ("n_valid", np.int32),
                              ("n_inliers", np.int32), ("iterations", np.int32), ("accepted", np.int32),
                              ("best", np.int32), ("zero_velocity", np.int32), ("success", np.int32),
                              ("status", np.int32), ("reserved", np.int32)])
assert REVE_RESULT_DTYPE.itemsize == 88

_bound = False


def _lib():
    global _bound
    L = load()
    if not _bound:
        vp, i32, pp, pr = C.c_void_p, C.c_int32, C.POINTER(ReveParams), C.POINTER(ReveResult)
        L.icp4r_reve_params_default.restype = None
        L.icp4r_reve_params_default.argtypes = [pp]
        L.icp4r_reve_ransac_iterations.restype = i32
        L.icp4r_reve_ransac_iterations.argtypes = [pp]
        L.icp4r_reve_draw.restype = C.c_int
        L.icp4r_reve_draw.argtypes = [C.c_uint64, i32, i32, C.POINTER(i32 * 3)]
        L.icp4r_reve_batch_device.restype = C.c_int
        L.icp4r_reve_batch_device.argtypes = [vp, vp, vp, vp, i32, i32, pp, vp, vp, vp]
        L.icp4r_reve_inlier_clouds_batch_device.restype = C.c_int
        L.icp4r_reve_inlier_clouds_batch_device.argtypes = [vp, vp, vp, vp, i32, i32, pp, vp, vp, vp, vp, vp, vp]
        L.icp4r_reve_estimate.restype = C.c_int
        L.icp4r_reve_estimate.argtypes = [vp, vp, i32, pp, pr, vp]
        L.icp4r_reve_inlier_cloud.restype = C.c_int
        L.icp4r_reve_inlier_cloud.argtypes = [vp, vp, i32, pp, pr, vp, C.POINTER(i32)]
        _bound = True
    return L


def default_params(**kw) -> ReveParams:
    """The node's settings (config_init); keyword arguments override fields by name."""
    p = ReveParams()
    _lib().icp4r_reve_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in _DOUBLES + _INTS + ["seed", "use_z_filter"]:
            raise AttributeError(f"icp4r_reve_params has no field {k!r}")
        setattr(p, k, v)
    return p


def ransac_iterations(params: ReveParams | None = None) -> int:
    """icp4r_reve_ransac_iterations (pure host): the hypothesis count of the settings."""
    p = params if params is not None else default_params()
    return int(_lib().icp4r_reve_ransac_iterations(C.byref(p)))


def draw(seed: int, k: int, n_valid: int) -> tuple[int, int, int]:
    """icp4r_reve_draw (pure host): the three valid-list indices of hypothesis k."""
    out = (C.c_int32 * 3)()
    _check(_lib().icp4r_reve_draw(C.c_uint64(seed & (2 ** 64 - 1)), k, n_valid, C.byref(out)), "icp4r_reve_draw")
    return int(out[0]), int(out[1]), int(out[2])


def _records(rec) -> np.ndarray:
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    if rec.ndim != 2 or rec.shape[1] != 5:
        raise ValueError(f"records must be (N, 5) float32 [x, y, z, intensity, doppler], got {rec.shape}")
    return rec


def estimate(records, params: ReveParams | None = None, ctx: Context | None = None, want_mask: bool = False):
    """One scan (icp4r_reve_estimate): (ReveResult, inlier mask or None)."""
    rec = _records(records)
    n = len(rec)
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    r = ReveResult()
    mask = np.zeros(n, np.uint8) if want_mask else None
    rc = _lib().icp4r_reve_estimate(ctx.handle, _ptr(rec), n, C.byref(p), C.byref(r),
                                    _ptr(mask) if mask is not None and n else None)
    _check(rc, "icp4r_reve_estimate")
    return r, mask


def inlier_cloud(records, params: ReveParams | None = None, ctx: Context | None = None):
    """One scan (icp4r_reve_inlier_cloud): (ReveResult, (n_inliers, 4) xyzi in input order) — the cloud the
    node fills `src` with (:329-342)."""
    rec = _records(records)
    n = len(rec)
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    r = ReveResult()
    out = np.zeros((n, 4), np.float32)
    ni = C.c_int32(0)
    rc = _lib().icp4r_reve_inlier_cloud(ctx.handle, _ptr(rec), n, C.byref(p), C.byref(r), _ptr(out), C.byref(ni))
    _check(rc, "icp4r_reve_inlier_cloud")
    return r, out[:ni.value].copy()


def estimate_batch_device(records_ptr: int, off_ptr: int, cnt_ptr: int, nscans: int, max_n: int, results_ptr: int,
                          params: ReveParams | None = None, mask_ptr: int | None = None, ctx: Context | None = None,
                          stream: int | None = None):
    """Many scans already in HBM (device pointers); asynchronous on `stream`.  results: nscans rows of
    REVE_RESULT_DTYPE; mask: one byte per record or None."""
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    _check(_lib().icp4r_reve_batch_device(ctx.handle, records_ptr, off_ptr, cnt_ptr, nscans, max_n, C.byref(p),
                                          results_ptr, mask_ptr, C.c_void_p(stream) if stream else None),
           "icp4r_reve_batch_device")


def inlier_clouds_batch_device(records_ptr: int, off_ptr: int, cnt_ptr: int, nscans: int, max_n: int, results_ptr: int,
                               clouds_ptr: int, pair_off_ptr: int, pair_n_ptr: int, params: ReveParams | None = None,
                               mask_ptr: int | None = None, ctx: Context | None = None, stream: int | None = None):
    """The estimator then the gate's compaction for many scans in HBM (device pointers); asynchronous on
    `stream`.  pair_off (int64) / pair_n (int32) hold nscans + 1 entries: [s0, s0, s1, ...]."""
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    _check(_lib().icp4r_reve_inlier_clouds_batch_device(ctx.handle, records_ptr, off_ptr, cnt_ptr, nscans, max_n,
                                                        C.byref(p), results_ptr, mask_ptr, clouds_ptr, pair_off_ptr,
                                                        pair_n_ptr, C.c_void_p(stream) if stream else None),
           "icp4r_reve_inlier_clouds_batch_device")
