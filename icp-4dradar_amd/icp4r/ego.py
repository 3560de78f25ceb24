"""Radar ego velocity and the scan parse (include/icp4r/icp4r_ego.h), mirroring the reference node's
per-frame code around its ICP call (src/iterative_closest_point.cpp):

    fitSineRansac(points, A_best, b_best, iterations, sigma)        :85-128   -> fitSineRansac()
    parse of the 5-float records into RadarPoint_Info2               :354-385  -> radar_features()
    static / dynamic split, Vxyz = (KᵀK)⁻¹ Kᵀ Vr                     :391-431  -> ego_velocity()

GPU-only: there is no CPU fallback (the library raises if it is missing).  Hypothesis pairs are
drawn reproducibly (SplitMix64 of seed + k, mod n) — the reference's std::random_device draw with
an inclusive upper bound is one of the bugs this fixes (icp4r_ego.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import RESULT_DTYPE, Context, Params, _check, _ptr, default_context, load

SIGMA = 0.5              # fitSineRansac's default (:89)
DYNAMIC_THRESHOLD = 0.2  # :396
# include/icp4r/icp4r_gate.h: the Doppler gate (ICP over each scan's static points, USE_STATIC_POINTS)
GATE_STATIC, GATE_ALL = 0, 1
PAIR_NODE, PAIR_STRICT = 0, 1
GATE_TILE = 1024         # points per (scan, tile) of the compaction (kGateTile, csrc/icp4r_internal.hpp)


class EgoParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("reserved0", C.c_int32), ("sigma", C.c_double),
                ("dynamic_threshold", C.c_double), ("seed", C.c_uint64), ("reserved", C.c_int32 * 8)]


class EgoResult(C.Structure):
    _fields_ = [("A", C.c_double), ("b", C.c_double), ("v", C.c_double * 3), ("score", C.c_double),
                ("n", C.c_int32), ("n_static", C.c_int32), ("iterations", C.c_int32), ("best", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]

    def velocity(self) -> np.ndarray:
        return np.array(self.v, np.float64)


assert C.sizeof(EgoResult) == 72
EGO_RESULT_DTYPE = np.dtype([("A", np.float64), ("b", np.float64), ("v", np.float64, 3), ("score", np.float64),
                             ("n", np.int32), ("n_static", np.int32), ("iterations", np.int32), ("best", np.int32),
                             ("status", np.int32), ("reserved", np.int32)])
assert EGO_RESULT_DTYPE.itemsize == 72

_bound = False


def _lib():
    global _bound
    L = load()
    if not _bound:
        vp, i32 = C.c_void_p, C.c_int32
        L.icp4r_ego_params_default.restype = None
        L.icp4r_ego_params_default.argtypes = [C.POINTER(EgoParams)]
        L.icp4r_radar_features.restype = C.c_int
        L.icp4r_radar_features.argtypes = [vp, vp, i32, vp, vp]
        L.icp4r_ego_velocity.restype = C.c_int
        L.icp4r_ego_velocity.argtypes = [vp, vp, i32, C.POINTER(EgoParams), C.POINTER(EgoResult), vp, vp]
        L.icp4r_ego_velocity_batch_device.restype = C.c_int
        L.icp4r_ego_velocity_batch_device.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(EgoParams), vp, vp, vp]
        # icp4r_gate.h
        L.icp4r_compact_by_mask_batch_device.restype = C.c_int
        L.icp4r_compact_by_mask_batch_device.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
        L.icp4r_static_clouds_batch_device.restype = C.c_int
        L.icp4r_static_clouds_batch_device.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(EgoParams), i32, vp, vp, vp,
                                                       vp, vp, vp]
        L.icp4r_static_cloud.restype = C.c_int
        L.icp4r_static_cloud.argtypes = [vp, vp, i32, C.POINTER(EgoParams), C.POINTER(EgoResult), vp, C.POINTER(i32)]
        L.icp4r_sequence_pairs.restype = C.c_int
        L.icp4r_sequence_pairs.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        L.icp4r_register_static_sequence.restype = C.c_int
        L.icp4r_register_static_sequence.argtypes = [vp, vp, vp, vp, i32, C.POINTER(EgoParams), C.POINTER(Params), i32,
                                                     i32, vp, vp, vp]
        L.icp4r_register_static_sequence_ex.restype = C.c_int
        L.icp4r_register_static_sequence_ex.argtypes = L.icp4r_register_static_sequence.argtypes + [vp, vp, vp]
        _bound = True
    return L


def default_params(**kw) -> EgoParams:
    p = EgoParams()
    _lib().icp4r_ego_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _records(rec) -> np.ndarray:
    rec = np.ascontiguousarray(rec, dtype=np.float32)
    if rec.ndim != 2 or rec.shape[1] != 5:
        raise ValueError(f"records must be (N, 5) float32 [x, y, z, intensity, v_r], got {rec.shape}")
    return rec


def radar_features(records, ctx: Context | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(xyzi (N, 4): the PointXYZI cloud, feat (N, 4): distance, arfa, beta [deg], v_r)."""
    rec = _records(records)
    n = len(rec)
    xyzi = np.zeros((n, 4), np.float32)
    feat = np.zeros((n, 4), np.float32)
    ctx = ctx or default_context()
    _check(_lib().icp4r_radar_features(ctx.handle, _ptr(rec), n, _ptr(xyzi), _ptr(feat)), "icp4r_radar_features")
    return xyzi, feat


def ego_velocity(records, params: EgoParams | None = None, ctx: Context | None = None, want_mask: bool = False,
                 want_scores: bool = False):
    """Ego velocity of one scan: (EgoResult, static mask or None, per-hypothesis scores or None)."""
    rec = _records(records)
    n = len(rec)
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    r = EgoResult()
    mask = np.zeros(n, np.uint8) if want_mask else None
    H = p.iterations if p.iterations > 0 else int(n * 0.2)
    scores = np.zeros(max(H, 0), np.float64) if want_scores else None
    rc = _lib().icp4r_ego_velocity(ctx.handle, _ptr(rec), n, C.byref(p), C.byref(r),
                                   _ptr(mask) if mask is not None else None,
                                   _ptr(scores) if scores is not None and scores.size else None)
    _check(rc, "icp4r_ego_velocity")
    return r, mask, scores


def ego_velocity_batch_device(records_ptr: int, off_ptr: int, cnt_ptr: int, nscans: int, max_n: int,
                              results_ptr: int, params: EgoParams | None = None, mask_ptr: int | None = None,
                              ctx: Context | None = None, stream: int | None = None):
    """Many scans already in HBM (device pointers); asynchronous on `stream`."""
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    _check(_lib().icp4r_ego_velocity_batch_device(ctx.handle, records_ptr, off_ptr, cnt_ptr, nscans, max_n,
                                                  C.byref(p), results_ptr, mask_ptr,
                                                  C.c_void_p(stream) if stream else None),
           "icp4r_ego_velocity_batch_device")


def fitSineRansac(points, A_best: float = 0.0, b_best: float = 0.0, iterations: int | None = None,  # noqa: N802
                  sigma: float = SIGMA, seed: int | None = None, ctx: Context | None = None):
    """The node's fitSineRansac (:85-128) on a scan's records: returns (A_best, b_best, best score).
    A_best / b_best keep the values passed in when no hypothesis scores > 0."""
    kw = {"sigma": sigma}
    if iterations is not None:
        kw["iterations"] = int(iterations)
    if seed is not None:
        kw["seed"] = seed
    r, _, _ = ego_velocity(points, default_params(**kw), ctx)
    if r.best < 0:
        return A_best, b_best, r.score
    return r.A, r.b, r.score


# ---------------------------------------------------------------------------------------------------
# Doppler-gated registration (include/icp4r/icp4r_gate.h): the node built with USE_STATIC_POINTS.

def static_cloud(records, params: EgoParams | None = None, ctx: Context | None = None):
    """One scan's ego velocity and its static points (icp4r_static_cloud): (EgoResult, (n_static, 4)
    xyzi in input order) — what the node pushes into cloud_src_in with USE_STATIC_POINTS (:404-406)."""
    rec = _records(records)
    n = len(rec)
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    r = EgoResult()
    out = np.zeros((n, 4), np.float32)
    ns = C.c_int32(0)
    rc = _lib().icp4r_static_cloud(ctx.handle, _ptr(rec), n, C.byref(p), C.byref(r), _ptr(out), C.byref(ns))
    _check(rc, "icp4r_static_cloud")
    return r, out[:ns.value].copy()


def compact_by_mask_batch_device(xyzi_ptr: int, off_ptr: int, cnt_ptr: int, mask_ptr: int | None, nscans: int,
                                 max_n: int, clouds_ptr: int, pair_off_ptr: int, pair_n_ptr: int,
                                 mode: int = GATE_STATIC, ctx: Context | None = None, stream: int | None = None):
    """The gate's compaction on a caller's mask, everything in HBM (device pointers); asynchronous on
    `stream`.  pair_off (int64) / pair_n (int32) hold nscans + 1 entries: [s0, s0, s1, ...]."""
    ctx = ctx or default_context()
    _check(_lib().icp4r_compact_by_mask_batch_device(ctx.handle, xyzi_ptr, off_ptr, cnt_ptr, mask_ptr, nscans, max_n,
                                                     mode, clouds_ptr, pair_off_ptr, pair_n_ptr,
                                                     C.c_void_p(stream) if stream else None),
           "icp4r_compact_by_mask_batch_device")


def static_clouds_batch_device(records_ptr: int, off_ptr: int, cnt_ptr: int, nscans: int, max_n: int,
                               results_ptr: int, clouds_ptr: int, pair_off_ptr: int, pair_n_ptr: int,
                               params: EgoParams | None = None, mode: int = GATE_STATIC, mask_ptr: int | None = None,
                               ctx: Context | None = None, stream: int | None = None):
    """Ego velocity then the gate for many scans in HBM (device pointers); asynchronous on `stream`."""
    p = params if params is not None else default_params()
    ctx = ctx or default_context()
    _check(_lib().icp4r_static_clouds_batch_device(ctx.handle, records_ptr, off_ptr, cnt_ptr, nscans, max_n, C.byref(p),
                                                   mode, results_ptr, mask_ptr, clouds_ptr, pair_off_ptr, pair_n_ptr,
                                                   C.c_void_p(stream) if stream else None),
           "icp4r_static_clouds_batch_device")


def sequence_pairs(counts):
    """icp4r_sequence_pairs (pure host): the node's running-cloud rule over per-scan point counts.
    Returns (src_first, src_last, tgt_first, tgt_last, registered), int32 arrays of len(counts): frame
    k's clouds are the inclusive scan ranges [src_first[k], src_last[k]] and [tgt_first[k], tgt_last[k]]."""
    c = np.ascontiguousarray(counts, np.int32).reshape(-1)
    out = [np.zeros(len(c), np.int32) for _ in range(5)]
    _check(_lib().icp4r_sequence_pairs(_ptr(c), len(c), *[_ptr(o) for o in out]), "icp4r_sequence_pairs")
    return tuple(out)


def register_static_sequence(frames, mode: int = GATE_STATIC, pairing: int = PAIR_NODE,
                             ego_params: EgoParams | None = None, icp_params: Params | None = None,
                             ctx: Context | None = None, want_masks: bool = False, want_clouds: bool = False):
    """A whole sequence in one call (icp4r_register_static_sequence): frames = a list of (N_k, 5)
    records.  Returns (ego results (EGO_RESULT_DTYPE), ICP results (RESULT_DTYPE, frame k at k),
    registered (int32, 0: a frame the node skips)), then on request the per-scan masks (a list of
    uint8 arrays) and the packed clouds (a list of (n_k, 4) arrays, scan k's kept points)."""
    recs = [_records(f) for f in frames]
    ns = len(recs)
    cnt = np.array([len(r) for r in recs], np.int32)
    off = np.zeros(ns, np.int64)
    if ns:
        off[1:] = np.cumsum(cnt[:-1], dtype=np.int64)
    flat = np.ascontiguousarray(np.concatenate(recs)) if ns else np.zeros((0, 5), np.float32)
    ego_res = np.zeros(ns, EGO_RESULT_DTYPE)
    icp_res = np.zeros(ns, RESULT_DTYPE)
    registered = np.zeros(ns, np.int32)
    mask = np.zeros(len(flat), np.uint8)
    clouds = np.zeros((len(flat), 4), np.float32)
    pair_n = np.zeros(ns + 1, np.int32)
    p = ego_params if ego_params is not None else default_params()
    ctx = ctx or default_context()
    ip = C.byref(icp_params) if icp_params is not None else None
    if want_masks or want_clouds:
        rc = _lib().icp4r_register_static_sequence_ex(ctx.handle, _ptr(flat), _ptr(off), _ptr(cnt), ns, C.byref(p), ip,
                                                      mode, pairing, _ptr(ego_res), _ptr(icp_res), _ptr(registered),
                                                      _ptr(mask), _ptr(clouds), _ptr(pair_n))
    else:
        rc = _lib().icp4r_register_static_sequence(ctx.handle, _ptr(flat), _ptr(off), _ptr(cnt), ns, C.byref(p), ip,
                                                   mode, pairing, _ptr(ego_res), _ptr(icp_res), _ptr(registered))
    _check(rc, "icp4r_register_static_sequence")
    out = [ego_res, icp_res, registered]
    if want_masks:
        out.append([mask[o:o + n].copy() for o, n in zip(off, cnt)])
    if want_clouds:
        po = np.concatenate([[0], np.cumsum(pair_n[1:], dtype=np.int64)])
        out.append([clouds[po[k]:po[k + 1]].copy() for k in range(ns)])
    return tuple(out)
