"""Voxelized generalized ICP (include/icp4r/icp4r_vgicp.h), mirroring fast_gicp::FastVGICP: the target
becomes a map of Gaussian voxels and a correspondence is a voxel lookup at the transformed source point.

    fast_gicp::FastVGICP<PointXYZI, PointXYZI> vgicp;                    -> FastVGICP()
    vgicp.setResolution(1.0);                                            -> setResolution
    vgicp.setNeighborSearchMethod(fast_gicp::NeighborSearchMethod::DIRECT7);  -> setNeighborSearchMethod
    vgicp.setInputTarget(map); vgicp.setInputSource(scan); vgicp.align(out);  -> same names

GPU-only: there is no CPU fallback (the library raises if it is missing).  fast_gicp itself is not in
this image; the algorithm restated is described in icp4r_vgicp.h and tests/vgicp_twin.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import (E_EMPTY, E_INVALID, E_NONFINITE, OK, VGICP_EXPORTED_SYMBOLS, Batch, Context, Result, _check,  # noqa: F401
               _cloud, _ptr, default_context, load)
from . import gicp as _gicp
from .gicp import GicpParams

DIRECT1, DIRECT7, DIRECT27, DIRECT_RADIUS = 0, 1, 2, 3  # fast_gicp::NeighborSearchMethod
ADDITIVE, ADDITIVE_WEIGHTED, MULTIPLICATIVE = 0, 1, 2   # fast_gicp::VoxelAccumulationMode


class VgicpParams(C.Structure):
    _fields_ = [("gicp", GicpParams), ("voxel_resolution", C.c_double), ("neighbor_search", C.c_int32),
                ("voxel_accumulation", C.c_int32), ("reserved", C.c_int32 * 8)]


_bound = False


def _lib():
    global _bound
    L = load()
    if not _bound:
        vp, i32 = C.c_void_p, C.c_int32
        L.icp4r_vgicp_params_default.restype = None
        L.icp4r_vgicp_params_default.argtypes = [C.POINTER(VgicpParams)]
        L.icp4r_vgicp_align.restype = C.c_int
        L.icp4r_vgicp_align.argtypes = [vp, vp, i32, i32, vp, i32, i32, vp, C.POINTER(VgicpParams), C.POINTER(Result),
                                        vp, i32]
        L.icp4r_vgicp_align_batch_device.restype = C.c_int
        L.icp4r_vgicp_align_batch_device.argtypes = [vp, C.POINTER(Batch), C.POINTER(VgicpParams), vp, vp]
        L.icp4r_vgicp_voxel_map.restype = C.c_int
        L.icp4r_vgicp_voxel_map.argtypes = [vp, vp, i32, i32, vp, i32, i32, C.c_double, i32, vp, vp, vp, vp,
                                            C.POINTER(i32)]
        _bound = True
    return L


def default_params(**kw) -> VgicpParams:
    """fast_gicp's defaults; a keyword names a field of VgicpParams or of its GICP part."""
    p = VgicpParams()
    _lib().icp4r_vgicp_params_default(C.byref(p))
    own = {f[0] for f in VgicpParams._fields_}
    for k, v in kw.items():
        setattr(p if k in own else p.gicp, k, v)
    return p


def align(src, tgt, params: VgicpParams | None = None, guess=None, want_aligned: bool = False,
          ctx: Context | None = None) -> tuple[Result, np.ndarray | None]:
    """One pair from host arrays (N, >=3) float32; guess row-major 4x4 or None."""
    ctx = ctx or default_context()
    s, n, ss = _cloud(src)
    t, m, ts = _cloud(tgt)
    p = params if params is not None else default_params()
    g = None if guess is None else np.ascontiguousarray(np.asarray(guess, np.float32).T.reshape(16))
    out = np.zeros((n, 4), np.float32) if want_aligned else None
    r = Result()
    rc = _lib().icp4r_vgicp_align(ctx.handle, _ptr(s), n, ss, _ptr(t), m, ts, _ptr(g) if g is not None else None,
                                  C.byref(p), C.byref(r), _ptr(out) if out is not None else None, 16)
    if rc not in (OK, E_EMPTY, E_NONFINITE) and not (rc == E_INVALID and r.status == E_INVALID):
        _check(rc, "icp4r_vgicp_align")
    return r, out


def align_batch_device(batch: Batch, params: VgicpParams, results_ptr: int, stream: int | None = None,
                       ctx: Context | None = None):
    """Device-resident batch (icp4r_batch of torch.cuda tensor pointers); asynchronous on `stream`."""
    ctx = ctx or default_context()
    _check(_lib().icp4r_vgicp_align_batch_device(ctx.handle, C.byref(batch), C.byref(params),
                                                 C.c_void_p(results_ptr), C.c_void_p(stream) if stream else None),
           "icp4r_vgicp_align_batch_device")


def voxel_map(cloud, resolution: float = 1.0, cov=None, k: int = 20, regularization: int = _gicp.REG_PLANE,
              cap: int | None = None, ctx: Context | None = None):
    """fast_gicp's GaussianVoxelMap of one cloud: (coords (V, 3) int32 in lexicographic order, num_points
    (V,) int32, mean (V, 3), cov (V, 3, 3)).  cov: the points' (N, 3, 3) covariances, or None for the
    k-NN ones.  cap: room for that many voxels (default: one per point); more raise ICP4R_E_INVALID."""
    ctx = ctx or default_context()
    c, n, cs = _cloud(cloud)
    cap = n if cap is None else int(cap)
    cin = None if cov is None else np.ascontiguousarray(np.asarray(cov, np.float64).reshape(n, 9))
    room = max(cap, 1)
    coords = np.zeros((room, 3), np.int32)
    num = np.zeros(room, np.int32)
    mean = np.zeros((room, 3), np.float64)
    vcov = np.zeros((room, 3, 3), np.float64)
    nv = C.c_int32(0)
    _check(_lib().icp4r_vgicp_voxel_map(ctx.handle, _ptr(c), n, cs, _ptr(cin) if cin is not None else None, k,
                                        regularization, float(resolution), cap, _ptr(coords), _ptr(num), _ptr(mean),
                                        _ptr(vcov), C.byref(nv)), "icp4r_vgicp_voxel_map")
    v = nv.value
    return coords[:v], num[:v], mean[:v], vcov[:v]


class FastVGICP(_gicp.FastGICPSingleThread):
    """fast_gicp::FastVGICP<PointXYZI, PointXYZI>: FastGICP's surface plus the voxel map's settings."""

    def __init__(self, context: Context | None = None):
        super().__init__(context)
        self._vp = default_params()

    def setResolution(self, resolution: float):
        self._vp.voxel_resolution = float(resolution)

    def setNeighborSearchMethod(self, method: int):
        self._vp.neighbor_search = int(method)

    def setVoxelAccumulationMode(self, mode: int):
        self._vp.voxel_accumulation = int(mode)

    def params(self) -> VgicpParams:
        self._vp.gicp = self._p
        return self._vp

    def _align_call(self, guess):
        return align(self._src, self._tgt, self.params(), guess=guess, want_aligned=True, ctx=self._ctx)
