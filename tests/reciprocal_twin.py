"""numpy twin of PCL 1.8.1 ICP with setUseReciprocalCorrespondences — TEST INFRASTRUCTURE.

The loop of tests/golden/numpy_twin.py (whose f32 path tests/test_oracle.py holds bit-equal to the C
oracle) with determineReciprocalCorrespondences in the place of determineCorrespondences
(correspondence_estimation.hpp): per iteration, with X the moved source,

  1. m = exact NN of X_i in the target, d2_i its distance (FLANN L2_Simple, float, ties to the lowest
     index); skip i if d2_i > max_d2;
  2. j = exact NN of t_m in X under the same rule; skip i if that distance is > max_d2 or j != i;
  3. the list is the survivors in source order, each with (i, m, d2_i).

Umeyama, the |C| < 3 failure, the MSE and n_correspondences run over that list; the fitness score is
not reciprocal.  reciprocal=False states numpy_twin's own loop (the tests assert equal bits).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from numpy_twin import (F32, _seq_sum_f64, l2_simple_all, mat4_mul_f32, nearest,  # noqa: E402
                        pcl_converged_transform, transform, umeyama_f32, umeyama_f64)

DBL_MAX = float(np.finfo(np.float64).max)
PCL_MAX_DIST = float(np.sqrt(np.finfo(np.float64).max))


def reciprocal_keep(X, tgt, idx, d2, max_d2):
    """The direct definition: the mask of the correspondences (i, idx[i], d2[i]) PCL keeps."""
    n = len(X)
    ridx, rd2 = nearest(tgt, X)  # the NN of every target in the moved source
    return ((d2.astype(np.float64) <= max_d2) & (rd2[idx].astype(np.float64) <= max_d2)
            & (ridx[idx] == np.arange(n)))


def _key(d2, i):
    return (np.asarray(d2, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(i, np.uint64)


def reciprocal_keep_by_key(X, tgt, idx, d2, max_d2):
    """The equivalent form: i is kept iff d2_i <= max_d2 and no source j has
    (d2(X_j, t_m), j) < (d2_i, i) in the u64 key order ((float bits of d2) << 32 | index)."""
    n = len(X)
    keep = d2.astype(np.float64) <= max_d2
    mine = _key(d2, np.arange(n))
    for i in np.nonzero(keep)[0]:
        D = l2_simple_all(tgt[idx[i]:idx[i] + 1], X)[0]
        keep[i] = _key(D, np.arange(n)).min() == mine[i]
    return keep


def huber_w(d2, delta):
    """oracle/icp_oracle.c huber_w: 1 inside delta, delta / r outside (double)."""
    r = np.sqrt(np.asarray(d2, np.float64))
    with np.errstate(divide="ignore"):
        return np.where(r <= delta, 1.0, delta / r)


def umeyama_f64_weighted(s, d, w):
    """oracle/icp_oracle.c umeyama_f64: raw weighted moments in double, mu = sum(w x) / sum(w),
    sigma = sum(w d s^T) / sum(w) - mu_d mu_s^T, Eigen's reflection rule, cast to Matrix4f."""
    s = s.astype(np.float64)
    d = d.astype(np.float64)
    sw = w.sum()
    ms, md = (w[:, None] * s).sum(0) / sw, (w[:, None] * d).sum(0) / sw
    sigma = (w[:, None] * d).T @ s / sw - np.outer(md, ms)
    U, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = U @ np.diag(S) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = md - R @ ms
    return T.astype(F32)


def icp(src, tgt, max_iterations=10, max_correspondence_distance=PCL_MAX_DIST, mse_threshold_absolute=1e-12,
        numerics="f32", huber_delta=np.inf, reciprocal=True, check_forms=False):
    """Returns dict(T, iterations, converged, state, status, fitness, n_correspondences, ncorr (per
    iteration, the failing one included), rejected (per iteration: candidates within max_d2 that the
    reciprocal rule dropped), aligned (n, 3)).  numerics "f32": PCL's float path; "f64": the Umeyama
    solve in double, with the Huber weights of huber_delta when finite (F64 only)."""
    assert numerics in ("f32", "f64") and (numerics == "f64" or not np.isfinite(huber_delta))
    src = np.asarray(src, F32)[:, :3]
    tgt = np.asarray(tgt, F32)[:, :3]
    X = src.copy()
    final = np.eye(4, dtype=F32)
    prev_mse = DBL_MAX
    max_d2 = max_correspondence_distance * max_correspondence_distance
    it, converged, state, status = 0, False, 0, 0
    ncorr, rejected = [], []
    while True:
        idx, d2 = nearest(X, tgt)
        near = d2.astype(np.float64) <= max_d2
        keep = reciprocal_keep(X, tgt, idx, d2, max_d2) if reciprocal else near
        if check_forms and reciprocal:
            assert (keep == reciprocal_keep_by_key(X, tgt, idx, d2, max_d2)).all()
        nk = int(keep.sum())
        ncorr.append(nk)
        rejected.append(int(near.sum()) - nk)
        if nk < 3:
            converged, state, status = False, 5, -3
            break
        s, d = X[keep], tgt[idx[keep]]
        if numerics == "f32":
            Tinc = umeyama_f32(s, d)[0]
        elif np.isfinite(huber_delta):
            Tinc = umeyama_f64_weighted(s, d, huber_w(d2[keep], huber_delta))
        else:
            Tinc = umeyama_f64(s, d)[0]
        X = transform(Tinc, X)
        final = mat4_mul_f32(Tinc, final)
        it += 1
        mse = _seq_sum_f64(d2[keep]) / nk
        if it >= max_iterations:
            converged, state = True, 1
            break
        cos_a, tsq = pcl_converged_transform(Tinc)
        if cos_a >= 1.0 and tsq <= 0.0:
            converged, state = True, 2
            break
        if abs(mse - prev_mse) < mse_threshold_absolute:
            converged, state = True, 3
            break
        prev_mse = mse
    Y = transform(final, src)
    _, fd = nearest(Y, tgt)
    fitness = _seq_sum_f64(fd) / len(fd) if len(fd) else DBL_MAX
    return {"T": final, "iterations": it, "converged": converged, "state": state, "status": status,
            "fitness": fitness, "n_correspondences": ncorr[-1], "ncorr": ncorr, "rejected": rejected,
            "aligned": Y}
