"""The 3D Doppler ego-velocity estimator as include/icp4r/icp4r_reve.h restates it, in numpy / Python:
the spec in executable form.  Every operation is an IEEE double + - * / sqrt in the header's order (numpy
float64 scalars and elementwise array arithmetic: no fused multiply-add, no reordering), so steps 1, 3
and 4 — masks, counts, the winning hypothesis — are what a conforming device computes bit for bit; the
refit sums run in index order (`reverse=True`: in reversed order, to measure what the order is worth).
"""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
JACOBI_SWEEPS = 8
F = np.float64

# config_init, src/radar_odometry.cpp:576-610 of the reference
DEFAULTS = dict(
    min_dist=0.25, max_dist=100.0, min_db=0.0, elevation_thresh_deg=60.0, azimuth_thresh_deg=60.0, filter_min_z=-3.0,
    filter_max_z=3.0, doppler_velocity_correction_factor=1.0, thresh_zero_velocity=0.05,
    allowed_outlier_percentage=0.25, sigma_zero_velocity_x=0.025, sigma_zero_velocity_y=0.025,
    sigma_zero_velocity_z=0.025, sigma_offset_radar_x=0.05, sigma_offset_radar_y=0.025, sigma_offset_radar_z=0.05,
    max_sigma_x=0.2, max_sigma_y=0.2, max_sigma_z=0.2, max_r_cond=1000.0, use_cholesky_instead_of_bdcsvd=1,
    use_ransac=1, outlier_prob=0.4, success_prob=0.9999, N_ransac_points=3, inlier_thresh=0.15, use_odr=1,
    sigma_v_d=0.125, min_speed_odr=4.0, model_noise_offset_deg=2.0, model_noise_scale_deg=10.0,
    seed=0x4E7E5EED, use_z_filter=0)


def params(**kw) -> dict:
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed: int, k: int, n_valid: int) -> tuple[int, int, int]:
    """The first three steps of a Fisher-Yates shuffle of range(n_valid), literally (the array as a dict
    of the positions that moved)."""
    a = {}
    out = []
    for i in range(3):
        j = i + splitmix64((seed + 3 * k + i) & M64) % (n_valid - i)
        ai, aj = a.get(i, i), a.get(j, j)
        a[i], a[j] = aj, ai
        out.append(a[i])
    return tuple(out)


def ransac_iterations(p: dict) -> int:
    return int(math.log(1.0 - p["success_prob"]) / math.log(1.0 - math.pow(1.0 - p["outlier_prob"], 3)))


def _rotate(app, aqq, apq, arp, arq):
    if not apq != 0.0:
        return app, aqq, apq, arp, arq
    theta = (aqq - app) / (F(2.0) * apq)
    t = F(1.0) / (np.abs(theta) + np.sqrt(theta * theta + F(1.0)))
    if theta < 0.0:
        t = -t
    c = F(1.0) / np.sqrt(t * t + F(1.0))
    s = t * c
    tp = t * apq
    return app - tp, aqq + tp, F(0.0), c * arp - s * arq, s * arp + c * arq


def jacobi_cond(m) -> float:
    """lambda_max / lambda_min of [m0 m1 m2; m1 m3 m4; m2 m4 m5] by fixed-sweep cyclic Jacobi."""
    a00, a01, a02, a11, a12, a22 = (F(x) for x in m)
    for _ in range(JACOBI_SWEEPS):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02)
    hi = lo = a00
    if a11 > hi:
        hi = a11
    if a22 > hi:
        hi = a22
    if a11 < lo:
        lo = a11
    if a22 < lo:
        lo = a22
    return hi / lo


def solve3(m, g):
    """(R row-major, v): the cofactor inverse of the header and v_i = (R_i0 g_0 + R_i1 g_1) + R_i2 g_2."""
    M = [[F(m[0]), F(m[1]), F(m[2])], [F(m[1]), F(m[3]), F(m[4])], [F(m[2]), F(m[4]), F(m[5])]]
    c0 = M[1][1] * M[2][2] - M[1][2] * M[2][1]
    c1 = M[2][1] * M[0][2] - M[2][2] * M[0][1]
    c2 = M[0][1] * M[1][2] - M[0][2] * M[1][1]
    det = (c0 * M[0][0] + c1 * M[1][0]) + c2 * M[2][0]
    inv = F(1.0) / det
    R = [c0 * inv, c1 * inv, c2 * inv,
         (M[1][2] * M[2][0] - M[1][0] * M[2][2]) * inv,
         (M[2][2] * M[0][0] - M[2][0] * M[0][2]) * inv,
         (M[0][2] * M[1][0] - M[0][0] * M[1][2]) * inv,
         (M[1][0] * M[2][1] - M[1][1] * M[2][0]) * inv,
         (M[2][0] * M[0][1] - M[2][1] * M[0][0]) * inv,
         (M[0][0] * M[1][1] - M[0][1] * M[1][0]) * inv]
    g = [F(x) for x in g]
    v = [(R[3 * i] * g[0] + R[3 * i + 1] * g[1]) + R[3 * i + 2] * g[2] for i in range(3)]
    return R, v


def valid_mask(rec, p) -> np.ndarray:
    rec = np.asarray(rec, np.float32).reshape(-1, 5)
    x, y, z, inten, dop = (rec[:, k].astype(np.float64) for k in range(5))
    xy = x * x + y * y
    r = np.sqrt(xy + z * z)
    d = dop * F(p["doppler_velocity_correction_factor"])
    az = F(p["azimuth_thresh_deg"]) * F(math.pi / 180.0)
    el = F(p["elevation_thresh_deg"]) * F(math.pi / 180.0)
    ok = (r > p["min_dist"]) & (r < p["max_dist"]) & (inten > p["min_db"])
    ok &= np.abs(np.arctan2(y, x)) < az
    ok &= np.abs(np.arctan2(np.sqrt(xy), z) - F(math.pi) / F(2.0)) < el
    ok &= np.isfinite(dop) & np.isfinite(d)
    if p["use_z_filter"] == 1:
        ok &= (z > p["filter_min_z"]) & (z < p["filter_max_z"])
    return ok


def _sum(a, reverse):
    """Sequential float64 sum in index (or reversed) order."""
    t = F(0.0)
    for x in (a[::-1] if reverse else a):
        t = t + x
    return t


def estimate(rec, p: dict | None = None, seed: int | None = None, reverse: bool = False) -> dict:
    """One scan.  Returns v, sigma (float64[3]), mask (uint8[n]), n, n_valid, n_inliers, iterations,
    accepted, best, zero_velocity, success, and for the tests: conds (every hypothesis' cond), counts (its
    inliers, -1: rejected), refit_cond, refit_M (the 6 unique sums of the refit's HtH)."""
    p = params() if p is None else p
    seed = p["seed"] if seed is None else seed
    with np.errstate(all="ignore"):
        return _estimate(np.asarray(rec, np.float32).reshape(-1, 5), p, seed, reverse)


def _estimate(rec, p, seed, reverse):
    n = len(rec)
    out = dict(v=np.zeros(3), sigma=np.zeros(3), mask=np.zeros(n, np.uint8), n=n, n_valid=0, n_inliers=0, iterations=0,
               accepted=0, best=-1, zero_velocity=0, success=0, conds=[], counts=[], refit_cond=None, refit_M=None)
    ok = valid_mask(rec, p)
    idx = np.flatnonzero(ok)
    m = len(idx)
    out["n_valid"] = m
    if m < 3:
        return out
    x, y, z = (rec[idx, k].astype(np.float64) for k in range(3))
    r = np.sqrt((x * x + y * y) + z * z)
    hx, hy, hz = x / r, y / r, z / r
    d = rec[idx, 4].astype(np.float64) * F(p["doppler_velocity_correction_factor"])
    # 3. standstill
    a = np.sort(np.abs(d))
    nth = int(F(m) * (F(1.0) - F(p["allowed_outlier_percentage"])))
    nth = min(nth, m - 1)
    if a[nth] < p["thresh_zero_velocity"]:
        inl = np.abs(d) < p["thresh_zero_velocity"]
        out["mask"][idx[inl]] = 1
        out.update(sigma=np.array([p["sigma_zero_velocity_x"], p["sigma_zero_velocity_y"], p["sigma_zero_velocity_z"]]),
                   n_inliers=int(inl.sum()), zero_velocity=1, success=1)
        return out
    # 4. RANSAC
    yv = -d
    H = ransac_iterations(p)
    out["iterations"] = H
    best, best_cnt, best_inl = -1, 0, None
    for k in range(H):
        tri = draw(seed, k, m)
        t = [[hx[j] * hx[j], hx[j] * hy[j], hx[j] * hz[j], hy[j] * hy[j], hy[j] * hz[j], hz[j] * hz[j],
              hx[j] * yv[j], hy[j] * yv[j], hz[j] * yv[j]] for j in tri]
        s = [(t[0][q] + t[1][q]) + t[2][q] for q in range(9)]
        cond = jacobi_cond(s[:6])
        out["conds"].append(float(cond))
        if not np.abs(cond) < p["max_r_cond"]:
            out["counts"].append(-1)
            continue
        out["accepted"] += 1
        _, v = solve3(s[:6], s[6:])
        inl = np.abs(yv - ((hx * v[0] + hy * v[1]) + hz * v[2])) < p["inlier_thresh"]
        c = int(inl.sum())
        out["counts"].append(c)
        if c > best_cnt:
            best, best_cnt, best_inl = k, c, inl
    out["best"] = best
    if best < 0:
        return out
    out["n_inliers"] = best_cnt
    out["mask"][idx[best_inl]] = 1
    # 5. refit
    bx, by, bz, byv = hx[best_inl], hy[best_inl], hz[best_inl], yv[best_inl]
    s = [_sum(q, reverse) for q in (bx * bx, bx * by, bx * bz, by * by, by * bz, bz * bz, bx * byv, by * byv, bz * byv)]
    out["refit_M"] = [float(q) for q in s[:6]]
    cond = jacobi_cond(s[:6])
    out["refit_cond"] = float(cond)
    if not np.abs(cond) < p["max_r_cond"]:
        return out
    R, v = solve3(s[:6], s[6:])
    e = ((bx * v[0] + by * v[1]) + bz * v[2]) - byv
    ee = _sum(e * e, reverse)
    off = [p["sigma_offset_radar_x"], p["sigma_offset_radar_y"], p["sigma_offset_radar_z"]]
    mx = [p["max_sigma_x"], p["max_sigma_y"], p["max_sigma_z"]]
    sig = [np.sqrt((ee * R[4 * i]) / F(best_cnt - 3)) + F(off[i]) for i in range(3)]
    out["v"] = np.array([float(q) for q in v])
    out["sigma"] = np.array([float(q) for q in sig])
    out["success"] = int(all(bool(sig[i] < mx[i]) for i in range(3)))
    return out


def estimate_batch(rec, off, cnt, max_n, p: dict | None = None):
    """The batch entries' contract: scan s = rec[off[s] : off[s] + cnt[s]] with the seed p.seed + (s << 32);
    a scan with cnt < 0 or cnt > max_n is refused (None) and its records are not looked at.  Returns the
    per-scan results and the mask indexed like rec (untouched bytes stay 0xFF-free: the caller's)."""
    p = params() if p is None else p
    rec = np.asarray(rec, np.float32).reshape(-1, 5)
    res = []
    for s, (o, c) in enumerate(zip(off, cnt)):
        o, c = int(o), int(c)
        if c < 0 or c > max_n:
            res.append(None)
            continue
        res.append(estimate(rec[o:o + c], p, seed=(p["seed"] + (s << 32)) & M64))
    return res
