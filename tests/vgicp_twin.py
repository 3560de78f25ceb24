"""The voxelized GICP of include/icp4r/icp4r_vgicp.h restated in numpy (fast_gicp's FastVGICP; fast_gicp
itself is not available, so this twin and known answers pin the device code).

Plain on purpose: a dict of voxels, loops over voxels and offsets.  The point covariances are inputs (the
tests feed the device's or the oracle's), so only the order of the Gauss-Newton sums differs from the
device: the sums here are numpy's.

    voxel_map(points, covs, resolution)        -> VoxelMap (coords in lexicographic order, num, mean, cov)
    lm_align(linearize, error, guess, ...)     -> LsqRegistration's Levenberg-Marquardt loop
    align(src, tgt, cov_src, cov_tgt, ...)     -> the registration
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

DIRECT1, DIRECT7, DIRECT27 = 0, 1, 2
KEY_RANGE = 1 << 20  # cells -2^20 .. 2^20 - 1 per axis


def offsets(mode: int) -> list[tuple[int, int, int]]:
    if mode == DIRECT1:
        return [(0, 0, 0)]
    if mode == DIRECT7:
        return [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    if mode == DIRECT27:
        return [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    raise ValueError(f"neighbor_search {mode}")


def cells(points: np.ndarray, resolution: float) -> np.ndarray:
    """floor(double(p) / resolution) per axis, as float64 (the caller checks the range)."""
    return np.floor(np.asarray(points, np.float64) / np.float64(resolution))


@dataclass
class VoxelMap:
    coords: np.ndarray   # (V, 3) int32, lexicographic order
    num: np.ndarray      # (V,) int32
    mean: np.ndarray     # (V, 3) float64
    cov: np.ndarray      # (V, 3, 3) float64
    index: dict          # (cx, cy, cz) -> v


def _sym_from_upper(m: np.ndarray) -> np.ndarray:
    """The matrix whose upper triangle is m's, mirrored."""
    u = np.triu(m)
    return u + np.swapaxes(np.triu(m, 1), -1, -2)


def voxel_map(points, covs, resolution: float) -> VoxelMap:
    """num_points, mean = Σp / num and cov = ΣC / num per cell, both sums sequential in ascending point
    index starting from the first term.  Of a covariance the upper triangle is read."""
    p = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    C = _sym_from_upper(np.asarray(covs, np.float64).reshape(-1, 3, 3))
    c = cells(p, resolution)
    if len(p) and not np.all((c >= -KEY_RANGE) & (c < KEY_RANGE)):
        raise ValueError("a coordinate lies outside the key range")
    sums: dict = {}
    for i in range(len(p)):
        key = (int(c[i, 0]), int(c[i, 1]), int(c[i, 2]))
        if key not in sums:
            sums[key] = [1, p[i].copy(), C[i].copy()]
        else:
            s = sums[key]
            s[0] += 1
            s[1] = s[1] + p[i]
            s[2] = s[2] + C[i]
    keys = sorted(sums)
    V = len(keys)
    out = VoxelMap(np.zeros((V, 3), np.int32), np.zeros(V, np.int32), np.zeros((V, 3)), np.zeros((V, 3, 3)), {})
    for v, key in enumerate(keys):
        n, sp, sc = sums[key]
        out.coords[v] = key
        out.num[v] = n
        out.mean[v] = sp / np.float64(n)
        out.cov[v] = sc / np.float64(n)
        out.index[key] = v
    return out


# ------------------------------------------------------------------------------------ LsqRegistration
def so3_exp(w: np.ndarray) -> np.ndarray:
    """fast_gicp's so3_exp then Eigen's Quaternion::toRotationMatrix."""
    w = np.asarray(w, np.float64)
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 < 1e-10:
        th4 = th2 * th2
        imag = 0.5 - 1.0 / 48.0 * th2 + 1.0 / 3840.0 * th4
        real = 1.0 - 1.0 / 8.0 * th2 + 1.0 / 384.0 * th4
    else:
        th = np.sqrt(th2)
        imag = np.sin(0.5 * th) / th
        real = np.cos(0.5 * th)
    qw, qx, qy, qz = real, imag * w[0], imag * w[1], imag * w[2]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def ldlt_solve(A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Eigen's LDLT solve without pivoting (a zero pivot leaves its column undivided and solves to 0)."""
    n = len(b)
    L = np.eye(n)
    D = np.zeros(n)
    for j in range(n):
        D[j] = A[j, j] - np.sum(L[j, :j] * L[j, :j] * D[:j])
        for i in range(j + 1, n):
            t = A[i, j] - np.sum(L[i, :j] * L[j, :j] * D[:j])
            L[i, j] = t / D[j] if D[j] != 0.0 else t
    y = np.zeros(n)
    for i in range(n):
        y[i] = b[i] - np.sum(L[i, :i] * y[:i])
    tiny = np.finfo(np.float64).tiny
    y = np.array([y[i] / D[i] if abs(D[i]) > tiny else 0.0 for i in range(n)])
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - np.sum(L[i + 1:, i] * x[i + 1:])
    return x


def _is_converged(dR, dt, rot_eps, trans_eps) -> bool:
    m = max(np.max(np.abs(dR - np.eye(3))) / rot_eps, np.max(np.abs(dt)) / trans_eps)
    return bool(m < 1.0)


def lm_align(linearize, error, guess=None, max_iterations=64, rotation_epsilon=2e-3, transformation_epsilon=5e-4,
             lm_max_iterations=10, lm_init_lambda_factor=1e-9) -> dict:
    """LsqRegistration::align with step_lm.  linearize(R, t) -> (H 6x6, g 6, y, n_correspondences, kept);
    error(R, t, kept) -> y at another pose over the kept correspondences.
    -> T (4x4 float64: x0), iterations (the index of the last iteration), converged, lm_failed, n_valid;
    a log beside them: trials (the trials evaluated per iteration) and stops (per iteration 1 accepted,
    2 converged on a rejected trial, 0 every trial rejected)."""
    G = np.eye(4) if guess is None else np.asarray(guess, np.float32).astype(np.float64)
    R, t = G[:3, :3].copy(), G[:3, 3].copy()
    lam = -1.0
    out = {"iterations": 0, "converged": False, "lm_failed": False, "n_valid": 0, "trials": [], "stops": []}
    with np.errstate(all="ignore"):
        for it in range(max_iterations):
            H, g, y0, n, kept = linearize(R, t)
            if lam < 0.0:
                lam = lm_init_lambda_factor * np.max(np.abs(np.diag(H)))
            nu = 2.0
            stop = 0
            dR, dt = np.eye(3), np.zeros(3)
            ntrials = 0
            for _ in range(lm_max_iterations):
                ntrials += 1
                d = ldlt_solve(H + lam * np.eye(6), -g)
                dR, dt = so3_exp(d[:3]), d[3:].copy()
                Rn, tn = dR @ R, dR @ t + dt
                yi = error(Rn, tn, kept)
                rho = np.float64(y0 - yi) / np.float64(np.dot(d, lam * d - g))
                if rho < 0:
                    if _is_converged(dR, dt, rotation_epsilon, transformation_epsilon):
                        stop = 2
                        break
                    lam = nu * lam
                    nu = 2 * nu
                else:
                    R, t = Rn, tn
                    lam = lam * np.fmax(1.0 / 3.0, 1 - (2 * rho - 1) ** 3)
                    stop = 1
                    break
            out["iterations"] = it
            out["n_valid"] = int(n)
            out["trials"].append(ntrials)
            out["stops"].append(stop)
            if not stop:
                out["lm_failed"] = True
                break
            if _is_converged(dR, dt, rotation_epsilon, transformation_epsilon):
                out["converged"] = True
                break
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    out["T"] = T
    return out


# ------------------------------------------------------------------------------------ the registration
def transform(R, t, a):
    """Ta = ((R[r][0] a0 + R[r][1] a1) + R[r][2] a2) + t[r] for every point of a (n, 3) float64."""
    return np.stack([((R[r, 0] * a[:, 0] + R[r, 1] * a[:, 1]) + R[r, 2] * a[:, 2]) + t[r] for r in range(3)], 1)


def inv3(m: np.ndarray) -> np.ndarray:
    """Eigen's cofactor inverse of (..., 3, 3)."""
    m = np.asarray(m, np.float64)
    a = [m[..., i // 3, i % 3] for i in range(9)]
    c0 = a[4] * a[8] - a[5] * a[7]
    c1 = a[7] * a[2] - a[8] * a[1]
    c2 = a[1] * a[5] - a[2] * a[4]
    idet = 1.0 / (c0 * a[0] + c1 * a[3] + c2 * a[6])
    r = [c0 * idet, c1 * idet, c2 * idet,
         (a[5] * a[6] - a[3] * a[8]) * idet, (a[8] * a[0] - a[6] * a[2]) * idet, (a[2] * a[3] - a[0] * a[5]) * idet,
         (a[3] * a[7] - a[4] * a[6]) * idet, (a[6] * a[1] - a[7] * a[0]) * idet, (a[0] * a[4] - a[1] * a[3]) * idet]
    return np.stack(r, -1).reshape(m.shape)


def skew(v: np.ndarray) -> np.ndarray:
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def correspondences(vm: VoxelMap, ta: np.ndarray, resolution: float, mode: int):
    """(point, voxel) for every point of ta and every offset, in (point, offset) order."""
    c = cells(ta, resolution)
    pi, vi = [], []
    offs = offsets(mode)
    for i in range(len(ta)):
        if not np.all((c[i] >= -KEY_RANGE) & (c[i] < KEY_RANGE)):
            continue
        base = (int(c[i, 0]), int(c[i, 1]), int(c[i, 2]))
        for d in offs:
            v = vm.index.get((base[0] + d[0], base[1] + d[1], base[2] + d[2]))
            if v is not None:
                pi.append(i)
                vi.append(v)
    return np.array(pi, np.int64), np.array(vi, np.int64)


def align(src, tgt, cov_src, cov_tgt, resolution=1.0, mode=DIRECT1, guess=None, **lm) -> dict:
    """FastVGICP::align.  cov_src / cov_tgt: the clouds' (regularised) point covariances."""
    a = np.asarray(src, np.float32)[:, :3].astype(np.float64)
    CA = _sym_from_upper(np.asarray(cov_src, np.float64).reshape(-1, 3, 3))
    vm = voxel_map(tgt, cov_tgt, resolution)

    def weights(R, pi, vi):
        Mi = inv3(vm.cov[vi] + R @ CA[pi] @ R.T)
        return np.sqrt(vm.num[vi].astype(np.float64))[:, None, None] * _sym_from_upper(Mi)

    def linearize(R, t):
        ta = transform(R, t, a)
        pi, vi = correspondences(vm, ta, resolution, mode)
        if len(pi) == 0:
            return np.zeros((6, 6)), np.zeros(6), 0.0, 0, (pi, vi, None)
        W = weights(R, pi, vi)
        e = vm.mean[vi] - ta[pi]
        J = np.concatenate([skew(ta[pi]), np.broadcast_to(-np.eye(3), (len(pi), 3, 3))], 2)
        H = np.einsum("nki,nkl,nlj->ij", J, W, J)
        g = np.einsum("nki,nkl,nl->i", J, W, e)
        y = np.einsum("nk,nkl,nl->", e, W, e)
        return H, g, float(y), len(pi), (pi, vi, W)

    def error(R, t, kept):
        pi, vi, W = kept
        if len(pi) == 0:
            return 0.0
        e = vm.mean[vi] - transform(R, t, a)[pi]
        return float(np.einsum("nk,nkl,nl->", e, W, e))

    r = lm_align(linearize, error, guess, **lm)
    r["map"] = vm
    return r


def fitness(src, tgt, T) -> float:
    """Registration::getFitnessScore(): the mean exact-NN d² (float L2_Simple) of float(T) * src in tgt."""
    s, g = np.asarray(src, np.float32)[:, :3], np.asarray(tgt, np.float32)[:, :3]
    Tf = np.asarray(T).astype(np.float32)
    x = np.empty_like(s)
    for r in range(3):
        v = Tf[r, 0] * s[:, 0]
        v = v + Tf[r, 1] * s[:, 1]
        v = v + Tf[r, 2] * s[:, 2]
        x[:, r] = v + Tf[r, 3]
    best = np.full(len(s), np.inf, np.float32)
    for j0 in range(0, len(g), 512):
        d = x[:, None, :] - g[None, j0:j0 + 512, :]
        d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        best = np.minimum(best, d2.min(1))
    return float(np.mean(best.astype(np.float64)))
