"""Shared test helpers (pose error metrics, fixture loading)."""
from __future__ import annotations

import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star parity bar: <= 1e-4 m translation, <= 1e-4 rad rotation on identical inputs
TOL_T = 1e-4
TOL_R = 1e-4


def rot_angle(R1: np.ndarray, R2: np.ndarray) -> float:
    """Angle (rad) of R1ᵀR2, accurate for small angles (atan2 of the skew part)."""
    M = np.asarray(R1, np.float64).T @ np.asarray(R2, np.float64)
    v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.arctan2(np.linalg.norm(v) / 2.0, (np.trace(M) - 1.0) / 2.0))


def pose_err(T1, T2) -> tuple[float, float]:
    T1 = np.asarray(T1, np.float64)
    T2 = np.asarray(T2, np.float64)
    return float(np.abs(T1[:3, 3] - T2[:3, 3]).max()), rot_angle(T1[:3, :3], T2[:3, :3])


# ---------------------------------------------------------------------------------------------------
# Map store: random maps, points at a chosen heading, and the sector-edge filter that lets the map
# tests demand array equality with the oracle (tests/test_map_exact.py, tests/test_map.py).

EDGE_TOL_DEG = 1e-3     # float asin / heading error on either side of a sector edge is ~1e-5 deg
EDGE_MAX_SHARE = 1e-4   # the filter may remove at most this share of a map per query

# The four centre / heading pairs of the map tests.  Their sector edges (heading +- 60, and the
# dh > 300 edge) lie away from calc_heading = +-90, where asinf(r -> 1) is ill-conditioned
# (sqrt(2 ulp) ~ 0.02 deg) and a 1e-3 deg band would not cover the float error.
MAP_QUERIES = (([0, 0, 0], 0.0), ([10.5, -4.0, 1.0], 75.0), ([0, 0, 0], 179.5), ([-30, 20, 0], -90.0))


def random_map(rng, n, extent=150.0):
    """n uniform points in a flat box (z scaled by 0.1), random intensities."""
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    pts[:, 2] *= 0.1
    pts[:, 3] = rng.uniform(0, 50, n).astype(np.float32)
    return pts


def point_at(radius, h_deg, z=0.0):
    """A point at `radius` with calc_heading == h (0 along +y, +90 along -x) around the origin."""
    a = np.deg2rad(h_deg)
    return [-radius * np.sin(a), radius * np.cos(a), z, 1.0]


def heading_f64(pts, center) -> np.ndarray:
    """oracle_calc_heading's formula, wrap included, in float64 on the float32 inputs."""
    c = np.asarray(center, np.float32).astype(np.float64).reshape(-1)[:3]
    d = np.asarray(pts, np.float32)[:, :3].astype(np.float64) - c
    with np.errstate(invalid="ignore", divide="ignore"):
        r = d[:, 0] / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        a = np.arcsin(np.clip(r, -1.0, 1.0))  # NaN (the centre itself) stays NaN
        h = np.where(d[:, 1] < 0, 180.0 + a * 180.0 / np.pi, -a * 180.0 / np.pi)
        h = np.where((h > 180.0) & (h < 360.0), h - 360.0, h)
    return h


def sector_dh_f64(pts, center, heading) -> np.ndarray:
    return np.abs(heading_f64(pts, center) - float(np.float32(heading)))


def sector_keep_f64(pts, center, radius, heading) -> np.ndarray:
    """Search_by_sector's keep test with the heading in float64; the radius test stays the float32
    unfused ((dx*dx + dy*dy) + dz*dz) <= r*r of calc_dist, which needs no tolerance."""
    c = np.asarray(center, np.float32).reshape(-1)[:3]
    d = np.asarray(pts, np.float32)[:, :3] - c
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r = np.float32(radius)
    with np.errstate(invalid="ignore"):
        dh = sector_dh_f64(pts, center, heading)
        return ((d2 <= r * r) & (dh < 60.0)) | (dh > 300.0)


def sector_edge_filter(pts, queries):
    """Remove from the input map every point whose |dh| lies within EDGE_TOL_DEG of 60 or 300 for
    any of `queries` ((centre, heading) pairs): what is left has an unambiguous oracle answer, so
    device and oracle must agree exactly.  Asserts that each query removes at most EDGE_MAX_SHARE of
    the map.  Returns (filtered points, [removed count per query])."""
    pts = np.asarray(pts, np.float32)
    drop = np.zeros(len(pts), bool)
    removed = []
    for c, heading in queries:
        with np.errstate(invalid="ignore"):
            dh = sector_dh_f64(pts, c, heading)
            e = (np.abs(dh - 60.0) < EDGE_TOL_DEG) | (np.abs(dh - 300.0) < EDGE_TOL_DEG)
        assert e.sum() <= EDGE_MAX_SHARE * len(pts), (int(e.sum()), len(pts), c, heading)
        removed.append(int(e.sum()))
        drop |= e
    return pts[~drop], removed


def filtered_map(rng, n, queries, extent=150.0, ncols=4):
    """Exactly n random points that survive the edge filter of every query, the point's index in the
    intensity (exact below 2**24): a comparison of whole rows then sees order and multiplicity.
    The filter runs on a pool of at least 30 000 candidates (about 2e-5 of random points lie in the
    edge bands, so on a small map one removed point would already exceed the 1e-4 cap); the map is the
    pool's first n survivors.  Returns (points (n, ncols), [removed count per query])."""
    raw = random_map(rng, max(n + 64 + n // 2000, 30_000), extent)
    kept, removed = sector_edge_filter(raw, queries)
    assert len(kept) >= n
    out = np.zeros((n, ncols), np.float32)
    out[:, :3] = kept[:n, :3]
    if ncols > 3:
        out[:, 3] = np.arange(n, dtype=np.float32)
    if ncols > 4:
        out[:, 4:] = rng.uniform(-1, 1, (n, ncols - 4)).astype(np.float32)  # ignored by pack_host
    return out, removed


def load_case_clouds(case: dict):
    from icp4r import synth

    src = synth.records_to_xyzi(synth.read_bin(os.path.join(GOLDEN_DIR, case["src_bin"])))
    tgt = synth.records_to_xyzi(synth.read_bin(os.path.join(GOLDEN_DIR, case["tgt_bin"])))
    return src, tgt
