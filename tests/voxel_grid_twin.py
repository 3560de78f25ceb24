"""The voxel-grid contract (include/icp4r/icp4r_voxel.h: PCL 1.8.1 VoxelGrid::applyFilter with the
stable member order) in numpy float32, one voxel after the other.  Independent of the library: the
GPU tests compare whole arrays with it, bit for bit; tests/cpp/voxel_host_check.cpp is the second
restatement (C++, x86-64 SSE)."""
import numpy as np

F = np.float32
INT32_MAX = 2**31 - 1


class GridOverflow(Exception):
    """PCL: "Leaf size is too small for the input dataset" (and the documented deviations)."""


def as_xyzi(cloud):
    """(N, >=3) -> (N, 4) float32; a 12-byte point has intensity 0, floats past the fourth are ignored."""
    a = np.asarray(cloud, F)
    out = np.zeros((len(a), 4), F)
    k = min(a.shape[1], 4) if a.ndim == 2 else 0
    out[:, :k] = a[:, :k]
    return out


def grid(pts, leaf):
    """-> None (no participating point) or (inv, min_b, div, take); raises GridOverflow."""
    leaf = np.broadcast_to(np.asarray(leaf, F).reshape(-1), (3,))
    assert np.isfinite(leaf).all() and (leaf > 0).all()
    inv = F(1.0) / leaf  # float32 division, correctly rounded
    take = np.isfinite(pts[:, :3]).all(axis=1)
    if not take.any():
        return None
    min_p, max_p = pts[take, :3].min(axis=0), pts[take, :3].max(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        ext = (max_p - min_p) * inv            # float32
        lo, hi = np.floor(min_p * inv), np.floor(max_p * inv)
    if not (ext < F(2**31)).all():             # d[k] = (int64)ext + 1 must lie in [1, 2^31]
        raise GridOverflow("d")
    d = [int(e) + 1 for e in ext]
    if d[0] * d[1] * d[2] > INT32_MAX:         # Python integers: no wrap
        raise GridOverflow("d0 d1 d2")
    if not ((lo >= F(-2**31)).all() and (hi < F(2**31)).all()):
        raise GridOverflow("floorf(p * inv) is no int")
    min_b = [int(v) for v in lo]
    div = [int(h) - b + 1 for h, b in zip(hi, min_b)]
    if max(div) > 2**24 or div[0] * div[1] * div[2] > INT32_MAX:
        raise GridOverflow("div")
    return inv, min_b, div, take


def leaf_index(pts, inv, min_b, div):
    """idx of every row of pts (all finite)."""
    ijk = (np.floor(pts[:, :3] * inv) - np.asarray(min_b, F)).astype(np.int64)  # float32 up to the cast
    return ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]


def voxel_filter(cloud, leaf, downsample_all_data=True, min_points_per_voxel=0):
    """-> (K, 4) float32 centroids in ascending leaf index; raises GridOverflow."""
    pts = as_xyzi(cloud)
    g = grid(pts, leaf)
    if g is None:
        return np.zeros((0, 4), F)
    inv, min_b, div, take = g
    rows = np.flatnonzero(take)
    idx = leaf_index(pts[rows], inv, min_b, div)
    assert idx.min() >= 0 and idx.max() <= INT32_MAX - 1
    order = np.argsort(idx, kind="stable")     # members of a voxel stay in ascending input index
    sidx = idx[order]
    starts = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]])
    ends = np.r_[starts[1:], len(sidx)]
    out = []
    zero = np.zeros((1, 4), F)
    for s, e in zip(starts, ends):
        m = int(e - s)
        if m < min_points_per_voxel:
            continue
        members = pts[rows[order[s:e]]]
        # s = +0.0f; s += value, member by member: a float32 cumulative sum is that chain
        tot = np.cumsum(np.concatenate([zero, members]), axis=0, dtype=F)[-1]
        c = tot / F(m)
        if not downsample_all_data:
            c[3] = F(0.0)
        out.append(c)
    return np.array(out, F).reshape(-1, 4)


# ---- seeded test clouds (shared by the CPU and GPU tests)
def radar_cloud(n, seed):
    """A radar-shaped cloud: a flat scatter out to about 80 m with clusters, intensities in [0, 40)."""
    r = np.random.default_rng(seed)
    rng = r.uniform(1.0, 80.0, n)
    az = r.uniform(-np.pi / 3, np.pi / 3, n)
    xyz = np.stack([rng * np.cos(az), rng * np.sin(az), r.normal(0.0, 1.5, n)], axis=1)
    centres = r.integers(0, n, max(n // 8, 1))
    pick = r.random(n) < 0.5
    xyz[pick] = xyz[centres[r.integers(0, len(centres), pick.sum())]] + r.normal(0.0, 0.2, (pick.sum(), 3))
    return np.concatenate([xyz, r.uniform(0.0, 40.0, (n, 1))], axis=1).astype(F)


def crowded_cloud(sites=50, copies=40, seed=7):
    """`sites` spots with `copies` jittered points each, interleaved: voxels of many members whose
    centroid bits depend on the member order."""
    r = np.random.default_rng(seed)
    c = r.uniform(-30.0, 30.0, (sites, 3)) * np.array([1.0, 1.0, 0.1])
    c = (np.floor(c / 0.5) + 0.5) * 0.5        # the centre of a 0.5 m cell: the jitter stays inside
    xyz = c[None, :, :] + r.uniform(-0.2, 0.2, (copies, sites, 3))
    inten = r.uniform(0.0, 40.0, (copies, sites, 1))
    return np.concatenate([xyz, inten], axis=2).reshape(-1, 4).astype(F)
