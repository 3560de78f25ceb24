"""The incremental voxel grid's contract (include/icp4r/icp4r_voxel_acc.h) in numpy float32: a
dictionary per absolute cell holding the four partial sums and the member count, the accumulated
bounding box for the overflow verdict, and the range rule.  Independent of the library and of
tests/voxel_grid_twin.py's sort-based filter, which it must equal bit for bit after every add."""
import numpy as np

from voxel_grid_twin import GridOverflow, INT32_MAX, as_xyzi

F = np.float32
RANGE = 2**20  # axis offsets from the origin lie in [-RANGE, RANGE)


class RangeError(Exception):
    """The add would leave the range of +-2^20 cells around the origin; the accumulator is as it was."""


class VoxelAccumulatorTwin:
    def __init__(self, leaf, downsample_all_data=True, min_points_per_voxel=0):
        leaf = np.broadcast_to(np.asarray(leaf, F).reshape(-1), (3,))
        assert np.isfinite(leaf).all() and (leaf > 0).all()
        self.inv = F(1.0) / leaf
        self.all_data = bool(downsample_all_data)
        self.min_pts = int(min_points_per_voxel)
        self.clear()

    def clear(self):
        self.cells = {}      # (cz, cy, cx) -> [sums (4,) float32, count]
        self.min_p = None    # the accumulated box of the participating points
        self.max_p = None
        self.origin = None
        self.points = 0

    def add(self, cloud):
        pts = as_xyzi(cloud)
        take = np.isfinite(pts[:, :3]).all(axis=1)
        if not take.any():
            self.points += len(pts)
            return
        p = pts[take]
        lo, hi = p[:, :3].min(axis=0), p[:, :3].max(axis=0)
        with np.errstate(over="ignore", invalid="ignore"):
            flo, fhi = np.floor(lo * self.inv), np.floor(hi * self.inv)
        if not ((flo >= F(-2**31)).all() and (fhi < F(2**31)).all()):
            raise RangeError("a cell is no int")
        minc, maxc = [int(v) for v in flo], [int(v) for v in fhi]
        org = self.origin if self.origin is not None else minc
        for k in range(3):
            if minc[k] - org[k] < -RANGE or maxc[k] - org[k] >= RANGE:
                raise RangeError(f"axis {k}")
        self.origin = org
        self.points += len(pts)
        self.min_p = lo if self.min_p is None else np.minimum(self.min_p, lo)
        self.max_p = hi if self.max_p is None else np.maximum(self.max_p, hi)
        c = np.floor(p[:, :3] * self.inv).astype(np.int64)  # float32 up to the cast
        for row, (cx, cy, cz) in zip(p, c.tolist()):
            e = self.cells.get((cz, cy, cx))
            if e is None:
                e = self.cells[(cz, cy, cx)] = [np.zeros(4, F), 0]  # the chain starts from +0.0f
            e[0] = e[0] + row                                        # float32, member by member
            e[1] += 1

    def overflow(self) -> bool:
        """The verdict of include/icp4r/icp4r_voxel.h from the accumulated box alone."""
        if self.min_p is None:
            return False
        with np.errstate(over="ignore", invalid="ignore"):
            ext = (self.max_p - self.min_p) * self.inv
            lo, hi = np.floor(self.min_p * self.inv), np.floor(self.max_p * self.inv)
        if not (ext < F(2**31)).all():
            return True
        d = [int(e) + 1 for e in ext]
        if d[0] * d[1] * d[2] > INT32_MAX:
            return True
        if not ((lo >= F(-2**31)).all() and (hi < F(2**31)).all()):
            return True
        div = [int(h) - int(l) + 1 for l, h in zip(lo, hi)]
        return max(div) > 2**24 or div[0] * div[1] * div[2] > INT32_MAX

    def size(self):
        return len(self.cells), self.points

    def filter(self):
        if self.overflow():
            raise GridOverflow("the accumulated box")
        out = []
        for key in sorted(self.cells):  # lexicographic (cz, cy, cx) = ascending leaf index
            s, m = self.cells[key]
            if m < self.min_pts:
                continue
            c = s / F(m)
            if not self.all_data:
                c[3] = F(0.0)
            out.append(c)
        return np.array(out, F).reshape(-1, 4)
