"""The incremental voxel grid on the GPU (include/icp4r/icp4r_voxel_acc.h).  The oracle is the full
filter's twin (tests/voxel_grid_twin.py) on the concatenation of everything added so far, compared as
whole arrays — count, order and bits, no tolerance — after every add; the final state is compared with
the library's own VoxelGrid.filter of the concatenation too."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import icp4r
import voxel_acc_twin as acc_twin
import voxel_grid_twin as twin
import voxel_tools as tools
from icp4r import mapstore, voxel
from test_voxel_acc import compile_acc_callsite, shifted
from voxel_tools import same_bits

pytestmark = pytest.mark.gpu
F = np.float32
B = 2048            # the merge kernel's state elements per workgroup (kAccMergeBlock)
INITIAL_CAP = 4096  # voxels of the first allocation
SMALL = 8192        # scans of at most this many points are sorted by one workgroup (kAccSmall)


def to_device(cloud):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(twin.as_xyzi(cloud), F)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()  # torch's copy runs on its stream
    return t


def device_filter(acc, stream=None):
    """filter_device -> (count, the whole output buffer)."""
    import torch

    dev = torch.device("cuda", 0)
    cap = max(acc.size()[0], 1)
    d_out = torch.full((cap + 4, 4), -7.5, dtype=torch.float32, device=dev)
    d_cnt = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    acc.filter_device(d_out.data_ptr(), d_cnt.data_ptr(), stream.cuda_stream if stream else None)
    torch.cuda.synchronize()
    return int(d_cnt.item()), d_out.cpu().numpy()


class Run:
    """An accumulator and the concatenation of what it was given."""

    def __init__(self, ctx, leaf=0.5, all_data=True, min_pts=0):
        self.ctx, self.leaf, self.all_data, self.min_pts = ctx, leaf, all_data, min_pts
        self.acc = voxel.VoxelAccumulator(leaf, all_data, min_pts, ctx=ctx)
        self.seen = np.zeros((0, 4), F)
        self.keep = []  # device tensors stay alive until the run ends

    def add(self, cloud, device=False, stream=None, check=True):
        if device:
            t = to_device(cloud)
            self.keep.append(t)
            self.acc.add_device(t.data_ptr(), len(cloud), stream.cuda_stream if stream else None)
        else:
            self.acc.add(cloud)
        self.seen = np.concatenate([self.seen, twin.as_xyzi(cloud)])
        return self.check() if check else None

    def want(self):
        return twin.voxel_filter(self.seen, self.leaf, self.all_data, self.min_pts)

    def check(self):
        import torch

        torch.cuda.synchronize()
        got, want = self.acc.filter(), self.want()
        assert got.shape == want.shape, (got.shape, want.shape)
        assert same_bits(got, want)
        return want

    def check_against_the_library(self):
        g = voxel.VoxelGrid(self.ctx)
        lf = np.broadcast_to(np.asarray(self.leaf, F).reshape(-1), (3,))
        g.setLeafSize(float(lf[0]), float(lf[1]), float(lf[2]))
        g.setDownsampleAllData(self.all_data)
        g.setMinimumPointsNumberPerVoxel(self.min_pts)
        assert same_bits(self.acc.filter(), g.filter(self.seen))

    def close(self):
        self.acc.close()


@pytest.fixture
def run(gpu_ctx):
    made = []

    def make(leaf=0.5, all_data=True, min_pts=0):
        made.append(Run(gpu_ctx, leaf, all_data, min_pts))
        return made[-1]

    yield make
    for r in made:
        r.close()


# ---- merges
@pytest.mark.parametrize("device", [False, True])
def test_six_radar_adds(run, device):
    """New cells before the first stored key, after the last and interleaved; a repeated scan (only
    existing cells); a scan of only new cells."""
    r = run()
    base = twin.radar_cloud(2000, seed=80)
    r.add(base, device)
    n0 = r.acc.size()[0]
    r.add(shifted(twin.radar_cloud(700, seed=81), dz=-30.0), device)    # all keys below the first stored one
    r.add(shifted(twin.radar_cloud(900, seed=82), dz=30.0), device)     # all above the last
    r.add(shifted(twin.radar_cloud(5000, seed=83), dx=3.0, dy=-2.0), device)  # interleaved, many shared cells
    n3 = r.acc.size()[0]
    r.add(base, device)                                                  # only existing cells
    assert r.acc.size() == (n3, 2000 + 700 + 900 + 5000 + 2000)
    r.add(shifted(twin.radar_cloud(1500, seed=84), dy=400.0), device)   # only new cells
    assert r.acc.size()[0] > n3 > n0
    r.check_against_the_library()


def line(cells):
    """One point per cell, the cells on a line along x (leaf 0.5): the state's order is the cells' order."""
    cells = np.asarray(cells, np.float64)
    c = np.zeros((len(cells), 4))
    c[:, 0] = cells * 0.5 + 0.25
    c[:, 1:3] = 0.25
    c[:, 3] = np.arange(len(cells)) % 37
    return c.astype(F)


@pytest.mark.parametrize("size", [B - 1, B, B + 1, 2 * B + 1])
@pytest.mark.parametrize("where", ["front", "boundary", "end", "all"])
def test_one_new_cell_into_a_state_of_block_size(run, size, where):
    """The stored cells are the even ones, so a new odd cell lands between any two of them."""
    r = run()
    r.add(line(2 * np.arange(size))[np.random.default_rng(size).permutation(size)], check=False)
    p = B if size > B else size - 1  # the new cell goes between positions p - 1 and p
    new = {"front": [-1], "boundary": [2 * p - 1], "end": [2 * size + 1], "all": [-1, 2 * p - 1, 2 * size + 1]}[where]
    want = r.add(line(new))
    assert len(want) == size + len(new) and r.acc.size()[0] == len(want)
    r.add(line([2 * p - 1, 2 * p - 2, 2 * p]), device=True)  # found runs next to the inserted one


# ---- chains across adds
@pytest.mark.parametrize("device", [False, True])
def test_crowded_cloud_over_three_adds(run, device):
    r = run()
    for part in np.array_split(twin.crowded_cloud(), 3):
        want = r.add(part, device)
    assert 40 <= len(want) <= 50
    r.check_against_the_library()


def test_one_voxel_growing_across_both_chain_forms(run):
    """1, 16, 17, 64, 65 and 9,000 members in successive adds: the one-lane walk and its limit, the wave's
    gather and its 64-member chunk, each continuing the stored sums."""
    r = run()
    g = np.random.default_rng(90)
    other = np.array([[3.3, 0.2, 0.2, 1.0]], F)  # a second voxel beside it
    for i, m in enumerate([1, 16, 17, 64, 65, 9000]):
        c = np.concatenate([g.uniform(0.01, 0.49, (m, 3)), g.uniform(0, 40, (m, 1))], axis=1).astype(F)
        want = r.add(np.concatenate([c, other]), device=bool(i & 1))
        assert len(want) == 2
    assert r.acc.size() == (2, 9163 + 6)
    r.check_against_the_library()


def test_negative_zero_first_member(run):
    r = run(1.0)
    want = r.add(np.array([[-0.0, 0.25, 0.25, -0.0]], F))
    assert want.view(np.uint32)[0, [0, 3]].tolist() == [0, 0]
    r.add(np.array([[-0.0, -0.0, -0.0, -0.0], [-0.0, -0.0, -0.0, -0.0]], F) + [0, 5, 0, 0], device=True)
    r.add(np.array([[-0.0, 0.5, 0.25, -0.0]], F))


def test_box_growing_towards_negative_coordinates(run):
    r = run()
    for s in range(5):
        want = r.add(shifted(twin.radar_cloud(800, seed=100 + s), dx=-35.0 * s, dy=-20.0 * s, dz=-3.0 * s), device=bool(s & 1))
    assert want[:, :3].min() < -100.0
    r.check_against_the_library()


# ---- points that do not take part
def test_non_finite_points_and_empty_adds(run):
    r = run()
    assert r.acc.filter().shape == (0, 4) and r.acc.size() == (0, 0)
    r.add(np.zeros((0, 4), F))
    r.add(np.full((300, 4), np.nan, F))                    # the first add with points has no finite one ...
    r.add(np.full((40, 4), np.inf, F), device=True)
    assert r.acc.size()[0] == 0
    first = shifted(twin.radar_cloud(1500, seed=110), dx=-50.0)
    want = r.add(first)                                      # ... so the origin comes from this one
    assert len(want) > 0
    c = twin.radar_cloud(3000, seed=111)
    g = np.random.default_rng(112)
    rows = np.r_[0, len(c) - 1, g.choice(len(c), 100, replace=False)]
    c[rows, g.integers(0, 3, len(rows))] = np.array([np.nan, np.inf, -np.inf], F)[g.integers(0, 3, len(rows))]
    r.add(c)
    r.add(c[::-1], device=True)
    n = r.acc.size()
    r.add(np.full((10, 4), np.nan, F), device=True)
    r.add(np.zeros((0, 4), F), device=True)
    assert r.acc.size()[0] == n[0]
    r.check_against_the_library()


# ---- parameters
@pytest.mark.parametrize("min_pts", [2, 3])
@pytest.mark.parametrize("all_data", [True, False])
def test_min_points_crossed_on_a_later_add(run, min_pts, all_data):
    r = run(0.5, all_data, min_pts)
    c = twin.radar_cloud(3000, seed=120)
    counts = [len(r.add(part, device=bool(i & 1))) for i, part in enumerate(np.array_split(c, 4))]
    assert 0 < counts[0] < counts[-1] < r.acc.size()[0]
    assert all_data or not r.want()[:, 3].any()
    r.check_against_the_library()


def test_anisotropic_leaf_with_inexact_inverse(run):
    r = run((0.3, 0.7, 1.1))
    for s in range(3):
        r.add(twin.radar_cloud(2000, seed=130 + s), device=s == 1)
    r.check_against_the_library()


# ---- the sort paths
@pytest.mark.parametrize("n", [1, 63, 1025, SMALL - 1, SMALL])
def test_small_scan_sort_sizes(run, n):
    """One workgroup sorts a scan of at most SMALL points in LDS: a single point, less than a wave, a
    partial round, the last size; host and device adds take it alike."""
    r = run()
    r.add(twin.radar_cloud(n, seed=300 + n))
    c = shifted(twin.radar_cloud(n, seed=301 + n), dx=-7.0)
    c[:: 7, 1] = np.nan
    r.add(c, device=True)
    r.check_against_the_library()


def test_small_scan_with_every_key_byte_varying(run):
    """Cells spread over the whole range on each axis at leaf 1: all 63 key bits differ between points, so
    the small sort runs all eight passes.  The box is grid overflow; the state's voxel count is the twin's."""
    g = np.random.default_rng(310)
    c = np.concatenate([g.integers(-2**19, 2**19, (3000, 3)) + 0.5, g.uniform(0, 40, (3000, 1))], axis=1).astype(F)
    c[0, :3], c[1, :3] = -2.0**19 + 0.5, 2.0**19 - 0.5
    c = np.concatenate([c, c[:500]])  # repeated cells
    t = acc_twin.VoxelAccumulatorTwin(1.0)
    t.add(c)
    r = run(1.0)
    r.acc.add(c)
    assert r.acc.size() == t.size() and t.overflow()
    d = to_device(c[::-1])
    r.acc.add_device(d.data_ptr(), len(c))
    t.add(c[::-1])
    assert r.acc.size() == t.size()


def test_large_compact_scan_takes_one_sort_and_device_adds_two(run):
    """Above SMALL points a host add reads the scan's box back and sorts a scan-relative key once; a
    device add cannot and sorts the 64-bit key's two words: the same scans through both give the same
    bytes, equal to the twin."""
    a, b = run(), run()
    for s, n in enumerate([SMALL + 1, 9000, 2 * SMALL + 5]):
        c = shifted(twin.radar_cloud(n, seed=140 + s), dx=20.0 * s)
        c[5::11, 2] = np.inf
        a.add(c)
        b.add(c, device=True, check=False)
    assert a.acc.filter().tobytes() == b.acc.filter().tobytes()
    a.check_against_the_library()


@pytest.mark.parametrize("n", [1000, 5000])
def test_scan_wider_than_31_key_bits(run, n):
    """Two clusters 400 km apart on each axis (leaf 0.5: 800,000 cells, inside the range): the scan's own
    box has more than 2^31 cells, so a host add of more than SMALL points sorts twice (2 n = 10,000) and
    a smaller one runs the small sort's upper passes.  Such a box is grid overflow for the full filter
    too, so the filter refuses; the state is whole: its voxel count is the twin's, and after a clear
    the near cluster alone filters as ever."""
    r = run()
    near = twin.radar_cloud(n, seed=150)
    far = shifted(twin.radar_cloud(n, seed=151), dx=4.0e5, dy=4.0e5, dz=4.0e5)
    both = np.concatenate([near, far])[np.random.default_rng(152).permutation(2 * n)]
    r.add(near)
    t = acc_twin.VoxelAccumulatorTwin(0.5)
    t.add(near)
    t.add(both)
    assert t.overflow()
    r.acc.add(both)
    assert r.acc.size() == t.size()
    with pytest.raises(icp4r.ICP4RError) as e:
        r.acc.filter()
    assert e.value.code == icp4r.E_TOO_LARGE
    d = to_device(both)
    r.acc.add_device(d.data_ptr(), len(both))
    t.add(both)
    assert r.acc.size() == t.size()
    r.acc.clear()
    r.seen = np.zeros((0, 4), F)
    r.add(near)


# ---- entries
@pytest.mark.parametrize("floats", [3, 4, 5, 8])
def test_host_strides(run, floats):
    """12, 16, 20 and 32 bytes per point; a 12-byte point has intensity 0."""
    r = run()
    src = twin.radar_cloud(2000, seed=160)
    for half in (src[:1000], src[1000:]):
        c = np.zeros((1000, floats), F)
        k = min(floats, 4)
        c[:, :k] = half[:, :k]
        c[:, 4:] = 77.0
        want = r.add(c)
    assert floats > 3 or not want[:, 3].any()


def test_device_entries_on_a_callers_stream(run):
    import torch

    r = run(0.5, True, 2)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    for s in range(3):
        want = r.add(twin.radar_cloud(3000, seed=170 + s), device=True, stream=stream)
    k, out = device_filter(r.acc, stream)
    assert k == len(want) and same_bits(out[:k], want) and (out[k:] == F(-7.5)).all()
    k, out = device_filter(r.acc, None)
    assert k == len(want) and same_bits(out[:k], want) and (out[k:] == F(-7.5)).all()


def test_add_map_equals_adding_the_stores_points(gpu_ctx, run):
    tree = mapstore.KD_TREE(ctx=gpu_ctx)
    try:
        tree.Build(twin.radar_cloud(3000, seed=180))
        tree.Add_Points(twin.radar_cloud(1500, seed=181), False)
        store = tree.Box_Search([-np.inf] * 3 + [np.inf] * 3)
        assert len(store) == 4500
        r = run()
        r.add(twin.radar_cloud(500, seed=182))
        r.acc.add_map(tree)
        r.seen = np.concatenate([r.seen, store])
        r.check()
        assert same_bits(tree.Box_Search([-np.inf] * 3 + [np.inf] * 3), store)
    finally:
        tree.close()


def raw_filter(acc, out, out_cap):
    k = C.c_int64(12345)
    rc = icp4r.load().icp4r_voxel_acc_filter(acc.handle, out.ctypes.data, out_cap, C.byref(k))
    return rc, k.value


OVERFLOWS = [np.array([[0, 0, 0, 1], [1300, 1300, 1300, 2]], F), np.array([[0.9, 0.9, 0.9, 1], [1290.1, 1290.1, 1290.1, 2]], F)]


@pytest.mark.parametrize("which", [0, 1])
def test_overflow_reached_on_a_later_add(run, which):
    c = OVERFLOWS[which]
    r = run(1.0)
    r.add(c[:1])
    r.acc.add(c[1:])
    with pytest.raises(twin.GridOverflow):
        twin.voxel_filter(c, 1.0)
    out = np.full((4, 4), -7.5, F)
    rc, n = raw_filter(r.acc, out, 4)
    assert rc == icp4r.E_TOO_LARGE and n == -1 and (out == F(-7.5)).all()
    with pytest.raises(icp4r.ICP4RError) as e:
        r.acc.filter()
    assert e.value.code == icp4r.E_TOO_LARGE
    k, dout = device_filter(r.acc)
    assert k == -1 and (dout == F(-7.5)).all()
    assert r.acc.size() == (2, 2)          # the state is whole
    r.acc.add(c[:1])                        # and adds still merge
    assert r.acc.size() == (2, 3)
    r.acc.clear()
    r.seen = np.zeros((0, 4), F)
    assert r.acc.size() == (0, 0)
    r.add(twin.radar_cloud(300, seed=190))


def test_host_add_outside_the_range_is_refused(run):
    r = run()
    first = twin.radar_cloud(1000, seed=200)
    r.add(first)
    before = r.acc.size()
    far = shifted(first, dx=0.5 * 2**20 + 100.0)
    L = icp4r.load()
    assert L.icp4r_voxel_acc_add(r.acc.handle, far.ctypes.data, len(far), 16) == icp4r.E_TOO_LARGE
    with pytest.raises(icp4r.ICP4RError):
        r.acc.add(np.array([[0.0, -1e30, 0.0, 1.0]], F))   # a cell that is no int
    assert r.acc.size() == before
    r.check()                                                # the twin without those adds
    r.add(shifted(first[:50], dx=-0.5 * 2**20 + 200.0), check=False)   # just inside, the other way
    assert r.acc.size() == acc_size_of(r)


def acc_size_of(r):
    t = acc_twin.VoxelAccumulatorTwin(r.leaf, r.all_data, r.min_pts)
    t.add(r.seen)
    return t.size()


def test_device_add_outside_the_range_sets_the_flag_until_clear(run):
    r = run()
    first = twin.radar_cloud(1000, seed=210)
    r.add(first)
    far = to_device(shifted(first, dy=-0.5 * 2**20 - 100.0))
    r.acc.add_device(far.data_ptr(), len(first))
    assert r.acc.size()[0] == len(r.want())                  # the add was skipped whole
    k, dout = device_filter(r.acc)
    assert k == -2 and (dout == F(-7.5)).all()
    out = np.full((4, 4), -7.5, F)
    rc, n = raw_filter(r.acc, out, 4)
    assert rc == icp4r.E_TOO_LARGE and n == -2 and (out == F(-7.5)).all()
    r.acc.add(first[:10])                                    # sticky
    assert device_filter(r.acc)[0] == -2
    r.acc.clear()
    r.seen = np.zeros((0, 4), F)
    r.add(first, device=True)


def test_output_capacity(run):
    r = run()
    want = r.add(twin.radar_cloud(3000, seed=220))
    k = len(want)
    out = np.full((k + 8, 4), -7.5, F)
    rc, n = raw_filter(r.acc, out, k - 1)
    assert rc == icp4r.E_TOO_LARGE and n == k and (out == F(-7.5)).all()
    rc, n = raw_filter(r.acc, out, k)
    assert rc == icp4r.OK and n == k and same_bits(out[:k], want) and (out[k:] == F(-7.5)).all()


def grid_cloud(nx, ny, z):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), axis=-1).reshape(-1, 2)
    c = np.concatenate([g * 0.5 + 0.25, np.full((len(g), 1), z * 0.5 + 0.25), (np.arange(len(g))[:, None] % 41)], axis=1)
    return c.astype(F)


@pytest.mark.parametrize("reserve, device", [(False, False), (False, True), (True, True)])
def test_growth_past_three_times_the_initial_capacity(run, reserve, device):
    """From 1 voxel to 5 x 2,601 + 1 > 3 x INITIAL_CAP, every add of new cells only."""
    r = run()
    if reserve:
        r.acc.reserve(5 * 2601 + 1)
    r.add(np.array([[-3.3, 0.1, 0.1, 1.0]], F), device)
    for z in (4, 1, 3, 0, 2):
        r.add(grid_cloud(51, 51, z), device, check=z in (4, 2))
    assert r.acc.size() == (5 * 2601 + 1, 5 * 2601 + 1) and 5 * 2601 + 1 > 3 * INITIAL_CAP


def test_invalid_arguments(gpu_ctx, run):
    L = icp4r.load()
    h = C.c_void_p()
    for leaf in ((0.0, 0.5, 0.5), (0.5, -1.0, 0.5), (0.5, 0.5, np.inf), (np.nan, 0.5, 0.5)):
        p = voxel.voxel_params(leaf)
        assert L.icp4r_voxel_acc_create(gpu_ctx.handle, C.byref(p), C.byref(h)) == icp4r.E_INVALID and not h
    p = voxel.voxel_params(0.5)
    assert L.icp4r_voxel_acc_create(None, C.byref(p), C.byref(h)) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_create(gpu_ctx.handle, None, C.byref(h)) == icp4r.E_INVALID
    r = run()
    a = twin.radar_cloud(10, seed=230)
    acc = r.acc.handle
    k = C.c_int64()
    assert L.icp4r_voxel_acc_add(acc, a.ctypes.data, 10, 8) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_add(acc, a.ctypes.data, 10, 18) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_add(acc, None, 10, 16) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_add(acc, a.ctypes.data, -1, 16) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_add(acc, a.ctypes.data, 2**31, 16) == icp4r.E_TOO_LARGE
    assert L.icp4r_voxel_acc_add_device(acc, None, 10, None) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_add_device(acc, 256, 2**31, None) == icp4r.E_TOO_LARGE
    assert L.icp4r_voxel_acc_add_map(acc, None) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_filter(acc, None, 0, None) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_filter(acc, None, 5, C.byref(k)) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_filter_device(acc, None, None, None) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_reserve(acc, -1) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_reserve(acc, 2**31) == icp4r.E_TOO_LARGE
    assert L.icp4r_voxel_acc_add(None, a.ctypes.data, 10, 16) == icp4r.E_INVALID
    assert L.icp4r_voxel_acc_add(acc, None, 0, 16) == icp4r.OK
    assert L.icp4r_voxel_acc_filter(acc, None, 0, C.byref(k)) == icp4r.OK and k.value == 0
    assert r.acc.size() == (0, 0)


def test_accumulator_of_a_closed_context():
    ctx = icp4r.Context(0)
    acc = voxel.VoxelAccumulator(0.5, ctx=ctx)
    try:
        acc.add(twin.radar_cloud(100, seed=240))
        assert len(acc.filter()) > 0
        ctx.close()
        c = twin.radar_cloud(10, seed=241)
        for call in (lambda: acc.add(c), lambda: acc.add_device(256, 10), lambda: acc.filter_device(256, 256), acc.size,
                     acc.clear, lambda: acc.reserve(10), acc.filter):
            with pytest.raises(icp4r.ICP4RError) as e:
                call()
            assert e.value.code == icp4r.E_INVALID
    finally:
        acc.close()
        ctx.close()


def test_filter_twice_and_two_runs_give_identical_bytes(run):
    outs = []
    for _ in range(2):
        r = run()
        r.add(twin.crowded_cloud(), check=False)
        for s in range(3):
            r.add(shifted(twin.radar_cloud(4000, seed=250 + s), dx=5.0 * s), device=bool(s & 1), check=False)
        a, b = r.acc.filter(), r.acc.filter()
        assert a.tobytes() == b.tobytes() and len(a) > 0
        r.add(twin.radar_cloud(10, seed=259))  # adds may follow a filter
        outs.append(a.tobytes())
    assert outs[0] == outs[1]


def test_facade_program_equals_the_twin(tmp_path):
    """tests/cpp/voxel_acc_callsite.cpp: three scans from files through voxel_acc_compat.hpp."""
    exe = compile_acc_callsite(tmp_path, pcl18=False)
    scans = [shifted(twin.radar_cloud(2000, seed=260 + s), dx=4.0 * s) for s in range(3)]
    paths = []
    for s, c in enumerate(scans):
        paths.append(str(tmp_path / f"scan{s}.bin"))
        c.tofile(paths[-1])
    dst = str(tmp_path / "out.bin")
    r = subprocess.run([exe, dst, *paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert same_bits(tools.read_result(dst), twin.voxel_filter(np.concatenate(scans), 0.5))
