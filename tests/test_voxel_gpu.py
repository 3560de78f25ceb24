"""Voxel-grid downsampling on the GPU (include/icp4r/icp4r_voxel.h) against the contract's numpy twin
(tests/voxel_grid_twin.py; pinned to the C++ restatement of PCL's loop in tests/test_voxel.py): whole
arrays — count, order and bits — with no tolerance.  Host entry, device entry, the map entries and
the C++ facade program."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import icp4r
import voxel_grid_twin as twin
import voxel_tools as tools
from icp4r import mapstore, voxel
from voxel_tools import same_bits

pytestmark = pytest.mark.gpu
F = np.float32
BLOCK = 4096  # the compactions' and the radix sort's block


@pytest.fixture(scope="module")
def vg(gpu_ctx):
    return lambda leaf=0.5, all_data=True, min_pts=0: _grid(gpu_ctx, leaf, all_data, min_pts)


def _grid(ctx, leaf, all_data, min_pts):
    g = voxel.VoxelGrid(ctx)
    lf = np.broadcast_to(np.asarray(leaf, F).reshape(-1), (3,))
    g.setLeafSize(float(lf[0]), float(lf[1]), float(lf[2]))
    g.setDownsampleAllData(all_data)
    g.setMinimumPointsNumberPerVoxel(min_pts)
    return g


def check(vg, cloud, leaf=0.5, all_data=True, min_pts=0):
    got = vg(leaf, all_data, min_pts).filter(cloud)
    want = twin.voxel_filter(cloud, leaf, all_data, min_pts)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert same_bits(got, want)
    return want


def raw_filter(ctx, cloud, leaf, out, out_cap):
    """The C entry itself: -> (status, out_n)."""
    a = np.ascontiguousarray(cloud, F)
    p = voxel.voxel_params(leaf)
    k = C.c_int64(12345)
    rc = icp4r.load().icp4r_voxel_filter(ctx.handle, a.ctypes.data, len(a), a.shape[1] * 4, C.byref(p), out.ctypes.data,
                                         out_cap, C.byref(k))
    return rc, k.value


# ---- host entry against the twin
@pytest.mark.parametrize("n", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 5])
def test_block_edges(vg, n):
    want = check(vg, twin.radar_cloud(n, seed=100 + n))
    assert 0 < len(want) <= n


def test_one_voxel_of_9000_members(vg):
    """One segment across three blocks, one long chain (the wave-cooperative walk, 141 chunks)."""
    r = np.random.default_rng(5)
    c = np.concatenate([r.uniform(0.01, 0.49, (9000, 3)), r.uniform(0, 40, (9000, 1))], axis=1).astype(F)
    assert len(check(vg, c)) == 1


def test_every_point_its_own_voxel(vg):
    g = np.stack(np.meshgrid(np.arange(25), np.arange(20), np.arange(10), indexing="ij"), axis=-1).reshape(-1, 3)
    c = np.concatenate([g + 0.25, np.arange(len(g))[:, None] % 97], axis=1).astype(F)
    c = c[np.random.default_rng(6).permutation(len(c))]
    assert len(check(vg, c)) == 5000


def test_crowded_voxels(vg):
    """50 sites x 40 copies: members beyond the one-lane walk's 16, order reaching the bits."""
    want = check(vg, twin.crowded_cloud())
    assert 40 <= len(want) <= 50


def test_voxel_sizes_around_the_short_walk_limit(vg):
    """Voxels of 1 .. 70 members side by side: the one-lane walk (<= 16, in fours), the cooperative walk
    (> 16), a chunk boundary at 64, all in one wave."""
    r = np.random.default_rng(8)
    rows = []
    for m in range(1, 71):
        rows.append(np.concatenate([r.uniform(0.05, 0.45, (m, 3)) + [0.5 * m, 0.0, 0.0], r.uniform(0, 40, (m, 1))], axis=1))
    c = np.concatenate(rows).astype(F)
    c = c[r.permutation(len(c))]
    assert len(check(vg, c)) == 70


def test_non_finite_points_scattered(vg):
    c = twin.radar_cloud(10000, seed=9)
    r = np.random.default_rng(10)
    bad = np.array([np.nan, np.inf, -np.inf], F)
    rows = np.r_[0, len(c) - 1, r.choice(len(c), 200, replace=False)]
    c[rows, r.integers(0, 3, len(rows))] = bad[r.integers(0, 3, len(rows))]
    c[BLOCK:2 * BLOCK, 1] = np.nan  # a whole block
    want = check(vg, c)
    assert 0 < len(want) < 6000
    assert len(vg().filter(np.full((300, 4), np.nan, F))) == 0
    assert len(vg().filter(np.zeros((0, 4), F))) == 0


@pytest.mark.parametrize("leaf, lo, hi", [(2.0, 1, 2**8), (0.5, 2**8, 2**16), (0.0625, 2**16, 2**24),
                                          (0.0078125, 2**24, 2**31)])
def test_key_widths(vg, leaf, lo, hi):
    """One cloud, the leaf sets how many bits the leaf index needs: one to four radix passes."""
    r = np.random.default_rng(11)
    c = (r.uniform(0, 1, (3000, 4)) * [8.0, 8.0, 2.0, 40.0]).astype(F)
    _, _, div, _ = twin.grid(c, leaf)
    assert lo <= div[0] * div[1] * div[2] < hi
    check(vg, c, leaf)


def test_leaf_index_at_or_above_2_30(vg):
    r = np.random.default_rng(12)
    a = r.uniform(0, 3, (500, 4))
    b = r.uniform(0, 3, (500, 4)) + [1000.0, 1000.0, 1100.0, 0.0]
    c = np.concatenate([a, b]).astype(F)[r.permutation(1000)]
    inv, min_b, div, _ = twin.grid(c, 1.0)
    assert twin.leaf_index(c, inv, min_b, div).max() >= 2**30
    check(vg, c, 1.0)


def test_denormal_coordinates(vg):
    """A denormal coordinate keeps its cell (floorf of a denormal product) and its bits (a lone member's
    centroid is the member): nothing is flushed to zero."""
    d = F(1e-40)
    assert d != 0 and d < np.finfo(F).tiny
    c = np.array([[d, 0.2, 0.2, 1.0], [-d, 0.2, 0.2, 2.0], [0.3, 0.2, 0.2, d], [0.2, -d, 0.1, 4.0]], F)
    want = check(vg, c)
    assert len(want) == 3 and (want.view(np.uint32) == (-d).view(np.uint32)).any()


def test_anisotropic_leaf(vg):
    check(vg, twin.radar_cloud(5000, seed=13), (0.3, 0.5, 1.0))


@pytest.fixture(scope="module")
def cloud6000():
    return twin.radar_cloud(6000, seed=14)


@pytest.mark.parametrize("min_pts", [0, 1, 2, 5])
@pytest.mark.parametrize("all_data", [False, True])
def test_min_points_and_all_data(vg, cloud6000, min_pts, all_data):
    want = check(vg, cloud6000, 0.5, all_data, min_pts)
    assert len(want) > 0 and (all_data or not want[:, 3].any())


@pytest.mark.parametrize("floats", [3, 4, 5, 8])
def test_strides(vg, cloud6000, floats):
    """12, 16, 20 and 32 bytes per point; a 12-byte point has intensity 0."""
    c = np.zeros((2000, floats), F)
    k = min(floats, 4)
    c[:, :k] = cloud6000[:2000, :k]
    c[:, 4:] = 77.0
    want = check(vg, c)
    assert floats > 3 or not want[:, 3].any()


def test_output_capacity(gpu_ctx, cloud6000):
    """One row short: ICP4R_E_TOO_LARGE, *out_n = the number needed, nothing written."""
    want = twin.voxel_filter(cloud6000, 0.5)
    k = len(want)
    out = np.full((k + 8, 4), -7.5, F)
    rc, n = raw_filter(gpu_ctx, cloud6000, 0.5, out, k - 1)
    assert rc == icp4r.E_TOO_LARGE and n == k and (out == F(-7.5)).all()
    rc, n = raw_filter(gpu_ctx, cloud6000, 0.5, out, k)
    assert rc == icp4r.OK and n == k and same_bits(out[:k], want) and (out[k:] == F(-7.5)).all()


OVERFLOWS = [np.array([[0, 0, 0, 1], [1300, 1300, 1300, 2]], F), np.array([[0.9, 0.9, 0.9, 1], [1290.1, 1290.1, 1290.1, 2]], F)]


@pytest.mark.parametrize("which", [0, 1])
def test_grid_overflow(gpu_ctx, vg, which):
    c = OVERFLOWS[which]
    with pytest.raises(twin.GridOverflow):
        twin.voxel_filter(c, 1.0)
    out = np.full((4, 4), -7.5, F)
    rc, n = raw_filter(gpu_ctx, c, 1.0, out, 4)
    assert rc == icp4r.E_TOO_LARGE and n == -1 and (out == F(-7.5)).all()
    with pytest.raises(icp4r.ICP4RError) as e:
        vg(1.0).filter(c)
    assert e.value.code == icp4r.E_TOO_LARGE


def test_invalid_arguments(gpu_ctx, cloud6000):
    out = np.zeros((10, 4), F)
    L = icp4r.load()
    k = C.c_int64()
    for leaf in ((0.0, 0.5, 0.5), (0.5, -1.0, 0.5), (0.5, 0.5, np.inf), (np.nan, 0.5, 0.5)):
        rc, _ = raw_filter(gpu_ctx, cloud6000[:10], leaf, out, 10)
        assert rc == icp4r.E_INVALID, leaf
    p = voxel.voxel_params(0.5)
    a = cloud6000[:10].copy()
    assert L.icp4r_voxel_filter(gpu_ctx.handle, a.ctypes.data, 10, 8, C.byref(p), out.ctypes.data, 10, C.byref(k)) == icp4r.E_INVALID
    assert L.icp4r_voxel_filter(gpu_ctx.handle, None, 10, 16, C.byref(p), out.ctypes.data, 10, C.byref(k)) == icp4r.E_INVALID
    assert L.icp4r_voxel_filter(gpu_ctx.handle, a.ctypes.data, 2**31, 16, C.byref(p), out.ctypes.data, 10, C.byref(k)) == icp4r.E_TOO_LARGE
    assert L.icp4r_voxel_filter(gpu_ctx.handle, None, 0, 16, C.byref(p), None, 0, C.byref(k)) == icp4r.OK and k.value == 0


# ---- the other entries
def device_filter(grid, cloud, stream=None):
    import torch

    dev = torch.device("cuda", 0)
    n = len(cloud)
    d_in = torch.from_numpy(np.ascontiguousarray(cloud, F)).to(dev)
    d_out = torch.full((n, 4), -7.5, dtype=torch.float32, device=dev)
    d_cnt = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # torch's copies and fills run on its stream
    grid.filter_device(d_in.data_ptr(), n, d_out.data_ptr(), d_cnt.data_ptr(), stream.cuda_stream if stream else None)
    torch.cuda.synchronize()
    return int(d_cnt.item()), d_out.cpu().numpy()


def test_device_entry_on_a_callers_stream(vg, cloud6000):
    import torch

    host = vg(0.5, True, 2).filter(cloud6000)
    for stream in (torch.cuda.Stream(torch.device("cuda", 0)), None):
        k, out = device_filter(vg(0.5, True, 2), cloud6000, stream)
        assert k == len(host) and same_bits(out[:k], host) and (out[k:] == F(-7.5)).all()
    ms, calls = vg().time_ms()
    assert calls >= 3 and ms > 0.0


@pytest.mark.parametrize("which", [0, 1])
def test_device_entry_stores_minus_one_on_overflow(vg, which):
    k, out = device_filter(vg(1.0), OVERFLOWS[which])
    assert k == -1 and (out == F(-7.5)).all()


def test_device_entry_without_a_finite_point(vg):
    k, _ = device_filter(vg(), np.full((100, 4), np.nan, F))
    assert k == 0


ALL = [-np.inf] * 3 + [np.inf] * 3


def scans(count, n, seed):
    r = np.random.default_rng(seed)
    for s in range(count):
        yaw = 0.1 * s
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        yield twin.radar_cloud(n, seed + s), R, np.array([2.0 * s, 0.5 * s, 0.0]) + r.normal(0, 0.01, 3)


def test_map_entries(gpu_ctx):
    """Build + three add_scan, then voxel_filter: equal to the twin on the store's content; the store and
    its k-NN index are as they were."""
    import torch

    tree = mapstore.KD_TREE(ctx=gpu_ctx)
    try:
        tree.Build(twin.radar_cloud(3000, seed=20))
        for scan, R, t in scans(3, 1500, 21):
            tree.add_scan(scan, R, t)
        tree.index_build()
        store = tree.Box_Search(ALL)  # every stored point (all finite), insertion order
        ptr, n = tree.points_device()
        stats = tree.index_stats()
        assert n == 7500 == len(store) and stats["indexed"] == n
        want = twin.voxel_filter(store, 0.5)
        got = tree.voxel_filter(0.5)
        assert same_bits(got, want) and 0 < len(want) < n
        assert same_bits(tree.voxel_filter((0.3, 0.5, 1.0), False, 2), twin.voxel_filter(store, (0.3, 0.5, 1.0), False, 2))
        dev = torch.device("cuda", 0)
        d_out = torch.full((n, 4), -7.5, dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        tree.voxel_filter_device(0.5, d_out.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert int(d_cnt.item()) == len(want) and same_bits(d_out[: len(want)].cpu().numpy(), want)
        assert tree.points_device() == (ptr, n) and tree.index_stats() == stats
        assert same_bits(tree.Box_Search(ALL), store)
    finally:
        tree.close()


def test_map_of_a_closed_context_raises():
    ctx = icp4r.Context(0)
    tree = mapstore.KD_TREE(ctx=ctx)
    try:
        tree.Build(twin.radar_cloud(100, seed=30))
        assert len(tree.voxel_filter(0.5)) > 0
        ctx.close()
        for call in (lambda: tree.voxel_filter(0.5), lambda: tree.voxel_filter_device(0.5, 256, 256)):
            with pytest.raises(icp4r.ICP4RError) as e:
                call()
            assert e.value.code == icp4r.E_INVALID
    finally:
        tree.close()
        ctx.close()


def test_facade_program_equals_the_twin(tmp_path, cloud6000):
    """tests/cpp/voxel_callsite.cpp: the node's four lines through voxel_compat.hpp (32-byte PointXYZI)."""
    exe = tools.compile_callsite(tmp_path, pcl18=False)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    cloud6000.tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert same_bits(tools.read_result(dst), twin.voxel_filter(cloud6000, 0.5))


def test_two_runs_give_identical_bytes(vg):
    c = np.concatenate([twin.crowded_cloud(), twin.radar_cloud(9000, seed=31)])
    a, b = vg().filter(c), vg().filter(c)
    assert a.tobytes() == b.tobytes() and len(a) > 0
