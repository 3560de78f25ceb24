"""Scan-to-map store: exact, order- and multiplicity-sensitive comparison with the oracle.

tests/test_map.py compares kept SETS and tolerates mismatches within 1e-3 deg of a sector edge.  Here
the ambiguity is taken out of the INPUT instead (helpers.sector_edge_filter: every point whose
|dh| lies within EDGE_TOL_DEG of 60 or 300 for a query is removed from the map, at most 1e-4 of it
per query), every map carries the point's index in its intensity, and each comparison is
np.array_equal(got, pts[oracle indices]) — count, order and multiplicity at once.  The radius test
needs no filter: calc_dist is unfused float on both sides.

Branches reached here and nowhere else: the tile carry of sector_scan_kernel (a second tile of 1024
block counts first exists at 4096*1024 + 1 points), chosen ballot patterns in sector_write_kernel,
the E_TOO_LARGE return, the hip_stream argument of the device search, Build over a larger map and
the timers.
"""
import ctypes as C

import numpy as np
import pytest
from helpers import (EDGE_MAX_SHARE, MAP_QUERIES, filtered_map, point_at, random_map, sector_edge_filter,
                     sector_keep_f64)

BLOCK = 4096          # kSecBlock: points per workgroup of the count / write kernels
TILE = 1024           # block counts per tile of sector_scan_kernel
RADIUS = 80.0
CARRY_N = BLOCK * TILE + 1
CARRY_QUERIES = (([0, 0, 0], 0.0), ([0, 0, 0], 179.5))  # the second keeps ~22 % through dh > 300


def _exact(tree, oracle_mod, pts, c, radius, heading):
    """Device rows == the oracle's rows, in order.  Returns the kept count."""
    got = tree.Sector_Search(c, radius, heading)
    ref = oracle_mod.sector_search(pts, c, radius, heading)
    want = np.zeros((len(ref), 4), np.float32)
    k = min(pts.shape[1], 4)
    want[:, :k] = pts[ref, :k]
    assert got.shape == want.shape, (got.shape, want.shape, c, heading)
    assert np.array_equal(got, want), (c, heading)
    return len(ref)


# ------------------------------------------------------------------------------------------- A1 (CPU)
def test_edge_filter_makes_the_oracle_unambiguous(oracle_mod):
    """After the filter the float64 keep mask equals the oracle's float one: no kept/dropped decision
    that is left depends on the rounding of asinf or of the heading."""
    n = 300_000
    raw = random_map(np.random.default_rng(n), n)
    raw[:8] = np.array([point_at(80, 10), point_at(80, 60), point_at(80, -60), point_at(20, 180), [0, 0, 0, 1],
                        point_at(600, 179), point_at(600, -179), point_at(1, 0)], np.float32)
    for c, heading in MAP_QUERIES:
        pts, removed = sector_edge_filter(raw, [(c, heading)])
        assert removed[0] <= EDGE_MAX_SHARE * n and len(pts) == n - removed[0]
        orc = np.zeros(len(pts), bool)
        orc[oracle_mod.sector_search(pts, c, RADIUS, heading)] = True
        f64 = sector_keep_f64(pts, c, RADIUS, heading)
        assert np.array_equal(orc, f64), (c, heading, np.nonzero(orc != f64)[0][:8])
        assert 1000 < orc.sum() < n


def test_edge_filter_removes_exact_edges_and_caps():
    pts = np.array([point_at(10, 0), point_at(10, 60), point_at(10, -60), point_at(10, 59.9), point_at(10, 180)],
                   np.float32)
    with pytest.raises(AssertionError):  # 2 of 5 points on an edge: far above the 1e-4 cap
        sector_edge_filter(pts, [([0, 0, 0], 0.0)])
    big = np.concatenate([np.tile(np.array([point_at(10, 5)], np.float32), (30_000, 1)), pts[1:3]])
    kept, removed = sector_edge_filter(big, [([0, 0, 0], 0.0)])
    assert removed == [2] and len(kept) == 30_000


# ------------------------------------------------------------------------------------------- A3
@pytest.fixture(scope="module")
def carry_map():
    """4096*1024 + 1 edge-filtered points, built once for both carry tests."""
    pts, removed = filtered_map(np.random.default_rng(4096), CARRY_N, CARRY_QUERIES)
    print("edge filter removed per query:", removed)
    pts[-1, :3] = point_at(10, 0)[:3]  # block 1024's only point: ahead and near, kept at heading 0
    pts.setflags(write=False)
    return pts


@pytest.mark.gpu
def test_scan_carry_second_tile(gpu_ctx, oracle_mod, carry_map):
    """1025 blocks: the last block's offset is the carry out of the first tile of 1024."""
    from icp4r.mapstore import KD_TREE

    pts = carry_map
    tree = KD_TREE(ctx=gpu_ctx)
    try:
        tree.Build(pts[: CARRY_N // 2])
        tree.Add_Points(pts[CARRY_N // 2:], False)
        assert tree.size() == CARRY_N
        # the one point of block 1024 is kept by the first query: it is written at offset = carry
        assert oracle_mod.sector_search(pts, CARRY_QUERIES[0][0], RADIUS, CARRY_QUERIES[0][1])[-1] == CARRY_N - 1
        for c, heading in CARRY_QUERIES:  # the second query's count is the carry summed over both tiles
            assert _exact(tree, oracle_mod, pts, c, RADIUS, heading) > TILE
    finally:
        tree.close()


@pytest.mark.gpu
def test_scan_carry_one_full_tile(gpu_ctx, oracle_mod, carry_map):
    """Exactly 1024 blocks: one full tile, the carry written and never read."""
    from icp4r.mapstore import KD_TREE

    pts = carry_map[: BLOCK * TILE]
    tree = KD_TREE(ctx=gpu_ctx)
    try:
        tree.Build(pts)
        assert tree.size() == BLOCK * TILE
        c, heading = CARRY_QUERIES[1]
        assert _exact(tree, oracle_mod, pts, c, RADIUS, heading) > TILE
    finally:
        tree.close()


# ------------------------------------------------------------------------------------------- A4
BALLOT_N = 2 * BLOCK + 300


def _ballot_mask(name):
    i = np.arange(BALLOT_N)
    block, within = i // BLOCK, i % BLOCK
    rnd, tid = within // 256, within % 256
    wave, lane = tid // 64, tid % 64
    return {
        "all": np.ones(BALLOT_N, bool),
        "none": np.zeros(BALLOT_N, bool),
        "lane63": lane == 63,
        "lanes32_63": lane >= 32,
        "lanes0_31": lane < 32,
        "wave3": wave == 3,
        "waves1_and_3": (wave == 1) | (wave == 3),  # wave 3 ranks behind wave 1's count, not behind 0
        "round15": rnd == 15,
        "first_and_last": (i == 0) | (i == BALLOT_N - 1),
        "empty_block_between": block != 1,
        "random50": np.random.default_rng(50).random(BALLOT_N) < 0.5,
    }[name]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["all", "none", "lane63", "lanes32_63", "lanes0_31", "wave3", "waves1_and_3",
                                     "round15", "first_and_last", "empty_block_between", "random50"])
def test_write_kernel_ballot_patterns(gpu_ctx, oracle_mod, pattern):
    """A chosen keep pattern over two full blocks and a ragged one: keepers at heading 0, droppers at
    180 (no edge in reach), told apart by the index in the intensity."""
    from icp4r.mapstore import KD_TREE

    keep = _ballot_mask(pattern)
    pts = np.where(keep[:, None], np.array(point_at(10, 0), np.float32), np.array(point_at(10, 180), np.float32))
    pts = np.ascontiguousarray(pts, np.float32)
    pts[:, 3] = np.arange(BALLOT_N, dtype=np.float32)
    ref = oracle_mod.sector_search(pts, [0, 0, 0], RADIUS, 0.0)
    assert np.array_equal(ref, np.nonzero(keep)[0])  # the oracle keeps the pattern, nothing else
    tree = KD_TREE(ctx=gpu_ctx)
    try:
        tree.Build(pts)
        got = tree.Sector_Search([0, 0, 0], RADIUS, 0.0)
        assert got.shape == (int(keep.sum()), 4)
        assert np.array_equal(got, pts[ref])
    finally:
        tree.close()


# ------------------------------------------------------------------------------------------- A5
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097])
def test_shapes_around_the_block_size(gpu_ctx, oracle_mod, n):
    """Random edge-filtered maps at the workgroup and block boundaries; (N, 3), (N, 4) and (N, 6) input
    rows cover pack_host's strides (a 3-float row has no intensity: 0)."""
    from icp4r.mapstore import KD_TREE

    for ncols in (3, 4, 6):
        pts, _ = filtered_map(np.random.default_rng(1000 * n + ncols), n, MAP_QUERIES, extent=60.0, ncols=ncols)
        tree = KD_TREE(ctx=gpu_ctx)
        try:
            tree.Build(pts[: n // 2])
            tree.Add_Points(pts[n // 2:], False)
            assert tree.size() == n
            kept = sum(_exact(tree, oracle_mod, pts, c, RADIUS, heading) for c, heading in MAP_QUERIES)
            assert kept > 0 or n == 1
        finally:
            tree.close()


# ------------------------------------------------------------------------------------------- A6
def _raw_search(tree, c, radius, heading, out, cap):
    import icp4r

    c = np.ascontiguousarray(np.asarray(c, np.float32))
    k = C.c_int64(-1)
    rc = icp4r.load().icp4r_map_sector_search(tree.handle, c.ctypes.data, float(radius), float(heading),
                                              out.ctypes.data if out is not None else None, cap, C.byref(k))
    return rc, k.value


@pytest.fixture
def small_tree(gpu_ctx):
    from icp4r.mapstore import KD_TREE

    pts, _ = filtered_map(np.random.default_rng(77), 5000, MAP_QUERIES, extent=60.0)
    tree = KD_TREE(ctx=gpu_ctx)
    tree.Build(pts)
    yield tree, pts
    tree.close()


@pytest.mark.gpu
def test_out_cap_too_small(small_tree, oracle_mod):
    import icp4r

    tree, pts = small_tree
    c, heading = MAP_QUERIES[0]
    ref = oracle_mod.sector_search(pts, c, RADIUS, heading)
    k = len(ref)
    assert k > 100
    guard = 16
    out = np.full((k - 1 + guard, 4), np.float32(-12345.5))
    before = out.copy()
    rc, cnt = _raw_search(tree, c, RADIUS, heading, out, k - 1)
    assert rc == icp4r.E_TOO_LARGE and cnt == k
    assert np.array_equal(out[k - 1:], before[k - 1:])  # nothing past out_cap
    rc, cnt = _raw_search(tree, c, RADIUS, heading, out, k)  # the exact capacity is enough
    assert rc == icp4r.OK and cnt == k
    assert np.array_equal(out[:k], pts[ref]) and np.array_equal(out[k:], before[k:])


@pytest.mark.gpu
def test_radius_nan_negative_zero(small_tree, oracle_mod):
    import icp4r

    tree, pts = small_tree
    out = np.zeros((len(pts), 4), np.float32)
    for bad in (float("nan"), -1.0, -0.5):
        rc, _ = _raw_search(tree, [0, 0, 0], bad, 0.0, out, len(pts))
        assert rc == icp4r.E_INVALID, bad
    c, heading = MAP_QUERIES[2]  # heading 179.5: the dh > 300 clause keeps points whatever the radius
    ref = oracle_mod.sector_search(pts, c, 0.0, heading)
    assert len(ref) > 100
    assert np.array_equal(tree.Sector_Search(c, 0.0, heading), pts[ref])
    assert len(oracle_mod.sector_search(pts, c, 0.0, 0.0)) == 0
    assert len(tree.Sector_Search(c, 0.0, 0.0)) == 0


@pytest.mark.gpu
def test_device_search_on_a_caller_stream(small_tree):
    import torch

    tree, pts = small_tree
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    for c, heading in MAP_QUERIES:
        host = tree.Sector_Search(c, RADIUS, heading)
        d_out = torch.full((len(pts) + 8, 4), -7.0, dtype=torch.float32, device=dev)
        d_cnt = torch.full((3,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        tree.sector_search_device(c, RADIUS, heading, d_out.data_ptr(), d_cnt[1:].data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        cnt, out = d_cnt.cpu().numpy(), d_out.cpu().numpy()
        assert cnt.tolist() == [-1, len(host), -1]
        assert out[: len(host)].tobytes() == host.tobytes()
        assert (out[len(host):] == -7.0).all()  # nothing past the kept count


@pytest.mark.gpu
def test_build_replaces_a_larger_map(gpu_ctx, oracle_mod):
    from icp4r.mapstore import KD_TREE

    big, _ = filtered_map(np.random.default_rng(5), 3 * BLOCK + 7, MAP_QUERIES, extent=60.0)
    small, _ = filtered_map(np.random.default_rng(6), 300, MAP_QUERIES, extent=60.0)
    tree = KD_TREE(ctx=gpu_ctx)
    try:
        tree.Build(big)
        assert tree.size() == len(big)
        assert _exact(tree, oracle_mod, big, MAP_QUERIES[0][0], RADIUS, MAP_QUERIES[0][1]) > 300
        tree.Build(small)
        assert tree.size() == 300
        for c, heading in MAP_QUERIES:
            _exact(tree, oracle_mod, small, c, RADIUS, heading)
    finally:
        tree.close()


@pytest.mark.gpu
def test_timers_count_searches(small_tree):
    tree, _ = small_tree
    tree.reset_timers()
    assert tree.time_ms() == (0.0, 0)
    for k in range(1, 4):
        tree.Sector_Search([0, 0, 0], RADIUS, 10.0 * k)
        ms, calls = tree.time_ms()
        assert calls == k and ms > 0.0
    tree.reset_timers()
    assert tree.time_ms() == (0.0, 0)
    tree.Sector_Search([0, 0, 0], RADIUS, 0.0)
    assert tree.time_ms()[1] == 1
