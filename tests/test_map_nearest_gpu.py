"""The store's Nearest_Search on the device, held to the contract's numpy twin (tests/map_nearest_twin.py)
as arrays — points, distance bits, insertion positions and found — through the index (ICP4R_MAP_KNN_INDEX:
Morton order, 16-point leaves, a 64-ary tree of boxes, so sizes around 16, 1,024, 65,536 and 4,194,304 are
where a level starts), through ICP4R_MAP_KNN_BRUTE and through the default choice; and through the twin to what
the reference's own tree answered (tests/golden/ikd_nearest.npz).  Every tree is closed by `trees`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_edit_twin as edit
import map_nearest_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB = os.path.join(ROOT, "icp-4dradar_amd", "icp4r", "_lib")
F = np.float32
INDEX, BRUTE = 2, 1
PATHS = (INDEX, BRUTE, 0)
SIZES = (1, 4, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 65537, 200000)


@pytest.fixture
def trees(gpu_ctx):
    from icp4r.mapstore import KD_TREE

    made = []

    def make(ds=0.5):
        t = KD_TREE(0.5, 0.6, ds, ctx=gpu_ctx)
        made.append(t)
        return t

    yield make
    for t in made:
        t.close()


def cloud(rng, n, ext=50.0, first=0):
    p = np.zeros((n, 4), F)
    p[:, :3] = rng.uniform(-ext, ext, (n, 3))
    p[:, 2] *= F(0.1)
    p[:, 3] = np.arange(first, first + n)
    return p


def same(got, want):
    gp, gd, gi, gf = got
    wp, wd, wi, wf = want
    assert np.array_equal(gf, wf), ("found", np.flatnonzero(gf != wf)[:5])
    assert np.array_equal(gi, wi), ("index", np.argwhere(gi != wi)[:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), ("dist", np.argwhere(gd != wd)[:5])
    assert np.array_equal(gp.view(np.uint32), wp.view(np.uint32)), "points"


def check(tree, store, queries, k, max_dist=np.inf, paths=PATHS):
    """The store's answer on every path == the twin's (computed once); -> the twin's."""
    want = twin.nearest_search(store, queries, k, max_dist)
    for flags in paths:
        same(tree.nearest_search(queries, k, max_dist, flags=flags), want)
    return want


# ------------------------------------------------------------------------------- sizes and shapes
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_map_sizes(trees, n):
    rng = np.random.default_rng(n)
    store = cloud(rng, n)
    t = trees()
    t.Build(store)
    q = cloud(rng, 65, 65.0)
    q[:8, :3] = store[rng.integers(0, n, 8), :3]  # queries equal to stored points
    _, d, _, f = check(t, store, q, 5)
    assert (f == min(5, n)).all() and (d[:8, 0] == 0).all()
    md = 3.0 if n < 2000 else 2.0 if n < 100000 else 0.5
    f = check(t, store, q[:33], 20, md)[3]
    if n >= 1023:
        assert (f == 0).any() and (f > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (64 ** 3 * 16, 64 ** 3 * 16 + 1))
def test_fourth_tree_level(trees, n):
    """4,194,304 points are three levels of boxes with the top one full (64 nodes); one point more needs a fourth."""
    rng = np.random.default_rng(7)
    store = cloud(rng, n, 400.0)
    t = trees()
    t.Build(store)
    q = cloud(rng, 6, 420.0)
    q[:2, :3] = store[[0, n - 1], :3]
    assert (check(t, store, q, 5, paths=(INDEX, BRUTE))[1][:2, 0] == 0).all()
    f = check(t, store, q, 20, 1.0, paths=(INDEX,))[3]
    assert (f > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", (1, 63, 64, 65, 257))
def test_query_counts_and_k(trees, nq):
    rng = np.random.default_rng(100 + nq)
    store = cloud(rng, 5000)
    t = trees()
    t.Build(store)
    q = cloud(rng, nq, 65.0)
    for k in (1, 5, 20, 32):
        assert (check(t, store, q, k)[3] == k).all()
    # rows with no candidate, with fewer than k and with k
    f = check(t, store, q, 20, 6.0)[3]
    if nq >= 63:
        assert (f == 0).any() and ((f > 0) & (f < 20)).any() and (f == 20).any()


@pytest.mark.gpu
def test_k_greater_than_the_map(trees):
    rng = np.random.default_rng(3)
    store = cloud(rng, 4)
    t = trees()
    t.Build(store)
    _, d, i, f = check(t, store, cloud(rng, 65, 65.0), 20)
    assert (f == 4).all() and (i[:, 4:] == -1).all() and np.isinf(d[:, 4:]).all()


@pytest.mark.gpu
def test_query_placement(trees):
    rng = np.random.default_rng(4)
    store = cloud(rng, 20000)
    t = trees()
    t.Build(store)
    far = cloud(rng, 130, 10.0)
    far[:, 0] += F(500.0)  # all far outside on one side
    check(t, store, far, 5)
    assert (check(t, store, far, 5, 100.0)[3] == 0).all()
    mixed = cloud(rng, 128, 50.0)
    mixed[::3, :3] *= F(40.0)  # near and far queries side by side in the rows (and, sorted, in some wave)
    check(t, store, mixed, 20)
    check(t, store, mixed, 5, 4.0)
    on = store[rng.integers(0, len(store), 200)].copy()
    _, d, i, _ = check(t, store, on, 1)
    assert (d[:, 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ("ball", "identical", "lattice", "flat", "line"))
def test_map_shapes(trees, shape):
    rng = np.random.default_rng(5)
    if shape == "ball":  # 90 % of the map within 1 m
        store = cloud(rng, 20000)
        v = rng.normal(size=(18000, 3))
        store[:18000, :3] = (v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0, 1, (18000, 1)) + [7, -3, 0.5]).astype(F)
        q = np.concatenate([cloud(rng, 100, 65.0), store[rng.integers(0, 18000, 100)]])
        q[100:, :3] += F(0.01)
    elif shape == "identical":
        store = np.tile(np.array([[1.5, -2.5, 0.25, 0]], F), (3000, 1))
        q = np.concatenate([cloud(rng, 64, 10.0), store[:1]])
    elif shape == "lattice":  # 20 x 20 x 5 integer lattice: queries on nodes and cell centres tie
        g = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
        store = np.zeros((len(g), 4), F)
        store[:, :3] = g[rng.permutation(len(g))]
        q = np.zeros((200, 4), F)
        q[:100, :3] = g[rng.integers(0, len(g), 100)]
        q[100:, :3] = g[rng.integers(0, len(g), 100)] + 0.5
    elif shape == "flat":
        store = cloud(rng, 5000)
        store[:, 2] = F(1.25)
        q = cloud(rng, 130, 65.0)
    else:
        store = np.zeros((5000, 4), F)
        store[:, :3] = np.outer(rng.uniform(-50, 50, 5000), [1.0, 2.0, 0.0]).astype(F)
        q = cloud(rng, 130, 65.0)
    store[:, 3] = np.arange(len(store))
    t = trees()
    t.Build(store)
    for k, md in ((1, np.inf), (20, np.inf), (32, 1.5)):
        _, _, i, f = check(t, store, q, k, md)
        if shape == "identical" and np.isinf(md):
            assert (i == np.arange(k)).all()


@pytest.mark.gpu
def test_non_finite_points_and_queries(trees):
    rng = np.random.default_rng(6)
    store = cloud(rng, 3000)
    store[5, 0] = np.nan
    store[17, 1] = np.inf
    store[100:140, 2] = -np.inf
    store[2999, :3] = np.nan
    q = cloud(rng, 70, 65.0)
    q[3, 0] = np.nan
    q[64, 2] = np.inf
    q[10, :3] = [0, 0, 0]
    t = trees()
    t.Build(store)
    for k in (1, 20):
        _, _, i, f = check(t, store, q, k)
        assert f[3] == 0 and f[64] == 0 and not np.isin(i, [5, 17, 2999]).any()
    bad = np.full((40, 4), np.nan, F)
    t.Build(bad)
    assert (check(t, bad, q, 5)[3] == 0).all()


@pytest.mark.gpu
def test_overflowing_distance(trees):
    t = trees()
    far = np.array([[3e38, 0, 0, 1], [1, 0, 0, 2]], F)
    q = np.array([[-3e38, 0, 0], [0, 0, 0]], F)
    t.Build(far)
    _, d, i, f = check(t, far, q, 2)
    assert f[0] == 2 and np.isinf(d[0]).all() and i[0].tolist() == [0, 1]
    assert check(t, far, q, 2, 1e150)[3].tolist() == [0, 1]
    wide = np.array([[3e38, 0, 0, 1], [-3e38, 0, 0, 2], [0, 1, 0, 3]], F)  # the box's extent overflows
    t.Build(wide)
    check(t, wide, q, 3)


@pytest.mark.gpu
def test_max_dist_edges(trees):
    t = trees()
    store = np.array([[3, 4, 0, 7], [0, 0, 12, 8], [100, 0, 0, 9]], F)
    q = np.zeros((1, 3), F)
    t.Build(store)
    assert check(t, store, q, 2, 5.0)[3][0] == 1
    assert check(t, store, q, 2, float(np.nextafter(5.0, 0.0)))[3][0] == 0
    assert check(t, store, q, 3, -13.0)[3][0] == 2
    assert check(t, store, q, 3, float("nan"))[3][0] == 0
    rng = np.random.default_rng(8)
    store = cloud(rng, 4000)
    t.Build(store)
    qs = cloud(rng, 100, 55.0)
    for md in (-2.0, float("nan"), 0.0, 1e-3, 1e30):
        check(t, store, qs, 8, md)


# ------------------------------------------------------------------------------------ the index's life
def stats(t):
    s = t.index_stats()
    return s["indexed"], s["tail"], s["builds"]


@pytest.mark.gpu
def test_edit_sequence(trees):
    rng = np.random.default_rng(9)
    store = cloud(rng, 3000)
    q = cloud(rng, 130, 60.0)
    t = trees(0.5)
    t.Build(store)
    assert stats(t) == (0, 3000, 0)
    same(t.nearest_search(q, 5), twin.nearest_search(store, q, 5))
    assert stats(t) == (3000, 0, 1)
    add = cloud(rng, 100, 50.0, 3000)
    t.Add_Points(add)
    store = np.concatenate([store, add])
    qa = np.concatenate([add, q])
    want = twin.nearest_search(store, qa, 5)
    got = t.nearest_search(qa, 5)
    same(got, want)
    assert stats(t) == (3000, 100, 1)
    assert (got[1][:100, 0] == 0).all() and (got[2][:100, 0] >= 3000).all()
    t.index_build()
    assert stats(t) == (3100, 0, 2)
    same(t.nearest_search(qa, 5), want)
    t.index_build()  # nothing to do
    assert stats(t) == (3100, 0, 2)
    boxes = np.array([[-20, -20, -10, 0, 5, 10], [10, 10, -10, 30, 30, 10]], F)
    store, gone = edit.delete_boxes(store, boxes)
    assert t.Delete_Point_Boxes(boxes) == gone and gone > 100
    assert stats(t) == (0, len(store), 2)
    _, _, i, _ = check(t, store, qa, 20, paths=(0, BRUTE))
    assert i.max() < len(store) and stats(t) == (len(store), 0, 3)
    arr = cloud(rng, 300, 50.0, 5000)
    store, cnt = edit.add_points_downsample(store, arr, 0.5)
    assert t.Add_Points(arr, True) == cnt
    assert stats(t)[0] == 0
    check(t, store, qa, 5, paths=(0, BRUTE))
    assert stats(t) == (len(store), 0, 4)
    small = cloud(rng, 1500)
    t.Build(small)
    assert stats(t) == (0, 1500, 4)
    check(t, small, qa, 5, paths=(0, BRUTE))
    assert stats(t) == (1500, 0, 5)


@pytest.mark.gpu
def test_tail_limit_rebuilds(trees):
    rng = np.random.default_rng(10)
    store = cloud(rng, 3000)
    q = cloud(rng, 70, 60.0)
    t = trees()
    t.Build(store)
    t.index_build()
    limit = t.index_stats()["tail_limit"]
    assert limit >= 1
    add = cloud(rng, limit, 50.0, 3000)
    t.Add_Points(add)
    store = np.concatenate([store, add])
    check(t, store, q, 5, paths=(0,))
    assert stats(t) == (3000, limit, 1)  # at the limit: still swept
    one = cloud(rng, 1, 50.0, len(store))
    t.Add_Points(one)
    store = np.concatenate([store, one])
    check(t, store, q, 5, paths=(0,))
    assert stats(t) == (len(store), 0, 2)  # past it: rebuilt


@pytest.mark.gpu
def test_growth_past_the_capacity(trees):
    rng = np.random.default_rng(11)
    store = cloud(rng, 65530)
    q = cloud(rng, 70, 60.0)
    t = trees()
    t.Build(store)
    check(t, store, q, 5, paths=(0,))
    before = t.points_device()[0]
    add = cloud(rng, 100, 50.0, 65530)
    t.Add_Points(add)  # crosses the store's first capacity of 65,536: it moves
    store = np.concatenate([store, add])
    assert t.points_device()[0] != before
    qa = np.concatenate([add[:20], q])
    check(t, store, qa, 5, paths=(0, BRUTE))
    assert stats(t)[:2] == (65630, 0)


@pytest.mark.gpu
def test_empty_map_and_no_queries(trees):
    t = trees()
    q = np.zeros((3, 3), F)
    for flags in PATHS:
        p, d, i, f = t.nearest_search(q, 4, flags=flags)
        assert (f == 0).all() and (i == -1).all() and np.isinf(d).all() and (p == 0).all()
    t.index_build()
    assert stats(t) == (0, 0, 0)
    t.Build(np.ones((10, 4), F))
    p, d, i, f = t.nearest_search(np.zeros((0, 3), F), 4)
    assert p.shape == (0, 4, 4) and f.shape == (0,)
    pts, dist = t.Nearest_Search([1, 1, 1], 3, 0.5)
    assert pts.shape == (3, 4) and dist.tolist() == [0, 0, 0]
    pts, dist = t.Nearest_Search([5, 5, 5], 3, 0.5)
    assert pts.shape == (0, 4) and dist.shape == (0,)


# ----------------------------------------------------------------------------- the device variant
@pytest.mark.gpu
def test_device_variant_on_a_stream(trees):
    import torch

    rng = np.random.default_rng(12)
    store = cloud(rng, 30000)
    q = cloud(rng, 300, 60.0)
    t = trees()
    t.Build(store)
    k, guard = 5, 7
    want = t.nearest_search(q, k, 6.0)
    same(want, twin.nearest_search(store, q, k, 6.0))
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    for flags in (0, BRUTE):
        dq = torch.from_numpy(q).to(dev)
        dp = torch.full(((len(q) + guard) * k, 4), -7.0, device=dev)
        dd = torch.full(((len(q) + guard) * k,), -7.0, device=dev)
        di = torch.full(((len(q) + guard) * k,), -7, dtype=torch.int32, device=dev)
        df = torch.full((len(q) + guard,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t.nearest_search_device(dq.data_ptr(), len(q), k, 6.0, dp.data_ptr(), dd.data_ptr(), di.data_ptr(),
                                    df.data_ptr(), stream=stream.cuda_stream, flags=flags)
        stream.synchronize()
        n = len(q) * k
        got = (dp[:n].cpu().numpy().reshape(len(q), k, 4), dd[:n].cpu().numpy().reshape(len(q), k),
               di[:n].cpu().numpy().reshape(len(q), k), df[:len(q)].cpu().numpy())
        same(got, want)
        assert (dp[n:] == -7).all() and (dd[n:] == -7).all() and (di[n:] == -7).all() and (df[len(q):] == -7).all()
    # outputs are optional
    df = torch.zeros(len(q), dtype=torch.int32, device=dev)
    t.nearest_search_device(dq.data_ptr(), len(q), k, 6.0, d_found=df.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(df.cpu().numpy(), want[3])
    ms, calls = t.time_ms()
    assert calls >= 4 and ms > 0


# ------------------------------------------------------------------------------------------ errors
@pytest.mark.gpu
def test_errors(trees, gpu_ctx):
    import icp4r
    from icp4r.mapstore import KD_TREE

    L = icp4r.load()
    t = trees()
    t.Build(np.ones((10, 4), F))
    q = np.zeros((2, 4), F)
    out = np.zeros(64, np.int32)

    def call(nq=2, stride=16, k=2, flags=0, qp=q.ctypes.data, h=None):
        return L.icp4r_map_nearest_search(h or t.handle, qp, nq, stride, k, 1.0, flags, None, None, None, out.ctypes.data)

    assert call() == icp4r.OK
    for bad in (dict(flags=4), dict(flags=3), dict(flags=-1), dict(nq=-1), dict(qp=None), dict(stride=8), dict(k=0),
                dict(k=33), dict(k=-1)):
        assert call(**bad) == icp4r.E_INVALID, bad
    assert call(nq=0, qp=None) == icp4r.OK
    assert L.icp4r_map_nearest_search_device(t.handle, None, 2, 2, 1.0, 0, None, None, None, None, None) == icp4r.E_INVALID
    assert L.icp4r_map_nearest_search_device(t.handle, None, 0, 2, 1.0, 0, None, None, None, None, None) == icp4r.OK
    assert L.icp4r_map_index_build(None) == icp4r.E_INVALID
    with pytest.raises(icp4r.ICP4RError):
        t.nearest_search(q, 40)
    # a detached map answers every entry with ICP4R_E_INVALID
    ctx = icp4r.Context(0)
    d = KD_TREE(ctx=ctx)
    d.Build(np.ones((10, 4), F))
    ctx.close()
    try:
        assert call(h=d.handle) == icp4r.E_INVALID
        assert L.icp4r_map_index_build(d.handle) == icp4r.E_INVALID
        assert L.icp4r_map_index_stats(d.handle, None, None, None, None) == icp4r.E_INVALID
    finally:
        d.close()


# --------------------------------------------------------------------- the reference's own answers
@pytest.mark.gpu
@pytest.mark.parametrize("case", "abc")
def test_reference_fixture_through_the_store(trees, case):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ikd_nearest.npz"))
    store, queries = g[f"{case}_store"], g[f"{case}_queries"]
    t = trees()
    t.Build(store)
    for s, (k, md) in enumerate(zip(g["searches_k"], g["searches_max_dist"])):
        for flags in (INDEX, BRUTE):
            _, d, i, f = t.nearest_search(queries, int(k), float(md), flags=flags)
            assert np.array_equal(f, g[f"{case}_found_{s}"])
            assert np.array_equal(d.view(np.uint32), g[f"{case}_dist_{s}"].view(np.uint32))
            untied = np.array([not twin.tied(store, q, int(k)) for q in queries])
            assert np.array_equal(i[untied], g[f"{case}_index_{s}"][untied])


@pytest.mark.gpu
def test_reference_call_text_runs(tmp_path):
    """tests/cpp/nearest_callsite.cpp (the reference's call text over ikd_compat.hpp) == the twin."""
    exe = tmp_path / "nearest_callsite"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{CPP}/pcl18", f"-I{ROOT}/include", "-o", str(exe),
                        os.path.join(CPP, "nearest_callsite.cpp"), f"-L{LIB}", "-licp4r", f"-Wl,-rpath,{LIB}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    rng = np.random.default_rng(13)
    built, added, q = cloud(rng, 2000), cloud(rng, 300, 50.0, 2000), cloud(rng, 40, 60.0)
    store = np.concatenate([built, added])
    for k, md in ((5, -1.0), (20, 4.0)):
        case = tmp_path / f"case_{k}.txt"
        with open(case, "w") as f:
            f.write(f"{len(built)} {len(added)} {len(q)} {k} {md!r}\n")
            for p in np.concatenate([store, q]):
                f.write(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n")
        r = subprocess.run([str(exe), str(case)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        _, wd, wi, wf = twin.nearest_search(store, q, k, np.inf if md < 0 else md)
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(q)
        for j, line in enumerate(lines):
            items = line.split(":")[1].split()
            assert len(items) == wf[j]
            assert [int(x.split("/")[0]) for x in items] == wi[j, :wf[j]].tolist()
            assert [int(x.split("/")[1], 16) for x in items] == wd[j, :wf[j]].view(np.uint32).tolist()
