"""The store's map maintenance on the device — Delete_Point_Boxes, Box_Search, Radius_Search and the
downsampling Add_Points(.., True) — held to tests/map_edit_twin.py as arrays: count, order and values
(the intensity carries the point's index), and through it to the outputs recorded from the reference's
ikd-Tree (tests/golden/ikd_edit.npz).  Every tree is closed by the `trees` fixture.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_edit_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ikd_edit.npz")
F = np.float32
ALL = np.array([-np.inf] * 3 + [np.inf] * 3, F)
BLOCK = 4096  # points per workgroup of the compaction
SIZES = (0, 1, 255, 256, 4095, 4096, 4097, 3 * 4096 + 5)
PATTERNS = ("all", "none", "alternating", "block_first", "block_last")


@pytest.fixture(scope="module")
def fx():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def trees(gpu_ctx):
    """trees(ds) -> a KD_TREE with that downsample box on the session's context, closed at teardown."""
    from icp4r.mapstore import KD_TREE

    made = []

    def make(ds=0.5):
        t = KD_TREE(0.5, 0.6, ds, ctx=gpu_ctx)
        made.append(t)
        return t

    yield make
    for t in made:
        t.close()


def _indexed(xyz, first=0):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), F)
    out[:, :3] = xyz
    out[:, 3] = np.arange(first, first + len(xyz), dtype=F)
    return out


def _same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------- 1. reference fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_reference_fixture(trees, fx, case):
    store, add, ds = _indexed(fx[f"{case}_build"]), None, float(fx[f"{case}_ds"])
    add = _indexed(fx[f"{case}_add"], len(store))
    tree = trees(ds)
    tree.Build(store)
    counter = tree.Add_Points(add, True)
    s_tw, c_tw = tw.add_points_downsample(store, add, ds)
    assert counter == int(fx[f"{case}_counter"]) == c_tw
    s = tree.Box_Search(ALL)
    assert tree.size() == len(s_tw) and _same(s, s_tw)
    assert np.array_equal(s[:, 3].astype(np.int32), fx[f"{case}_survivors"])
    r = tree.Radius_Search(fx["center"], float(fx["radius"]))
    assert _same(r, tw.radius_search(s_tw, fx["center"], fx["radius"]))
    assert np.array_equal(r[:, 3].astype(np.int32), fx[f"{case}_radius"])
    deleted = tree.Delete_Point_Boxes(fx["boxes"])
    left_tw, d_tw = tw.delete_boxes(s_tw, fx["boxes"])
    assert deleted == int(fx[f"{case}_deleted"]) == d_tw
    after = tree.Box_Search(ALL)
    assert tree.size() == len(left_tw) and _same(after, left_tw)
    assert np.array_equal(after[:, 3].astype(np.int32), fx[f"{case}_after_delete"])


# --------------------------------------------------------------------- 2. compaction boundaries
def _mask(n, pattern):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "block_first":
        return i % BLOCK == 0
    return (i % BLOCK == BLOCK - 1) | (i == n - 1)


# The search box [0, 1) x [0, 1)^2 and the radius query (centre (0, .25, .25), r = .75) both keep
# x in {0.0, 0.75} — the box's min face, and d^2 = r^2 exactly — and drop x in {1.0, 2.0}: the box's
# max face and beyond.  y = z = 0.25 sits on the delete boxes' min faces.
BOX = np.array([0, 0, 0, 1, 1, 1], F)
CENTER, RADIUS = np.array([0, 0.25, 0.25], F), 0.75
# Deleting removes x in {1.0, 2.0}: 1.0 lies on the min face of the first two boxes and in both, 2.0 in
# the second and third; x = 0.0 lies on the fourth box's max face and stays.
DEL_BOXES = np.array([[1.0, 0.25, 0.25, 1.5, 1, 1], [1.0, 0.25, 0.25, 3.0, 1, 1], [1.2, 0, 0, 2.5, 1, 1],
                      [-2.0, 0, 0, 0.0, 1, 1]], F)


def _pattern_points(n, pattern):
    keep = _mask(n, pattern)
    even = np.arange(n) % 4 < 2
    x = np.where(keep, np.where(even, 0.0, 0.75), np.where(even, 1.0, 2.0))
    return _indexed(np.stack([x, np.full(n, 0.25), np.full(n, 0.25)], 1)), keep


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_compaction_boundaries(trees, n):
    tree = trees()
    for pattern in PATTERNS:
        pts, keep = _pattern_points(n, pattern)
        tree.Build(pts)
        want = pts[keep]
        assert _same(tw.box_search(pts, BOX), want) and _same(tw.radius_search(pts, CENTER, RADIUS), want)
        assert _same(tree.Box_Search(BOX), want), pattern
        assert _same(tree.Radius_Search(CENTER, RADIUS), want), pattern
        assert tree.Delete_Point_Boxes(np.zeros((0, 6), F)) == 0 and tree.size() == n  # nb = 0
        left, deleted = tw.delete_boxes(pts, DEL_BOXES)
        assert _same(left, want) and deleted == n - int(keep.sum())
        assert tree.Delete_Point_Boxes(DEL_BOXES) == deleted, pattern
        assert tree.size() == len(want) and _same(tree.Box_Search(ALL), want), pattern
        assert tree.Delete_Point_Boxes(DEL_BOXES) == 0  # nothing left inside


@pytest.mark.gpu
def test_nan_is_never_found_or_deleted(trees):
    tree = trees()
    pts = _indexed([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, np.nan], [0.25, 0.5, 0.5]])
    tree.Build(pts)
    assert _same(tree.Box_Search(ALL), pts[[0, 3]])
    assert _same(tree.Radius_Search([0.5, 0.5, 0.5], 10.0), pts[[0, 3]])
    assert len(tree.Box_Search([0, 0, 0, np.nan, 1, 1])) == 0
    assert tree.Delete_Point_Boxes(ALL) == 2 and tree.size() == 2


# ------------------------------------------------------------------------ 3. downsampled insert
def _check_ds(tree, store, arr, ds):
    store = np.ascontiguousarray(store, F).reshape(-1, 4)
    arr = np.ascontiguousarray(arr, F).reshape(-1, 4)
    tree.set_downsample_param(ds)
    tree.Build(store)
    counter = tree.Add_Points(arr, True)
    want, c_tw = tw.add_points_downsample(store, arr, ds)
    got = tree.Box_Search(ALL)
    assert counter == c_tw, (counter, c_tw)
    assert tree.size() == len(want) and _same(got, want)
    return counter


def _one_cell(ds, radii_stored, radii_arr, rng):
    """Points of the cell [0, ds)^3 at the given distances from its centre, along seeded axis directions
    (+-x, +-y, +-z): radii that are multiples of ds / 4096 make the float distances exact, so equal
    radii tie exactly."""
    def place(radii):
        axis = rng.integers(0, 3, len(radii))
        sign = rng.choice([-1.0, 1.0], len(radii))
        p = np.full((len(radii), 3), ds / 2)
        p[np.arange(len(radii)), axis] += sign * np.asarray(radii)
        return p

    store = _indexed(place(radii_stored))
    return store, _indexed(place(radii_arr), len(store))


@pytest.mark.gpu
@pytest.mark.parametrize("ds", [0.5, 0.25])
@pytest.mark.parametrize("order", ["decreasing", "increasing", "shuffled"])
def test_downsample_one_crowded_cell(trees, ds, order):
    rng = np.random.default_rng(11)
    u = ds / 4096
    # stored radii: beyond every arrival's when the arrivals come nearer and nearer, so that each one
    # replaces the holder; among the arrivals' radii otherwise
    rs = u * rng.permutation(np.arange(1850, 2040) if order == "decreasing" else np.arange(700, 2000))[:70]
    if order == "shuffled":  # exact ties (few distinct radii, some equal to stored ones) and exact duplicates
        ra = u * rng.choice(np.concatenate([np.arange(100, 140), rs[:5] / u]), 300)
        store, arr = _one_cell(ds, rs, ra, rng)
        arr[150:200, :3] = arr[100:150, :3]
    else:
        ra = u * (np.arange(300) * 6 + 10.0)  # some below, some above the stored minimum
        ra = ra[::-1] if order == "decreasing" else ra
        store, arr = _one_cell(ds, rs, ra, rng)
    d = tw.calc_dist(arr, np.full(3, ds / 2, F))
    if order == "decreasing":
        assert (np.diff(d) < 0).all()
    elif order == "increasing":
        assert (np.diff(d) > 0).all()
    else:
        assert len(np.unique(d)) < 60
    counter = _check_ds(trees(ds), store, arr, ds)
    if order == "decreasing":
        assert counter == 300  # every arrival is nearer than the holder before it
    # the same arrivals into an empty store
    arr0 = arr.copy()
    arr0[:, 3] = np.arange(len(arr0), dtype=F)
    _check_ds(trees(ds), np.zeros((0, 4), F), arr0, ds)


@pytest.mark.gpu
@pytest.mark.parametrize("ds", [0.5, 0.25])
def test_downsample_sizes_and_cells(trees, ds):
    rng = np.random.default_rng(5)
    tree = trees(ds)
    half = 10 * ds  # 20^3 = 8,000 cells over negative and positive coordinates
    store = _indexed(rng.uniform(-half, half, (3000, 3)))
    assert _check_ds(tree, store, np.zeros((0, 4), F), ds) == 0  # zero arrivals
    for na in (257, 4097, 8000):
        arr = _indexed(rng.uniform(-half, half, (na, 3)), len(store))
        if na == 8000:
            cells = np.unique(np.floor(arr[:, :3] / F(ds)), axis=0)
            assert 4500 < len(cells) < 5500  # the table probes: ~5,000 cells in 16,384 slots
        _check_ds(tree, store, arr, ds)
        arr[:, 3] -= len(store)
        _check_ds(tree, np.zeros((0, 4), F), arr, ds)  # an empty store


@pytest.mark.gpu
@pytest.mark.parametrize("ds", [0.5, 0.25])
def test_downsample_handmade(trees, ds):
    tree = trees(ds)
    c = ds / 2
    # cells that differ on one axis only, one stored point and two arrivals each (one nearer, one farther)
    cells = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], float) * ds
    store = _indexed(cells + c + 0.2 * ds)
    arr = _indexed(np.concatenate([cells + c + 0.1 * ds, cells + c - 0.3 * ds]), len(store))
    assert _check_ds(tree, store, arr, ds) == 7
    # -0.0 and 0.0 are one cell; the stored point at -0.0 is the farther one
    store = _indexed([[-0.0, c, c], [c, -0.0, 0.0]])
    arr = _indexed([[0.0, c, c], [0.0, c, c + ds / 8], [c, 0.0, -0.0], [c + ds / 8, c, c]], 2)
    _check_ds(tree, store, arr, ds)
    # same_point: an arrival 4e-7 beside a stored, nearer point is counted and the stored values stay
    s = np.array([[c + 0.05, c, c]], F)
    a = s + F(4e-7)
    assert 0 < float(a[0, 0] - s[0, 0]) < 1e-6 and tw.calc_dist(a, np.full(3, c, F))[0] > tw.calc_dist(s, np.full(3, c, F))[0]
    store, arr = _indexed(s), _indexed(np.concatenate([a, s + F(0.01)]), 1)
    assert _check_ds(tree, store, arr, ds) == 1 and _same(tree.Box_Search(ALL), store)
    # stored points of a touched cell at exactly equal distance: the lowest index stays
    store = _indexed([[c + ds / 8, c, c], [c - ds / 8, c, c], [c, c + ds / 8, c], [5 * ds + c, c, c]])
    arr = _indexed([[c + ds / 4, c, c]], 4)
    assert _check_ds(tree, store, arr, ds) == 1 and _same(tree.Box_Search(ALL), store[[0, 3]])


# -------------------------------------------------------------------- 4. carried state and growth
@pytest.mark.gpu
def test_carried_state_and_growth(trees, oracle_mod):
    from helpers import sector_edge_filter

    rng = np.random.default_rng(77)
    ds, center, heading = 0.5, [3.0, -2.0, 0.0], 25.0
    q = [(center, heading)]

    def cloud(n, extent=150.0):
        raw = np.concatenate([rng.uniform(-extent, extent, (n + 40, 2)), rng.uniform(-3, 3, (n + 40, 1))], 1).astype(F)
        kept, removed = sector_edge_filter(raw, q)  # asserts at most 1e-4 of the cloud removed
        assert len(kept) >= n
        return kept[:n]

    build = cloud(65_000)
    near = build[rng.integers(0, len(build), 1000)] + rng.uniform(-0.2, 0.2, (1000, 3)).astype(F)
    adds = [np.concatenate([sector_edge_filter(near, q)[0], cloud(1000)]), cloud(1500, 40.0), cloud(700, 60.0)]
    first = [len(build)]
    for a in adds:
        first.append(first[-1] + len(a))
    build = _indexed(build)
    adds = [_indexed(a, f) for a, f in zip(adds, first)]
    assert first[-1] < 2 ** 24  # the index in the intensity is exact

    tree = trees(ds)
    tree.Build(build)
    c = tree.Add_Points(adds[0], True)
    s, c_tw = tw.add_points_downsample(build, adds[0], ds)
    assert c == c_tw and len(s) > 65_536  # past the store's first capacity
    assert _same(tree.Box_Search(ALL), s)
    boxes = np.array([[-20, -30, -5, 0, -10, 5], [-10, -20, -1, 10, 0, 1]], F)
    d = tree.Delete_Point_Boxes(boxes)
    s, d_tw = tw.delete_boxes(s, boxes)
    assert d == d_tw > 0 and _same(tree.Box_Search(ALL), s)
    c = tree.Add_Points(adds[1], True)
    s, c_tw = tw.add_points_downsample(s, adds[1], ds)
    assert c == c_tw and _same(tree.Box_Search(ALL), s)
    assert tree.Add_Points(adds[2], False) == 0
    s = np.concatenate([s, adds[2]])
    assert tree.size() == len(s) and _same(tree.Box_Search(ALL), s)
    r = tree.Radius_Search(center, 80.0)
    assert len(r) > 1000 and _same(r, tw.radius_search(s, center, 80.0))
    ref = oracle_mod.sector_search(s, center, 80.0, heading)
    assert len(ref) > 1000 and _same(tree.Sector_Search(center, 80.0, heading), s[ref])


# ------------------------------------------------------------------------------------ 5. errors
@pytest.mark.gpu
def test_edit_errors(trees):
    import icp4r

    tree = trees()
    lib, h = icp4r.load(), tree.handle
    pts = _indexed(np.random.default_rng(3).uniform(0, 1, (300, 3)))
    tree.Build(pts)
    k, inv = C.c_int64(-5), icp4r.E_INVALID
    box, out = ALL.copy(), np.zeros((400, 4), F)
    p = lambda a: a.ctypes.data  # noqa: E731
    # NULL arguments
    assert lib.icp4r_map_delete_boxes(None, p(box), 1, C.byref(k)) == inv
    assert lib.icp4r_map_delete_boxes(h, None, 1, C.byref(k)) == inv
    assert lib.icp4r_map_delete_boxes(h, p(box), 1, None) == inv
    assert lib.icp4r_map_box_search(None, p(box), p(out), 400, C.byref(k)) == inv
    assert lib.icp4r_map_box_search(h, None, p(out), 400, C.byref(k)) == inv
    assert lib.icp4r_map_box_search(h, p(box), None, 400, C.byref(k)) == inv
    assert lib.icp4r_map_box_search(h, p(box), p(out), 400, None) == inv
    assert lib.icp4r_map_radius_search(None, p(box), 1.0, p(out), 400, C.byref(k)) == inv
    assert lib.icp4r_map_radius_search(h, None, 1.0, p(out), 400, C.byref(k)) == inv
    assert lib.icp4r_map_radius_search(h, p(box), 1.0, p(out), 400, None) == inv
    assert lib.icp4r_map_box_search_device(h, p(box), None, None, None) == inv
    assert lib.icp4r_map_radius_search_device(h, p(box), 1.0, None, None, None) == inv
    assert lib.icp4r_map_add_points_downsample(None, p(pts), 300, 16, 0.5, C.byref(k)) == inv
    assert lib.icp4r_map_add_points_downsample(h, None, 300, 16, 0.5, C.byref(k)) == inv
    assert lib.icp4r_map_add_points_downsample(h, p(pts), 300, 16, 0.5, None) == inv
    # box_length 0, negative, NaN, infinite; a negative or NaN radius
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        assert lib.icp4r_map_add_points_downsample(h, p(pts), 300, 16, bad, C.byref(k)) == inv
    for bad in (-1.0, float("nan")):
        assert lib.icp4r_map_radius_search(h, p(box), bad, p(out), 400, C.byref(k)) == inv
    assert lib.icp4r_map_add_points(h, p(pts), 300, 16, 1) == inv  # carries no box length
    assert lib.icp4r_map_delete_boxes(h, None, 0, C.byref(k)) == icp4r.OK and k.value == 0  # nb = 0
    assert tree.size() == 300 and _same(tree.Box_Search(ALL), pts)  # none of the above changed the store
    # out_cap one short: E_TOO_LARGE, *out_n set, nothing written
    guard = np.full((300 - 1 + 16, 4), F(-12345.5))
    for call in (lambda o: lib.icp4r_map_box_search(h, p(box), p(o), 299, C.byref(k)),
                 lambda o: lib.icp4r_map_radius_search(h, p(pts[0]), 10.0, p(o), 299, C.byref(k))):
        o = guard.copy()
        k.value = -5
        assert call(o) == icp4r.E_TOO_LARGE and k.value == 300
        assert o.tobytes() == guard.tobytes()
    assert lib.icp4r_map_box_search(h, p(box), p(out), 300, C.byref(k)) == icp4r.OK and k.value == 300


# --------------------------------------------------------------------------- 6. device variants
@pytest.mark.gpu
def test_device_variants_on_a_caller_stream(trees):
    import torch

    tree = trees()
    pts = _indexed(np.random.default_rng(9).uniform(-50, 50, (2 * BLOCK + 77, 3)))
    tree.Build(pts)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    box, center, radius = np.array([-20, -30, -50, 25, 10, 50], F), [5.0, -3.0, 1.0], 40.0
    hosts = [tree.Box_Search(box), tree.Radius_Search(center, radius)]
    assert all(100 < len(x) < len(pts) for x in hosts)
    for host, launch in zip(hosts, (lambda o, c: tree.box_search_device(box, o, c, stream=stream.cuda_stream),
                                    lambda o, c: tree.radius_search_device(center, radius, o, c,
                                                                           stream=stream.cuda_stream))):
        d_out = torch.full((len(pts) + 8, 4), -7.0, dtype=torch.float32, device=dev)
        d_cnt = torch.full((3,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        launch(d_out.data_ptr(), d_cnt[1:].data_ptr())
        stream.synchronize()
        cnt, out = d_cnt.cpu().numpy(), d_out.cpu().numpy()
        assert cnt.tolist() == [-1, len(host), -1]
        assert out[: len(host)].tobytes() == host.tobytes()
        assert (out[len(host):] == -7.0).all()


# ------------------------------------------------------------------------------- 7. C++ facade
@pytest.mark.gpu
@pytest.mark.parametrize("pcl18", [False, True])
def test_ikd_facade_edit_callsite(fx, tmp_path, pcl18):
    """tests/cpp/map_edit_callsite.cpp drives BoxPointType, Add_Points(.., true), Box_Search, Radius_Search
    and Delete_Point_Boxes through include/icp4r/ikd_compat.hpp on fixture case a, with the stand-in
    types and with the PCL-1.8-shaped include tree; the printed counter and index lists are the fixture's."""
    libdir = os.path.join(ROOT, "icp-4dradar_amd", "icp4r", "_lib")
    exe = str(tmp_path / "map_edit_callsite")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"]
    if pcl18:
        cmd.append("-I" + os.path.join(ROOT, "tests", "cpp", "pcl18"))
    cmd += ["-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "map_edit_callsite.cpp"),
            "-L" + libdir, "-licp4r", "-Wl,-rpath," + libdir]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    inp = tmp_path / "case_a.txt"
    build, add, boxes = fx["a_build"], fx["a_add"], np.asarray(fx["boxes"], F).reshape(-1, 6)
    with open(inp, "w") as f:
        f.write(f"{float(fx['a_ds'])!r} {len(build)} {len(add)} {len(boxes)}\n")
        f.write(" ".join(repr(float(v)) for v in np.asarray(fx["center"], F).reshape(-1)[:3]))
        f.write(f" {float(fx['radius'])!r}\n")
        for row in np.concatenate([build, add]).astype(F):
            f.write(" ".join(repr(float(v)) for v in row[:3]) + "\n")
        for row in boxes:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = dict(ln.split(":", 1) for ln in r.stdout.strip().split("\n"))
    ints = lambda key: np.array(out[key].split(), np.int64)  # noqa: E731
    assert int(out["counter"]) == int(fx["a_counter"]) and int(out["deleted"]) == int(fx["a_deleted"])
    assert np.array_equal(ints("survivors"), fx["a_survivors"])
    assert np.array_equal(ints("radius"), fx["a_radius"])
    assert np.array_equal(ints("after_delete"), fx["a_after_delete"])
    assert int(out["size"]) == len(fx["a_after_delete"])
