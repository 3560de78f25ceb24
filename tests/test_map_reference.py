"""The scan-to-map sector path held to the reference's own ikd-Tree.

tests/golden/ikd_sector.npz (make_ikd_sector_golden.md) holds what the real tree answered: a table of its
private calc_heading / calc_dist bits, two runs of the node's Build / Add_Points(.., false) / Sector_Search
loop, and two cases in which it returns lazily deleted points ("ghosts").  The CPU tests hold the oracle's
restatement (oracle/map_oracle.c) to that record; the GPU tests hold the store to it.  Where the reference
binaries are built (oracle/_ref/, `make -C oracle ref`) the live tests run the real tree next to the store on
the shapes where the store's kernels can go wrong, and the two map call-site programs against both headers.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import helpers
import ikd_ref
import make_ikd_sector_golden as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ikd_sector.npz")
EDIT_GOLDEN = os.path.join(ROOT, "tests", "golden", "ikd_edit.npz")
F = np.float32
RADIUS = 80.0
ALL = np.array([-np.inf] * 3 + [np.inf] * 3, F)
LOOP_SIZES = {"L1": (600,) + (300,) * 5, "L2": (2000,) + (600,) * 6}
SEC_BLOCK = 4096  # kSecBlock: points per workgroup of the sector filter
LIVE_QUERIES = helpers.MAP_QUERIES + (([10.5, -4.0, 1.0], 179.5),)
# The call-site programs' poses (x, y, yaw = heading, degrees): no point of the golden scans lies in a sector
# edge band for them (test_callsite_pose_keeps_clear_of_the_edges); the second one looks back along -y, where
# the dh > 300 branch keeps points.
POSES = ((5.0, -3.0, 45.0), (5.0, -3.0, 177.0))
SCAN_PAIRS = {"c1": ("c1_pair0_2k_tgt.bin", "c1_pair0_2k_src.bin"), "c2": ("c2_pair1_8k_tgt.bin", "c2_pair1_8k_src.bin")}

needs_ref = pytest.mark.skipif(not ikd_ref.available(), reason="oracle/_ref/ikd_ref is not built (no reference tree)")


@pytest.fixture(scope="module")
def fx():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _indexed(xyz, first=0):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    out = np.zeros((len(xyz), 4), F)
    out[:, :3] = xyz
    out[:, 3] = np.arange(first, first + len(xyz), dtype=F)
    return out


def _loop(fx, name):
    """-> (all points (n, 4) with the index in the intensity, frame offsets, [(centre, heading, kept, size)])."""
    off, ko = fx[f"{name}_frame_off"], fx[f"{name}_kept_off"]
    pts = _indexed(fx[f"{name}_frames"])
    frames = [(fx[f"{name}_centers"][k], float(fx[f"{name}_headings"][k]), fx[f"{name}_kept"][ko[k]:ko[k + 1]],
               int(fx[f"{name}_sizes"][k])) for k in range(len(off) - 2)]
    return pts, off, frames


def _rule(oracle_mod, pts, center, radius, heading):
    return oracle_mod.sector_search(np.ascontiguousarray(pts), center, float(radius), float(heading))


def _ghost_inputs(fx, g):
    """-> (every point ever given to the tree (n, 4), the recorded live indices, the recorded real result)."""
    xyz = fx["G1_points"] if g == "G1" else np.concatenate([fx["G2_build"], fx["G2_add"]])
    return _indexed(xyz), fx[f"{g}_live"], fx[f"{g}_sector"]


# ------------------------------------------------------------------------------------- CPU: the oracle
def test_heading_table_bits(oracle_mod, fx):
    """oracle_calc_heading / oracle_calc_dist give the real tree's bits on every row, NaN in the same rows."""
    L = oracle_mod.lib()
    p, c = np.ascontiguousarray(fx["table_points"], F), np.ascontiguousarray(fx["table_centers"], F)
    h = np.array([L.oracle_calc_heading(p[i].ctypes.data, c[i].ctypes.data) for i in range(len(p))], F)
    d = np.array([L.oracle_calc_dist(p[i].ctypes.data, c[i].ctypes.data) for i in range(len(p))], F)
    for got, bits in ((h, fx["table_heading_bits"]), (d, fx["table_dist_bits"])):
        want = bits.view(F)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        bad = np.nonzero((got.view(np.uint32) != bits) & ~nan)[0]
        assert len(bad) == 0, [(int(i), p[i].tolist(), c[i].tolist(), float(got[i]), float(want[i])) for i in bad[:5]]


def test_heading_table_holds_the_named_rows(fx):
    """The rows the table exists for, re-derived from its inputs and recorded outputs."""
    p, c = fx["table_points"], fx["table_centers"]
    h, d2 = fx["table_heading_bits"].view(F), fx["table_dist_bits"].view(F)
    assert len(p) >= 300 and int(fx["table_named"]) < len(p) // 2  # the rest random
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        dx, dy, dz = (p[:, k] - c[:, k] for k in range(3))
        r = dx / np.sqrt(d2, dtype=F)
    zero, neg = (lambda v: v == 0), np.signbit
    one_in = np.nextafter(F(1), F(0))
    sep = np.maximum(np.abs(dx), np.abs(dy))
    for name, rows in {
        "dy = +0": zero(dy) & ~neg(dy) & ~zero(dx), "dy = -0": zero(dy) & neg(dy) & ~zero(dx),
        "dx = 0": zero(dx) & ~zero(dy), "r = 0 through dz": zero(dx) & zero(dy) & ~zero(dz),
        "r = +1": r == 1, "r = -1": r == -1, "r one ulp inside +1": r == one_in, "r one ulp inside -1": r == -one_in,
        "the centre": zero(dx) & zero(dy) & zero(dz) & np.isnan(h),
        "above the wrap": (dy < 0) & (dx > 0) & (h < -179.9), "below the wrap": (dy < 0) & (dx < 0) & (h > 179.9),
        "denormal separation": (sep > 0) & (sep < np.finfo(F).tiny) & zero(dz), "d2 = inf": np.isinf(d2),
    }.items():
        assert rows.any(), name
    assert np.array_equal(np.isnan(h), np.isnan(r) | np.isinf(r))  # 0/0, x/0 with a denormal x, inf/inf


@pytest.mark.parametrize("name", ["L1", "L2"])
def test_oracle_replays_the_loop(oracle_mod, fx, name):
    """oracle.sector_search over the map as it stood at each frame gives exactly the recorded indices; the
    recorded size() is the number of points inserted.  The dh > 300 branch keeps points beyond the radius."""
    pts, off, frames = _loop(fx, name)
    beyond = 0
    for k, (c, heading, kept, size) in enumerate(frames):
        n = int(off[k + 2])
        assert size == n
        assert np.array_equal(_rule(oracle_mod, pts[:n], c, fx["radius"], heading), kept), (name, k)
        d2 = ((pts[kept, :3].astype(np.float64) - c) ** 2).sum(1)
        beyond += int((d2 > 1.01 * RADIUS ** 2).sum())
        if abs(abs(heading) - 180.0) <= 1.0:
            assert (d2 > 1.01 * RADIUS ** 2).sum() > 0, (name, k)
    assert beyond > 0


@pytest.mark.parametrize("g", ["G1", "G2"])
def test_ghosts_are_deleted_points_behind_the_sector(oracle_mod, fx, g):
    """After a deletion (G1) or a downsampling add (G2) the real tree's Sector_Search = the rule on the live
    points, plus lazily deleted points with |dh| > 300 (the keep test's `|| dh > 300` ignores the flag)."""
    pts, live, real = _ghost_inputs(fx, g)
    c, r, heading = fx["G_center"], float(fx["G_radius"]), float(fx["G_heading"])
    want = live[_rule(oracle_mod, pts[live], c, r, heading)]
    assert np.array_equal(np.intersect1d(real, live), want)
    ghosts = np.setdiff1d(real, live)
    assert len(np.unique(real)) == len(real) and ((ghosts >= 0) & (ghosts < len(pts))).all()
    dh = np.array([abs(oracle_mod.calc_heading(pts[i], c) - heading) for i in ghosts])
    assert (dh > 300).all()
    if g == "G1":
        assert len(ghosts) > 0  # the case exists to show them
        assert int(fx["G1_deleted"]) == len(pts) - len(live)


def _edge_band(pts, queries):
    return gen.in_edge_band(np.asarray(pts, F), queries)


def test_fixture_conditions(fx):
    """Sizes, the generator's removal counts and their cap, the edge-band condition re-checked in double, the
    planted duplicates and centre point, and the file's size."""
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert float(fx["radius"]) == RADIUS
    for name, sizes in LOOP_SIZES.items():
        pts, off, frames = _loop(fx, name)
        assert np.array_equal(np.diff(off), sizes) and len(frames) == len(sizes) - 1
        removed = fx[f"{name}_removed"]
        assert len(removed) == len(sizes) and all(r <= 1e-3 * n for r, n in zip(removed, sizes)), (name, removed)
        queries = [(c, h) for c, h, _, _ in frames]
        assert not _edge_band(pts, queries).any()
        dup = fx[f"{name}_dup"]
        assert len(dup) >= 5 and (dup[:, 1] < dup[:, 0]).all()
        assert np.array_equal(pts[dup[:, 0], :3], pts[dup[:, 1], :3])
        i, q = fx[f"{name}_center_point"]
        assert np.array_equal(pts[i, :3], frames[q][0]) and i < off[q + 1]  # stored before that query's frame
        assert any(abs(abs(h) - 180.0) <= 1.0 for _, h, _, _ in frames)
    gq = [(fx["G_center"], fx["G_heading"])]
    for key, n in (("G1_points", 1000), ("G2_build", 1000), ("G2_add", 1000)):
        assert len(fx[key]) == n and not _edge_band(fx[key], gq).any()  # below the 1500-point rebuild thread
    assert (fx["G1_removed"] <= 1).all() and (fx["G2_removed"] <= 1).all()  # 1e-3 of 1000


def test_reference_binaries_are_built_where_the_reference_is():
    """With the reference tree on this machine the three binaries must exist, so a skipped live test cannot
    go unnoticed here."""
    if not os.path.isdir(ikd_ref.REFERENCE):
        return
    missing = [b for b in ikd_ref.BINARIES if not os.path.isfile(os.path.join(ikd_ref.REF_DIR, b))]
    assert not missing and ikd_ref.available(), missing


def test_ref_target_without_a_reference_leaves_the_binaries_alone(tmp_path):
    """`make -C oracle ref` with REFERENCE at a missing directory: one line, exit 0, oracle/_ref/ untouched."""
    def listing():
        if not os.path.isdir(ikd_ref.REF_DIR):
            return None
        return sorted((f, os.stat(os.path.join(ikd_ref.REF_DIR, f)).st_mtime_ns) for f in os.listdir(ikd_ref.REF_DIR))

    before = listing()
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref", f"REFERENCE={tmp_path / 'absent'}"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.strip().split("\n")) == 1 and "no reference tree" in r.stdout
    assert listing() == before


@needs_ref
def test_fixture_regenerates(fx):
    """The generator's inputs are the committed ones, and the real tree answers its jobs as recorded."""
    inp = gen.make_inputs()
    for k, v in inp.items():
        assert np.asarray(v).dtype == fx[k].dtype and np.array_equal(v, fx[k], equal_nan=True), k
    out = gen.record(fx)
    assert set(inp) | set(out) == set(fx)
    for k, v in out.items():
        assert np.asarray(v).dtype == fx[k].dtype and np.array_equal(v, fx[k]), k


# ------------------------------------------------------------------ CPU: the call-site programs' inputs
def _callsite_world(pair, pose, oracle_mod):
    from icp4r import synth

    a, b = (os.path.join(helpers.GOLDEN_DIR, f) for f in SCAN_PAIRS[pair])
    x, y, yaw = pose
    first, nxt = (synth.records_to_xyzi(synth.read_bin(p)) for p in (a, b))
    co, si = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
    world = oracle_mod.associate_to_map(nxt, np.array([[co, -si, 0], [si, co, 0], [0, 0, 1]]), np.array([x, y, 0.0]))
    return a, b, np.concatenate([first, world])


@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("pair", sorted(SCAN_PAIRS))
def test_callsite_pose_keeps_clear_of_the_edges(oracle_mod, pair, pose):
    _, _, allp = _callsite_world(pair, pose, oracle_mod)
    x, y, yaw = pose
    assert len(allp) >= 4000 and not _edge_band(allp, [([x, y, 0.0], yaw)]).any()


# ---------------------------------------------------------------------------- GPU: the recorded fixture
@pytest.fixture
def trees(gpu_ctx):
    from icp4r.mapstore import KD_TREE

    made = []

    def make(*params):
        t = KD_TREE(*params, ctx=gpu_ctx)
        made.append(t)
        return t

    yield make
    for t in made:
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["L1", "L2"])
def test_store_replays_the_loop(trees, fx, name):
    """The node's loop on the store: per frame the rows are the recorded points, in insertion order."""
    pts, off, frames = _loop(fx, name)
    tree = trees(0.3, 0.6, 0.5)
    tree.Build(pts[: off[1]])
    tree.set_downsample_param(0.5)
    for k, (c, heading, kept, size) in enumerate(frames):
        assert tree.Add_Points(pts[off[k + 1]:off[k + 2]], False) == 0
        got = tree.Sector_Search(c, float(fx["radius"]), heading)
        assert got.shape == (len(kept), 4) and np.array_equal(got, pts[kept]), (name, k)
        assert tree.size() == size


@pytest.mark.gpu
@pytest.mark.parametrize("g", ["G1", "G2"])
def test_store_returns_no_ghosts(trees, oracle_mod, fx, g):
    """After Delete_Point_Boxes (G1) and Add_Points(.., True) (G2) the store holds the recorded live set and
    its Sector_Search is the rule on it: the real tree's recorded result without its ghosts."""
    pts, live, real = _ghost_inputs(fx, g)
    c, r, heading = fx["G_center"], float(fx["G_radius"]), float(fx["G_heading"])
    tree = trees(*gen.GHOST_TREE)
    if g == "G1":
        tree.Build(pts)
        assert tree.Delete_Point_Boxes(fx["G1_boxes"]) == int(fx["G1_deleted"])
    else:
        nb = len(fx["G2_build"])
        tree.Build(pts[:nb])
        tree.set_downsample_param(float(fx["G2_ds"]))
        assert tree.Add_Points(pts[nb:], True) == int(fx["G2_counter"])
    assert tree.size() == len(live) and np.array_equal(tree.Box_Search(ALL), pts[live])
    want = live[_rule(oracle_mod, pts[live], c, r, heading)]
    assert np.array_equal(want, np.intersect1d(real, live))
    got = tree.Sector_Search(c, r, heading)
    assert got.shape == (len(want), 4) and np.array_equal(got, pts[want])
    # a query that keeps live points too: the compacted store against the rule, in order
    for c2, h2 in (([0, 0, 0], 0.0), ([3.0, -2.0, 0.5], -100.0)):
        assert not _edge_band(pts, [(c2, h2)]).any()
        want = live[_rule(oracle_mod, pts[live], c2, r, h2)]
        assert len(want) > 0 and np.array_equal(tree.Sector_Search(c2, r, h2), pts[want])


# ------------------------------------------------------------------------- GPU: live against the real tree
def _live_compare(tree, job_results, queries, pts):
    for (c, heading), ref in zip(queries, job_results):
        got = tree.Sector_Search(c, RADIUS, heading)
        order = np.argsort(got[:, 3], kind="stable")
        assert np.array_equal(got[order, 3].astype(np.int32), ref), (c, heading, len(got), len(ref))
        assert np.array_equal(got[order], pts[ref])


def _ask(job, queries):
    for c, heading in queries:
        job.sector(c, RADIUS, heading)


@needs_ref
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, SEC_BLOCK - 1, SEC_BLOCK, SEC_BLOCK + 1, 3 * SEC_BLOCK + 5])
def test_live_sizes(trees, n):
    """A map built at n points and grown by two adds (129, then 1031 points), queried at every stage, next to
    the real tree: the rows, sorted by index, are the tree's indices.  n straddles the sector filter's
    workgroup size; the first add carries 4095 and 4096 over it."""
    total = n + 129 + 1031
    pts, _ = helpers.filtered_map(np.random.default_rng(1000 + n), total, LIVE_QUERIES)
    cuts, n = (n, n + 129, total), total
    tree, job = trees(0.3, 0.6, 0.5), ikd_ref.Job(0.3, 0.6, 0.5)
    job.build(pts[: cuts[0]])
    _ask(job, LIVE_QUERIES)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        job.add(pts[lo:hi], False)
        _ask(job, LIVE_QUERIES)
    job.size()
    res = [r for r in job.run() if isinstance(r, (np.ndarray, tuple))]
    nq = len(LIVE_QUERIES)
    tree.Build(pts[: cuts[0]])
    _live_compare(tree, res[:nq], LIVE_QUERIES, pts)
    for s, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:]), 1):
        tree.Add_Points(pts[lo:hi], False)
        _live_compare(tree, res[s * nq:(s + 1) * nq], LIVE_QUERIES, pts)
    assert res[-1][:2] == (n, n) and tree.size() == n


@needs_ref
@pytest.mark.gpu
def test_live_loop_and_rebuild(trees):
    """A 12-frame loop to 16,200 points, one query per frame, then Build a second time over a larger map than
    the first.  The added frames arrive sorted along x, as a moving radar's scans do: whole sides of the real
    tree outgrow its balance criterion and go through its rebuild thread (asserted), and its answers stay
    the store's."""
    n = 16_200
    pts, _ = helpers.filtered_map(np.random.default_rng(77), n, LIVE_QUERIES)
    cuts = [2700 + 1227 * k for k in range(11)] + [n]  # 12 frames: 2700, then eleven adds
    assert cuts[-2] < n
    pts[cuts[0]:, :3] = pts[cuts[0]:, :3][np.argsort(pts[cuts[0]:, 0], kind="stable")]
    queries = [LIVE_QUERIES[k % len(LIVE_QUERIES)] for k in range(11)]
    tree, job = trees(0.3, 0.6, 0.5), ikd_ref.Job(0.3, 0.6, 0.5)
    job.build(pts[: cuts[0]])
    job.set_downsample(0.5)
    for k in range(11):
        job.add(pts[cuts[k]:cuts[k + 1]], False)
        job.sector(queries[k][0], RADIUS, queries[k][1])
        job.size()
    big, _ = helpers.filtered_map(np.random.default_rng(78), n + 3 * SEC_BLOCK + 1, LIVE_QUERIES)
    job.build(big, first=0)
    _ask(job, LIVE_QUERIES)
    job.size()
    res = [r for r in job.run() if isinstance(r, (np.ndarray, tuple))]
    tree.Build(pts[: cuts[0]])
    tree.set_downsample_param(0.5)
    for k in range(11):
        tree.Add_Points(pts[cuts[k]:cuts[k + 1]], False)
        _live_compare(tree, [res[2 * k]], [queries[k]], pts)
        assert res[2 * k + 1][:2] == (cuts[k + 1], cuts[k + 1]) and tree.size() == cuts[k + 1]
    assert res[21][2] > 0  # rebuilds handed to the rebuild thread
    tree.Build(big)
    _live_compare(tree, res[22:22 + len(LIVE_QUERIES)], LIVE_QUERIES, big)
    assert res[-1][:2] == (len(big), len(big)) and tree.size() == len(big)


# ------------------------------------------------------------------ GPU: one call site, two headers
def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
    # the real tree announces its rebuild thread on stdout
    return [ln for ln in r.stdout.split("\n") if ln.strip() and "thread" not in ln]


@needs_ref
@pytest.mark.gpu
@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("pair", sorted(SCAN_PAIRS))
def test_map_callsite_against_both_headers(oracle_mod, pair, pose):
    """tests/cpp/map_callsite.cpp compiled against the facade and against the reference's ikd_Tree.h prints
    the same `map N submap M` line and the same points (the tree in its pre-order: compared sorted)."""
    a, b, allp = _callsite_world(pair, pose, oracle_mod)
    args = (a, b) + tuple(str(v) for v in pose)
    ours = _run(os.path.join(ROOT, "tests", "cpp", "_build", "map_callsite"), *args)
    real = _run(os.path.join(ikd_ref.REF_DIR, "ref_map_callsite"), *args)
    assert ours[0] == real[0] and ours[0].split()[1] == str(len(allp))
    assert int(ours[0].split()[3]) == len(ours) - 1 > 100
    assert sorted(ours[1:]) == sorted(real[1:])


@needs_ref
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_map_edit_callsite_against_both_headers(tmp_path, case):
    """tests/cpp/map_edit_callsite.cpp against both headers on the cases of ikd_edit.npz: counter, deleted and
    the index lists (sorted) agree.  size() is the one line that differs by design: the reference counts its
    lazily deleted nodes until a rebuild drops them, the store compacts."""
    with np.load(EDIT_GOLDEN) as z:
        e = {k: z[k] for k in z.files}
    build, add, boxes = e[f"{case}_build"], e[f"{case}_add"], np.asarray(e["boxes"], F).reshape(-1, 6)
    inp = tmp_path / f"case_{case}.txt"
    with open(inp, "w") as f:
        f.write(f"{float(e[f'{case}_ds'])!r} {len(build)} {len(add)} {len(boxes)}\n")
        f.write(" ".join(repr(float(v)) for v in np.asarray(e["center"], F).reshape(-1)[:3]))
        f.write(f" {float(e['radius'])!r}\n")
        for row in np.concatenate([build, add]).astype(F):
            f.write(" ".join(repr(float(v)) for v in row[:3]) + "\n")
        for row in boxes:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    outs = []
    for exe in (os.path.join(ROOT, "tests", "cpp", "_build", "map_edit_callsite"),
                os.path.join(ikd_ref.REF_DIR, "ref_map_edit_callsite")):
        out = dict(ln.split(":", 1) for ln in _run(exe, str(inp)) if ":" in ln)
        assert sorted(out) == ["after_delete", "counter", "deleted", "radius", "size", "survivors"]
        outs.append({k: sorted(int(v) for v in out[k].split()) for k in out})
    ours, real = outs
    for key in ("counter", "deleted", "survivors", "radius", "after_delete"):
        assert ours[key] == real[key], key
    assert ours["survivors"] == e[f"{case}_survivors"].tolist() and ours["counter"] == [int(e[f"{case}_counter"])]
    assert ours["size"] == [len(ours["after_delete"])] and real["size"][0] >= ours["size"][0]
