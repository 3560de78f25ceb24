"""Generator of tests/golden/ikd_sector.npz (see make_ikd_sector_golden.md): inputs drawn here, outputs
recorded from the reference's own ikd-Tree through oracle/ikd_ref.py.  Run by hand where the reference
binaries are built (`make -C oracle ref`), never by a test:

    python tests/golden/make_ikd_sector_golden.py

make_inputs() draws every input; record(inputs) asks the real tree.  tests/test_map_reference.py imports both
to re-check the committed file.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import helpers  # noqa: E402

F = np.float32
OUT = os.path.join(HERE, "ikd_sector.npz")
RADIUS = 80.0  # RADAR_RADIUS
ALL_BOX = np.array([-1e9] * 3 + [1e9] * 3, F)
REMOVED_CAP = 1e-3

# name: (tree parameters, frame sizes, extent, seed, query centres, query headings, drift)
# Frame k is drawn around drift * p_k.  L1's frames all cover the same ground, which leaves the tree balanced
# enough for inline rebuilds of small subtrees; L2's follow the pose, as a moving radar's scans do, so whole
# sides of the tree outgrow the balance criterion and are handed to the rebuild thread.
LOOPS = {
    "L1": ((0.3, 0.6, 0.5), (600,) + (300,) * 5, 150.0, 101,
           [(3.0 * k, -2.0 * k, 0.25 * k) for k in range(1, 6)], (20.0, 95.0, 179.5, -135.0, -60.0), 0.0),
    "L2": ((0.3, 0.6, 0.5), (2000,) + (600,) * 6, 90.0, 202,
           [(-24.0 * k, 15.0 * k, 0.1 * k) for k in range(1, 7)], (0.0, -179.75, 60.0, 179.5, -90.0, 130.0), 1.0),
}
CENTER_POINT = (1, 17, 2)  # frame, position in it, query whose centre that point equals (a later frame's)
GHOST_TREE = (0.5, 0.6, 0.2)
GHOST_QUERY = ((0.0, 0.0, 0.0), 10.0, 170.0)
G1 = dict(n=1000, ext=30.0, seed=26, boxes=[[-1e9, -1e9, -1e9, 1e9, 0.0, 1e9]])  # the y < 0 half
G2 = dict(nb=1000, na=1000, ext=30.0, seed=8, ds=2.0)
TABLE_SEED, TABLE_ROWS = 5, 300


def in_edge_band(pts, queries) -> np.ndarray:
    """True per point that lies within helpers.EDGE_TOL_DEG of |dh| = 60 or 300 for any (centre, heading)."""
    bad = np.zeros(len(pts), bool)
    for c, h in queries:
        with np.errstate(invalid="ignore"):
            dh = helpers.sector_dh_f64(pts, c, h)
            bad |= (np.abs(dh - 60.0) < helpers.EDGE_TOL_DEG) | (np.abs(dh - 300.0) < helpers.EDGE_TOL_DEG)
    return bad


def draw_cloud(rng, n, ext, queries, around=(0.0, 0.0, 0.0)):
    """2 n candidates, uniform in +-ext with z scaled by 0.1, moved to `around`; those in an edge band of any
    query go, the first n of the rest stay.  -> (points (n, 3) float32, how many of the candidates seen went)."""
    cand = rng.uniform(-ext, ext, (2 * n, 3)).astype(F)
    cand[:, 2] *= F(0.1)
    cand += np.array(around, F)
    bad = in_edge_band(cand, queries)
    keep = np.nonzero(~bad)[0][:n]
    assert len(keep) == n
    removed = int(bad[: keep[-1] + 1].sum())
    assert removed <= REMOVED_CAP * n, (removed, n)
    return cand[keep], removed


def _one_ulp_inside(rng):
    """(dx, dy) with float32 dx / sqrt(dx*dx + dy*dy) exactly one ulp below 1."""
    want = np.nextafter(F(1), F(0))
    while True:
        dx = F(rng.uniform(0.5, 50.0))
        for s in np.linspace(3.0e-4, 5.0e-4, 400):
            dy = F(dx * s)
            if dx / np.sqrt(dx * dx + dy * dy, dtype=F) == want:
                return dx, dy


def table_inputs():
    """The heading table's (point, centre) pairs: the named rows first, then random ones."""
    rng = np.random.default_rng(TABLE_SEED)
    dx1, dy1 = _one_ulp_inside(rng)
    z, nz = F(0.0), F(-0.0)
    rows = [
        # dy = +0 and dy = -0 (r = +-1 exactly: dx / sqrt(dx*dx))
        ((3, 0, 0), (0, 0, 0)), ((3, nz, 0), (0, 0, 0)), ((-3, 0, 0), (0, 0, 0)), ((-3, nz, 0), (0, 0, 0)),
        ((2.5, 3, 1), (1.5, 3, 1)), ((1, 3, 0.5), (2, 3, 0.5)),
        # r = +-1 with dy < 0: dy*dy underflows, the 180 + 90 = 270 -> -90 wrap
        ((3, -1e-30, 0), (0, 0, 0)), ((-3, -1e-30, 0), (0, 0, 0)),
        # r one ulp inside +-1, on both sides of dy = 0
        ((dx1, dy1, 0), (0, 0, 0)), ((-dx1, dy1, 0), (0, 0, 0)), ((dx1, -dy1, 0), (0, 0, 0)),
        ((-dx1, -dy1, 0), (0, 0, 0)),
        # dx = +0 / -0
        ((0, 5, 0), (0, 0, 0)), ((0, -5, 0), (0, 0, 0)), ((nz, 5, 0), (0, 0, 0)), ((nz, -5, 0), (0, 0, 0)),
        ((7.25, 1, 2), (7.25, -4, 0)),
        # dz != 0 with dx = dy = 0: r = 0
        ((0, 0, 2), (0, 0, 0)), ((0, 0, -2), (0, 0, 0)), ((nz, 0, 2), (0, 0, 0)), ((4, -6, 1.5), (4, -6, -0.5)),
        # the point at the centre: 0 / 0
        ((1.5, 2.5, 0.5), (1.5, 2.5, 0.5)), ((0, 0, 0), (0, 0, 0)),
        # both sides of the > 180 -> -360 wrap, and of heading 0
        ((0.001, -5, 0), (0, 0, 0)), ((-0.001, -5, 0), (0, 0, 0)), ((1e-6, -5, 0), (0, 0, 0)),
        ((-1e-6, -5, 0), (0, 0, 0)), ((0.001, 5, 0), (0, 0, 0)), ((-0.001, 5, 0), (0, 0, 0)),
        ((10.5, -4.00001, 1), (10.5, -4, 1)), ((10.500001, -4.5, 1), (10.5, -4, 1)),
        # denormal separations: d2 underflows to 0 (r = inf), and d2 itself denormal
        ((1e-40, 0, 0), (0, 0, 0)), ((1e-40, 1e-40, 0), (0, 0, 0)), ((1e-40, -1e-40, 0), (0, 0, 0)),
        ((1e-20, 1e-20, 0), (0, 0, 0)), ((-1e-20, -1e-20, 1e-21), (0, 0, 0)), ((1e-30, 2, 0), (0, 2, 0)),
        # d2 overflows to inf: r = +-0
        ((3e19, 3e19, 0), (0, 0, 0)), ((-3e19, -1, 0), (0, 0, 0)), ((3e19, -3e19, 0), (0, 0, 0)),
        ((2e38, 1, 0), (-2e38, 0, 0)),
    ]
    pts = np.array([r[0] for r in rows], F)
    ctr = np.array([r[1] for r in rows], F)
    n = TABLE_ROWS - len(rows)
    rp = rng.uniform(-150, 150, (n, 3)).astype(F)
    rp[:, 2] *= F(0.1)
    rc = np.array([c for c, _ in helpers.MAP_QUERIES], F)[rng.integers(0, len(helpers.MAP_QUERIES), n)]
    return np.concatenate([pts, rp]), np.concatenate([ctr, rc]), len(rows)


def loop_inputs(name):
    _, sizes, ext, seed, centers, headings, drift = LOOPS[name]
    rng = np.random.default_rng(seed)
    centers = np.array(centers, F)
    headings = np.array(headings, F)
    queries = list(zip(centers, headings))
    frames, removed = [], []
    for k, n in enumerate(sizes):
        pts, r = draw_cloud(rng, n, ext, queries, F(drift) * centers[k - 1] if k else (0.0, 0.0, 0.0))
        frames.append(pts)
        removed.append(r)
    # exact duplicates of earlier points: every 41st point of an added frame from position 3 on
    dup, start, k = [], sizes[0], 0
    for f in range(1, len(sizes)):
        for j in range(3, sizes[f], 41):
            src = (7 * k + 1) % start
            frames[f][j] = np.concatenate(frames)[src]
            dup.append((start + j, src))
            k += 1
        start += sizes[f]
    cf, cj, cq = CENTER_POINT
    frames[cf][cj] = centers[cq]
    allp = np.concatenate(frames)
    assert not in_edge_band(allp, queries).any(), name  # the overwritten rows too
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return {f"{name}_frames": allp, f"{name}_frame_off": off, f"{name}_centers": centers,
            f"{name}_headings": headings, f"{name}_removed": np.array(removed, np.int32),
            f"{name}_dup": np.array(dup, np.int32),
            f"{name}_center_point": np.array([off[cf] + cj, cq], np.int32)}


def make_inputs() -> dict:
    inp = {"radius": F(RADIUS)}
    tp, tc, named = table_inputs()
    inp.update(table_points=tp, table_centers=tc, table_named=np.int32(named))
    for name in LOOPS:
        inp.update(loop_inputs(name))
    c, r, h = GHOST_QUERY
    inp.update(G_center=np.array(c, F), G_radius=F(r), G_heading=F(h))
    gq = [(inp["G_center"], inp["G_heading"])]
    p, rem = draw_cloud(np.random.default_rng(G1["seed"]), G1["n"], G1["ext"], gq)
    inp.update(G1_points=p, G1_removed=np.array([rem], np.int32), G1_boxes=np.array(G1["boxes"], F))
    rng = np.random.default_rng(G2["seed"])
    b, rb = draw_cloud(rng, G2["nb"], G2["ext"], gq)
    a, ra = draw_cloud(rng, G2["na"], G2["ext"], gq)
    inp.update(G2_build=b, G2_add=a, G2_ds=F(G2["ds"]), G2_removed=np.array([rb, ra], np.int32))
    return inp


def loop_job(inp, name):
    import ikd_ref

    off = inp[f"{name}_frame_off"]
    frames = [inp[f"{name}_frames"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    job = ikd_ref.Job(*LOOPS[name][0])
    job.build(frames[0])
    job.set_downsample(0.5)
    for k in range(1, len(frames)):
        job.add(frames[k], False)
        job.sector(inp[f"{name}_centers"][k - 1], float(inp["radius"]), float(inp[f"{name}_headings"][k - 1]))
        job.size()
    return job


def record(inp) -> dict:
    """What the real tree answers to the jobs of `inp` (needs oracle/_ref/ikd_ref)."""
    import ikd_ref

    out = {}
    job = ikd_ref.Job()
    job.heading_table(inp["table_points"], inp["table_centers"])
    out["table_heading_bits"], out["table_dist_bits"] = job.run()[0]
    for name in LOOPS:
        res = loop_job(inp, name).run()[2:]
        kept, sizes = res[1::3], res[2::3]
        assert all(s == v for s, v, _ in sizes), name  # nothing deleted on this path
        assert (sizes[-1][2] > 0) == (LOOPS[name][6] != 0.0), (name, sizes[-1])  # the rebuild thread: L2 only
        out[f"{name}_sizes"] = np.array([s for s, _, _ in sizes], np.int32)
        out[f"{name}_kept"] = np.concatenate(kept).astype(np.int32)
        out[f"{name}_kept_off"] = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int32)
    q = (inp["G_center"], float(inp["G_radius"]), float(inp["G_heading"]))
    job = ikd_ref.Job(*GHOST_TREE)
    job.build(inp["G1_points"])
    job.delete_boxes(inp["G1_boxes"])
    job.box(ALL_BOX)
    job.size()
    job.sector(*q)
    _, deleted, live, (_, valid, threaded), sector = job.run()
    assert valid == len(live) and threaded == 0
    out.update(G1_deleted=np.int32(deleted), G1_live=live, G1_sector=sector)
    job = ikd_ref.Job(*GHOST_TREE)
    job.build(inp["G2_build"])
    job.set_downsample(float(inp["G2_ds"]))
    job.add(inp["G2_add"], True)
    job.box(ALL_BOX)
    job.size()
    job.sector(*q)
    _, _, counter, live, (_, valid, threaded), sector = job.run()
    assert valid == len(live) and threaded == 0
    out.update(G2_counter=np.int32(counter), G2_live=live, G2_sector=sector)
    return out


def main():
    inp = make_inputs()
    out = record(inp)
    np.savez_compressed(OUT, **inp, **out)
    ghosts = {g: len(np.setdiff1d(out[f"{g}_sector"], out[f"{g}_live"])) for g in ("G1", "G2")}
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; removed " +
          ", ".join(f"{k}={inp[k].tolist()}" for k in inp if k.endswith("_removed")) +
          f"; ghosts {ghosts}; G1 deleted {int(out['G1_deleted'])}, G2 counter {int(out['G2_counter'])}")


if __name__ == "__main__":
    main()
