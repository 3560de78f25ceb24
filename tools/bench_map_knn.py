"""The map store's Nearest_Search on one GPU: index build and batched k-NN search.

  * maps: tools/bench_map.py's posed radar scans (6,554 points each along its trajectory): 65,536
    points (10 scans, cut) and --scans scans (default 1500 -> 9.83 M points);
  * queries: the next scan in the world frame, k = 5, max_dist = inf and 1 m, device variant;
  * index build time and search time by the store's HIP events (the search's includes the query
    sort), queries/s; the brute path on the 65,536 map; the tail path after 1, 2 and 4 appended
    scans; index against brute on small maps (the default path's crossover).

Warm-up first (a small tree through every kernel), then --reps timed searches per figure.  One JSON
line per measurement; --append PATH also appends them to PATH.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("icp-4dradar_amd", "oracle", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import icp4r  # noqa: E402
from bench_map import pose  # noqa: E402
from icp4r import synth  # noqa: E402
from icp4r.mapstore import KD_TREE, KNN_BRUTE, KNN_INDEX  # noqa: E402

SCAN = 6554
K = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    ctx = icp4r.Context(0)
    base = [synth.make_pair(7000 + i, SCAN).src_xyzi() for i in range(64)]
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def world(k):
        R, t, _ = pose(k)
        s = base[k % len(base)]
        w = s.copy()
        w[:, :3] = (s[:, :3].astype(np.float64) @ R.T + t).astype(np.float32)
        return w

    out = {"p": torch.empty((SCAN * K, 4), device=dev), "d": torch.empty(SCAN * K, device=dev),
           "i": torch.empty(SCAN * K, dtype=torch.int32, device=dev), "f": torch.empty(SCAN, dtype=torch.int32, device=dev)}

    def search(tree, dq, md, flags, reps):
        """-> (average device ms over reps searches, found, index) after two warm-up searches."""
        for r in range(2 + reps):
            if r == 2:
                ctx.synchronize()
                tree.reset_timers()
            tree.nearest_search_device(dq.data_ptr(), SCAN, K, md, out["p"].data_ptr(), out["d"].data_ptr(),
                                       out["i"].data_ptr(), out["f"].data_ptr(), flags=flags)
        ctx.synchronize()
        ms, calls = tree.time_ms()
        assert calls == reps
        return ms, out["f"].cpu().numpy().copy(), out["i"].cpu().numpy().copy(), out["d"].cpu().numpy().copy()

    def build_ms(tree):
        ctx.synchronize()
        tree.reset_timers()
        tree.index_build()
        ms, calls = tree.time_ms()
        assert calls == 1
        return ms

    # warm-up: every kernel once on a small map
    warm = KD_TREE(ctx=ctx)
    warm.Build(world(0))
    dq = torch.from_numpy(world(1)).to(dev)
    for fl in (KNN_INDEX, KNN_BRUTE):
        search(warm, dq, float("inf"), fl, 1)
    warm.close()

    # small maps: index against brute (the default path's crossover)
    pool = np.concatenate([world(k) for k in range(10)])
    for n in (256, 1024, 4096, 16384):
        t = KD_TREE(ctx=ctx)
        t.Build(pool[:n])
        b = build_ms(t)
        dq = torch.from_numpy(world(10)).to(dev)
        mi, fi, ii, di = search(t, dq, float("inf"), KNN_INDEX, a.reps)
        mb, fb, ib, db = search(t, dq, float("inf"), KNN_BRUTE, a.reps)
        emit(measurement="knn_small_map", map_points=n, queries=SCAN, k=K, index_build_ms=b, index_search_ms=mi,
             brute_search_ms=mb, identical=bool((fi == fb).all() and (ii == ib).all() and (di == db).all()))
        t.close()

    for scans in (10, a.scans):
        t = KD_TREE(ctx=ctx)
        if scans == 10:
            t.Build(pool[:65536])
        else:
            for k in range(scans):
                R, tt, _ = pose(k)
                t.add_scan(base[k % len(base)], R, tt)
        n = t.size()
        b1 = build_ms(t)
        dq = torch.from_numpy(world(scans)).to(dev)
        for md in (float("inf"), 1.0):
            ms, f, idx, d = search(t, dq, md, KNN_INDEX, a.reps)
            rec = dict(measurement="knn_search", map_points=n, queries=SCAN, k=K, max_dist=md if md < 1e30 else "inf",
                       index_build_ms=b1, search_ms=ms, queries_per_s=SCAN / (ms * 1e-3), mean_found=float(f.mean()))
            if scans == 10:
                mb, fb, ib, db = search(t, dq, md, KNN_BRUTE, a.reps)
                rec.update(brute_search_ms=mb, identical_to_brute=bool((f == fb).all() and (idx == ib).all() and (d == db).all()))
            emit(**rec)
        # the tail path: appended scans swept by brute force behind the tree walk
        added = 0
        for tail_scans in (1, 2, 4):
            while added < tail_scans:
                R, tt, _ = pose(scans + added)
                t.add_scan(base[(scans + added) % len(base)], R, tt)
                added += 1
            st = t.index_stats()
            if st["tail"] + st["indexed"] != t.size() or st["tail"] > st["tail_limit"]:
                break
            dq2 = torch.from_numpy(world(scans + added)).to(dev)
            ms, f, _, _ = search(t, dq2, float("inf"), 0, a.reps)
            st2 = t.index_stats()
            emit(measurement="knn_tail", map_points=t.size(), indexed=st2["indexed"], tail=st2["tail"], queries=SCAN, k=K,
                 search_ms=ms, queries_per_s=SCAN / (ms * 1e-3))
        b2 = build_ms(t)  # the rebuild a search past tail_limit would pay
        emit(measurement="knn_rebuild", map_points=t.size(), index_build_ms=b2, first_build_ms=b1)
        t.close()
    ctx.close()
    if a.append:
        os.makedirs(os.path.dirname(os.path.abspath(a.append)), exist_ok=True)
        with open(a.append, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
