"""The map store's Nearest_Search contract (include/icp4r/icp4r_map.h) in numpy, for the tests:

  d_i = calc_dist(q, p_i) in float32, ((dx*dx) + dy*dy) + dz*dz (ikd_Tree.cpp:1427-1431);
  p_i is a candidate iff its three coordinates are finite and (double)d_i <= max_dist * max_dist
  (the product in double, as ikd_Tree.cpp:385 takes it);
  the answer is the min(k, #candidates) smallest candidates by (d_i, i), ascending;
  a query with a non-finite coordinate finds nothing.

Pinned to the reference's own tree by tests/test_map_nearest.py (tests/golden/ikd_nearest.npz).
"""
from __future__ import annotations

import numpy as np

F = np.float32


def calc_dist(q, store):
    """float32 squared distances of one query (3,) to every stored point (N, >=3), the reference's order."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (np.asarray(q, F)[:3] - np.asarray(store, F)[:, :3]).astype(F)
        s = (d[:, 0] * d[:, 0]).astype(F)
        s = (s + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
        s = (s + (d[:, 2] * d[:, 2]).astype(F)).astype(F)
    return s


def nearest_search(store, queries, k, max_dist=np.inf):
    """-> points (nq, k, 4), dist (nq, k), index (nq, k), found (nq,) with the store's filling of unused
    slots: a zero point, +inf and -1."""
    store = np.asarray(store, F).reshape(-1, 4)
    queries = np.asarray(queries, F)
    nq = len(queries)
    pts = np.zeros((nq, k, 4), F)
    dist = np.full((nq, k), np.inf, F)
    idx = np.full((nq, k), -1, np.int32)
    found = np.zeros(nq, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        md2 = np.float64(max_dist) * np.float64(max_dist)
    stored_ok = np.isfinite(store[:, :3]).all(axis=1) if len(store) else np.zeros(0, bool)
    for j, q in enumerate(queries):
        if not len(store) or not np.isfinite(q[:3]).all():
            continue
        d = calc_dist(q, store)
        with np.errstate(invalid="ignore"):
            cand = np.flatnonzero(stored_ok & (d.astype(np.float64) <= md2))
        if len(cand) > k:  # only candidates up to the k-th smallest distance can be in the answer
            dc = d[cand]
            cand = cand[dc <= np.partition(dc, k - 1)[k - 1]]
        order = cand[np.lexsort((cand, d[cand]))][:k]
        m = len(order)
        found[j] = m
        pts[j, :m] = store[order]
        dist[j, :m] = d[order]
        idx[j, :m] = order
    return pts, dist, idx, found


def tied(store, q, k):
    """True when the k + 1 smallest distances of query q hold an equal pair (the reference may then keep
    another index than the lowest)."""
    d = np.sort(calc_dist(q, np.asarray(store, F).reshape(-1, 4)))[:k + 1]
    return bool((d[1:] == d[:-1]).any())
