"""Sequential restatement of ikd-Tree's map-maintenance rules, in numpy float32 / float64 exactly as
third_party/ikd-Tree/ikd_Tree.cpp evaluates them: box membership, Delete_Point_Boxes, Box_Search,
Radius_Search and the downsampling Add_Points(.., true).  Pinned to recorded outputs of the reference's
own code by tests/test_map_edit.py::test_twin_matches_reference_fixture (tests/golden/ikd_edit.npz).

A store is an (N, 4) float32 array (x, y, z, intensity) in insertion order; functions return new arrays.
Where the reference depends on its tree order, this restatement decides: results are in insertion
order; surviving stored points keep their places and arriving points that stay are appended in input
order; among stored points that tie exactly for nearest in a box, the lowest index stays.
"""
from __future__ import annotations

import numpy as np

F = np.float32


def calc_dist(a, b):
    """KD_TREE::calc_dist (ikd_Tree.cpp:1427-1431): float, ((dx*dx + dy*dy) + dz*dz).  a: (..., 3)."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    d = (a[..., :3] - b[..., :3]).astype(F)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F) + d[..., 2] * d[..., 2]).astype(F)


def in_box(pts, lo, hi):
    """min[k] <= p[k] && max[k] > p[k] on all axes (ikd_Tree.cpp:678, :786, :1034)."""
    p = np.asarray(pts, F).reshape(-1, pts.shape[-1])[:, :3]
    lo = np.asarray(lo, F)
    hi = np.asarray(hi, F)
    return ((lo <= p) & (hi > p)).all(axis=1)


def box_search(store, box):
    box = np.asarray(box, F).reshape(6)
    return store[in_box(store, box[:3], box[3:])] if len(store) else store[:0]


def radius_search(store, center, radius):
    if not len(store):
        return store[:0]
    r = F(radius)
    return store[calc_dist(store, np.asarray(center, F)[:3]) <= F(r * r)]


def delete_boxes(store, boxes):
    """-> (survivors in order, number deleted); a point in several boxes counts once."""
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    dead = np.zeros(len(store), bool)
    if len(store):
        for b in boxes:
            dead |= in_box(store, b[:3], b[3:])
    return store[~dead], int(dead.sum())


def ds_box(p, ds):
    """The downsample box of p and its centre (ikd_Tree.cpp:432-440)."""
    ds = F(ds)
    lo = (np.floor((np.asarray(p, F)[:3] / ds).astype(F)).astype(F) * ds).astype(F)
    hi = (lo + ds).astype(F)
    mid = (lo.astype(np.float64) + (hi - lo).astype(F).astype(np.float64) / 2.0).astype(F)
    return lo, hi, mid


def same_point(a, b):
    """ikd_Tree.cpp:1422-1423: float fabs against the double 1e-6."""
    d = np.abs((np.asarray(a, F)[:3] - np.asarray(b, F)[:3]).astype(F)).astype(np.float64)
    return bool((d < 1e-6).all())


def add_points_downsample(store, pts, ds):
    """Add_Points(pts, true) (ikd_Tree.cpp:430-457) -> (new store, counter).  Surviving stored points
    keep their places; arriving points that stay are appended in input order.

    The box, its centre and the distance to it are functions of a point's own floor(p / ds) cell, so
    they are formed for all points at once; a stored point is a candidate of an arriving point's
    Search_by_range when the cells agree and it passes the box test.  (For a ds that is no power of two,
    fl(fl(k * ds) + ds) and fl((k + 1) * ds) can differ by an ulp, so the reference's neighbouring boxes
    overlap or leave a gap one ulp wide; within an ulp of such a face this differs from the reference,
    and the fixtures keep ds = 0.3 inputs 1e-4 ds away from faces.  For ds = 0.5 faces are exact.)
    The loop itself is the reference's, one arriving point after the other."""
    store = np.ascontiguousarray(store, F).reshape(-1, 4)
    pts = np.ascontiguousarray(pts, F).reshape(-1, 4)
    n0 = len(store)
    allp = np.concatenate([store, pts])
    if not len(allp):
        return allp, 0
    dsf = F(ds)
    cell = np.floor((allp[:, :3] / dsf).astype(F)).astype(F)
    lo = (cell * dsf).astype(F)
    hi = (lo + dsf).astype(F)
    mid = (lo.astype(np.float64) + (hi - lo).astype(F).astype(np.float64) / 2.0).astype(F)
    dist = calc_dist(allp, mid).tolist()
    inside = ((lo <= allp[:, :3]) & (hi > allp[:, :3])).all(axis=1)
    keys = [tuple(c) for c in cell.tolist()]
    alive = np.zeros(len(allp), bool)
    alive[:n0] = True
    members: dict[tuple, list[int]] = {}  # cell -> live points in its box, ascending store index first
    for i in range(n0):
        if inside[i]:
            members.setdefault(keys[i], []).append(i)
    counter = 0
    for j in range(n0, len(allp)):
        S = members.setdefault(keys[j], [])
        best, md = j, dist[j]
        for i in S:  # ties among stored points: the first, i.e. the lowest store index
            if dist[i] < md:
                md, best = dist[i], i
        if len(S) > 1 or best == j or same_point(allp[j], allp[best]):
            for i in S:
                alive[i] = False
            alive[best] = True
            S[:] = [best]
            counter += 1
    return allp[alive], counter
