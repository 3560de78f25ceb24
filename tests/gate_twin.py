"""A numpy statement of the Doppler gate's contract (include/icp4r/icp4r_gate.h): what the device
compaction must write, and the node's running-cloud pairing as its literal loop."""
from __future__ import annotations

import numpy as np

GATE_STATIC, GATE_ALL = 0, 1


def compact(xyzi, off, cnt, mask, max_n, mode=GATE_STATIC):
    """clouds (total, 4) float32, pair_off (nscans + 1) int64, pair_n (nscans + 1) int32: the kept points
    of scan 0, scan 1, ... tightly packed in input order; the descriptors preceded by one duplicate of
    scan 0's entry.  Point i of scan s is xyzi[off[s] + i], its mask byte mask[off[s] + i] (non-zero:
    kept).  A scan with cnt > max_n (or < 0) keeps nothing and its mask is not looked at."""
    xyzi = np.asarray(xyzi, np.float32).reshape(-1, 4)
    parts, counts = [], []
    for o, n in zip(off, cnt):
        o, n = int(o), int(n)
        if n < 0 or n > max_n:
            n = 0
        pts = xyzi[o:o + n]
        if mode == GATE_STATIC:
            pts = pts[np.asarray(mask[o:o + n]) != 0]
        parts.append(pts)
        counts.append(len(pts))
    clouds = np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)
    first = np.concatenate([[0], np.cumsum(counts)])[:len(counts)].astype(np.int64)
    pair_off = np.concatenate([first[:1], first]).astype(np.int64)
    pair_n = np.concatenate([counts[:1], counts]).astype(np.int32)
    return clouds.reshape(-1, 4), pair_off, pair_n


def sequence_pairs(counts):
    """The node's loop (src/iterative_closest_point.cpp:306-315, :505, :698-699), literally: every
    frame pushes the points of scan k onto cloud_src_in and those of scan k-1 (scan 0 for k = 0) onto
    cloud_tar_in; it registers iff both hold a point, and clears them only then.  A point is written
    as the index of the scan it came from.  Returns one (registered, src points, tgt points) per frame:
    the clouds as they stand at the frame's size test."""
    cloud_src_in, cloud_tar_in = [], []
    frames = []
    for k in range(len(counts)):
        last = k - 1 if k else 0
        for _ in range(int(counts[k])):
            cloud_src_in.append(k)
        for _ in range(int(counts[last])):
            cloud_tar_in.append(last)
        registered = bool(len(cloud_tar_in) and len(cloud_src_in))
        frames.append((registered, list(cloud_src_in), list(cloud_tar_in)))
        if registered:
            cloud_src_in.clear()
            cloud_tar_in.clear()
    return frames
