"""Voxel-grid downsampling of the map on one GPU: pcl::VoxelGrid at leaf 0.5 over the
resident store, the node's surround-map step (radar_odometry.cpp:426-429).

  * maps: tools/bench_map.py's posed radar scans (6,554 points each along its trajectory): 65,536
    points (10 scans, cut), --fit-scans scans (default 1000 -> 6.55 M points, the largest round number
    whose grid PCL accepts at leaf 0.5) and --scans scans (default 1500 -> 9.83 M points: grid overflow
    at leaf 0.5, PCL's "Leaf size is too small"; measured at leaf 0.5, the overflow path, and at leaf 1);
  * the device-resident form (KD_TREE.voxel_filter_device: no host round trip, 31-bit keys, four radix
    passes), timed by the library's HIP events around its launches: two warm-ups, then the mean of
    --reps; the bytes the kernels move by the pipeline's own account, and the TB/s that makes;
  * for context only: the C++ restatement of PCL's loop (tests/cpp/voxel_host_check.cpp, g++ -O2) on
    the same points on this machine's CPU, one run, file I/O excluded; its output is compared with
    the library's, bit for bit.

A first measurement: there is no earlier time and no reference time (PCL is not available).  One JSON
line per measurement; --append PATH also appends them to PATH.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("icp-4dradar_amd", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import icp4r  # noqa: E402
from bench_map import pose  # noqa: E402
from icp4r import synth  # noqa: E402
from icp4r.mapstore import KD_TREE  # noqa: E402
from icp4r.voxel import VoxelGrid  # noqa: E402

SCAN = 6554
LEAF = 0.5
RADIX_PASSES = 4  # the device entry sorts all 31 key bits


def bytes_moved(n: int, k: int) -> int:
    """Global-memory traffic by the pipeline's own account (reads + writes; cache hits not discounted):
    box 16 B/point; keys 16 + 8; per radix pass 8 (count) + 8 + 8 (scatter); run heads 8 + 8 (count and
    write passes over the sorted keys); centroids 8 (sorted index) + 16 (gather) per point; per voxel
    4 + 4 + 4 (heads written, read twice) + 8 + 8 (records written, read) + 16 (output)."""
    return n * (16 + 24 + RADIX_PASSES * 24 + 16 + 24) + k * 44


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1500)
    ap.add_argument("--fit-scans", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--append", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement's time")
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    ctx = icp4r.Context(0)
    timer = VoxelGrid(ctx)  # the context's voxel timers
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

    host_exe, tmp = None, None
    if not a.no_host and shutil.which("g++"):
        import voxel_tools

        tmp = tempfile.mkdtemp(prefix="bench_voxel_")
        host_exe = voxel_tools.compile_host_check(tmp)

    def measure(t, leaf):
        n = t.size()
        d_out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for r in range(2 + a.reps):
            if r == 2:
                ctx.synchronize()
                timer.reset_timers()
            t.voxel_filter_device(leaf, d_out.data_ptr(), d_cnt.data_ptr())
        ctx.synchronize()
        ms, calls = timer.time_ms()
        assert calls == a.reps
        k = int(d_cnt.item())
        moved = bytes_moved(n, max(k, 0))
        # on grid overflow (k = -1) every key is the non-participating one: the launches still run, over no voxel
        rec = dict(measurement="voxel_filter_device", map_points=n, leaf=leaf, voxels=k, grid_overflow=k < 0, reps=a.reps,
                   filter_ms=ms, points_per_s=n / (ms * 1e-3), bytes_moved=moved, tb_per_s=moved / (ms * 1e-3) / 1e12,
                   radix_passes=RADIX_PASSES)
        if host_exe:
            store = t.Box_Search([-np.inf] * 3 + [np.inf] * 3)  # the stored points (all finite), insertion order
            assert len(store) == n
            ref, host_ms = voxel_tools.run_host_check(host_exe, tmp, store, leaf)
            same = (ref is None) if k < 0 else (ref is not None and voxel_tools.same_bits(d_out[:k].cpu().numpy(), ref))
            rec.update(host_check_cpu_ms=host_ms, identical_to_host_check=bool(same))
        emit(**rec)

    t = KD_TREE(ctx=ctx)
    t.Build(np.concatenate([world(k) for k in range(10)])[:65536])
    measure(t, LEAF)
    t.close()
    # the posed-scan map as it grows: --fit-scans scans still fit PCL's grid at leaf 0.5 (div0 div1 div2 <=
    # INT32_MAX), --scans scans (3.7 km x 3.9 km x 45 m) do not — PCL refuses that map — and fit at leaf 1
    t = KD_TREE(ctx=ctx)
    added = 0
    for scans, leaves in ((min(a.fit_scans, a.scans), (LEAF,)), (a.scans, (LEAF, 2 * LEAF))):
        while added < scans:
            R, tt, _ = pose(added)
            t.add_scan(base[added % len(base)], R, tt)
            added += 1
        for leaf in leaves:
            measure(t, leaf)
    t.close()
    ctx.close()
    if tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.append:
        os.makedirs(os.path.dirname(os.path.abspath(a.append)), exist_ok=True)
        with open(a.append, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
