"""The incremental voxel grid against the full filter, per frame, on one GPU.

  * maps: tools/bench_voxel.py's posed radar scans (6,554 points each): 65,536 points (10 scans, cut) and
    --scans scans (default 1000 -> 6.55 M points), leaf 0.5;
  * a frame of the accumulator is add_device(the map's last 6,554 points) + filter_device on a state
    that holds the rest of the map.  Each repetition clears the accumulator and rebuilds that state
    untimed (scan by scan, add_device), reads size() once — as a caller may between frames, so the
    launches are sized by the true voxel count rather than by the points added — and times the frame;
  * the full filter is icp4r_voxel_filter_device over the whole map of the same size (the device entry:
    31-bit keys, four radix passes);
  * both in this process, alternating, HIP events on one stream around the launches: two warm-ups, then
    the mean of --reps; a repetition that takes longer than --limit-s ends the run;
  * after timing, the accumulator's output is compared with the full filter's, bit for bit.

--frames-only: no rebuilds and no full filter after the warm-up — the state is built once and --reps
frames follow (the map grows by a scan each); for a `rocprofv3 --kernel-trace` run, whose CSV
--stages PATH then turns into the per-kernel breakdown of the last frame.

One JSON line per measurement; --append PATH also appends them to PATH.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("icp-4dradar_amd", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

SCAN = 6554
LEAF = 0.5


def stages(path: str):
    """The kernels of the last accumulator frame in a rocprofv3 kernel-trace CSV: from the bounding-box
    kernel before the last acc_prep_kernel to the end of the last filter kernel."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    last = max(i for i, n in enumerate(names) if "acc_prep_kernel" in n)
    first = max(i for i in range(last) if "finite_bbox_kernel" in names[i])
    end = max(i for i, n in enumerate(names) if "acc_filter_kernel" in n or "acc_count_kernel" in n)
    assert first < last < end
    out, order = {}, []
    for r in rows[first:end + 1]:
        n = r["Kernel_Name"].split("(")[0].replace("icp4r::", "").replace("void ", "")
        if n not in out:
            out[n] = [0, 0.0]
            order.append(n)
        out[n][0] += 1
        out[n][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    span = (int(rows[end]["End_Timestamp"]) - int(rows[first]["Start_Timestamp"])) / 1e3
    return dict(measurement="voxel_acc_frame_stages", kernels=[dict(kernel=n, launches=out[n][0], us=round(out[n][1], 2)) for n in order],
                kernel_us=round(sum(v[1] for v in out.values()), 2), span_us=round(span, 2), launches=sum(v[0] for v in out.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit-s", type=float, default=60.0, help="time limit of one repetition")
    ap.add_argument("--frames-only", action="store_true")
    ap.add_argument("--stages", default=None, help="a rocprofv3 kernel-trace CSV: print the last frame's breakdown and exit")
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def finish():
        if a.append:
            os.makedirs(os.path.dirname(os.path.abspath(a.append)), exist_ok=True)
            with open(a.append, "a") as f:
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")

    if a.stages:
        emit(**stages(a.stages))
        return finish()

    import torch

    import icp4r
    from bench_map import pose
    from icp4r import synth
    from icp4r.voxel import VoxelAccumulator, VoxelGrid

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    ctx = icp4r.Context(0)
    base = [synth.make_pair(7000 + i, SCAN).src_xyzi() for i in range(64)]

    def world(k):
        R, t, _ = pose(k)
        s = base[k % len(base)]
        w = s.copy()
        w[:, :3] = (s[:, :3].astype(np.float64) @ R.T + t).astype(np.float32)
        return w

    stream = torch.cuda.Stream(dev)
    sp = stream.cuda_stream

    def measure(points: np.ndarray, label: str):
        n = len(points)
        extra = np.concatenate([world(a.scans + r) for r in range(2 + a.reps)]) if a.frames_only else np.zeros((0, 4), np.float32)
        d_map = torch.from_numpy(np.concatenate([points, extra])).to(dev)
        d_out = torch.empty((n + len(extra), 4), dtype=torch.float32, device=dev)
        d_full = torch.empty((n, 4), dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        acc = VoxelAccumulator(LEAF, ctx=ctx)
        acc.reserve(n + len(extra))
        full = VoxelGrid(ctx)
        full.setLeafSize(LEAF)
        ptr = d_map.data_ptr()
        cut = n - SCAN

        def build():
            acc.clear()
            for o in range(0, cut, SCAN):
                acc.add_device(ptr + 16 * o, min(SCAN, cut - o), sp)
            stream.synchronize()
            return acc.size()[0]

        def frame(first, count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            acc.add_device(ptr + 16 * first, count, sp)
            acc.filter_device(d_out.data_ptr(), d_cnt.data_ptr(), sp)
            e1.record(stream)
            return e0, e1

        def full_filter():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            full.filter_device(ptr, n, d_full.data_ptr(), d_cnt.data_ptr() + 4, sp)
            e1.record(stream)
            return e0, e1

        acc_ms, full_ms, state_voxels = [], [], 0
        if a.frames_only:
            state_voxels = build()
        for r in range(2 + a.reps):
            t0 = time.monotonic()
            if a.frames_only:
                ev_f = full_filter() if r < 2 else None
                ev_a = frame(cut if r == 0 else n + (r - 1) * SCAN, SCAN)
            else:
                state_voxels = build()
                ev_a = frame(cut, SCAN)
                ev_f = full_filter()
            stream.synchronize()
            if time.monotonic() - t0 > a.limit_s:
                raise SystemExit(f"{label}: repetition {r} took longer than {a.limit_s} s")
            if r >= 2:
                acc_ms.append(ev_a[0].elapsed_time(ev_a[1]))
                if ev_f:
                    full_ms.append(ev_f[0].elapsed_time(ev_f[1]))
        k_acc, k_full = int(d_cnt[0].item()), int(d_cnt[1].item())
        rec = dict(measurement="voxel_acc_frame", map=label, map_points=n, scan_points=SCAN, leaf=LEAF, reps=a.reps,
                   state_voxels=state_voxels, voxels=k_acc, acc_frame_ms=float(np.mean(acc_ms)),
                   acc_frame_ms_min=float(np.min(acc_ms)), acc_frame_ms_max=float(np.max(acc_ms)), frames_only=a.frames_only)
        if not a.frames_only:
            same = k_acc == k_full and bool((d_out[:k_acc].cpu().numpy().view(np.uint32) ==
                                             d_full[:k_full].cpu().numpy().view(np.uint32)).all())
            rec.update(full_filter_ms=float(np.mean(full_ms)), full_filter_ms_min=float(np.min(full_ms)),
                       full_filter_ms_max=float(np.max(full_ms)), full_voxels=k_full, identical_to_full_filter=same,
                       full_over_acc=float(np.mean(full_ms) / np.mean(acc_ms)))
        emit(**rec)
        acc.close()
        if not a.frames_only and not rec["identical_to_full_filter"]:
            raise SystemExit(f"{label}: the accumulator's output differs from the full filter's")

    if not a.frames_only:
        measure(np.concatenate([world(k) for k in range(10)])[:65536], "65,536 points")
    measure(np.concatenate([world(k) for k in range(a.scans)]), f"{a.scans} scans")
    ctx.close()
    finish()


if __name__ == "__main__":
    main()
