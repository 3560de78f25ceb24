"""What reciprocal correspondences cost on one GPU (icp4r_params.use_reciprocal_correspondences).

Two shapes, each registered with the flag off and on from the same device-resident batch:
  C3  --pairs (1024) pairs x --points (8192), 20 fixed iterations (bench.py's headline workload);
  C2  one pair of --points, 20 fixed iterations.
The two sides alternate in one process after warm-ups, timed with device events on one stream; median,
min and max of --reps.  With the flag on a further call runs with per-kernel events for the stage's own
time (icp4r_stage_time_ms(ICP4R_STAGE_RECIPROCAL): the two launches of one iteration) beside the
search's and the update's.  A first measurement: no threshold.  One JSON line per measurement;
--append PATH also appends them to PATH.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "icp-4dradar_amd"))

import numpy as np  # noqa: E402

import icp4r  # noqa: E402
from icp4r import synth  # noqa: E402


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="C3,C2")
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    ctx = icp4r.Context(0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(name, P, first):
        n = a.points
        src = np.empty((P, n, 4), np.float32)
        tgt = np.empty((P, n, 4), np.float32)
        for k in range(P):
            p = synth.make_pair(first + k, n)
            src[k], tgt[k] = p.src_xyzi(), p.tgt_xyzi()
        src_d = torch.from_numpy(src.reshape(-1, 4)).to(dev)
        tgt_d = torch.from_numpy(tgt.reshape(-1, 4)).to(dev)
        off = torch.arange(P, dtype=torch.int64, device=dev) * n
        cnt = torch.full((P,), n, dtype=torch.int32, device=dev)
        res = {f: torch.zeros((P, 96), dtype=torch.uint8, device=dev) for f in (0, 1)}
        torch.cuda.synchronize()
        batch = icp4r.Batch(src=src_d.data_ptr(), tgt=tgt_d.data_ptr(), src_off=off.data_ptr(), src_n=cnt.data_ptr(),
                            tgt_off=off.data_ptr(), tgt_n=cnt.data_ptr(), guess=None, aligned=None, npairs=P,
                            max_src_n=n, max_tgt_n=n)
        fixed = dict(max_iterations=a.iters, mse_threshold_absolute=-1.0, transformation_epsilon=-1.0)
        par = {f: icp4r.default_params(use_reciprocal_correspondences=f, **fixed) for f in (0, 1)}
        run = {f: (lambda f=f: ctx.align_batch_device(batch, par[f], res[f].data_ptr(), st)) for f in (0, 1)}
        ctx.set_kernel_timing(False)
        for _ in range(a.warmup):
            for f in (0, 1):
                timed(run[f])
        ms = {0: [], 1: []}
        for _ in range(a.reps):
            for f in (0, 1):
                ms[f].append(timed(run[f]))
        rows = {f: np.frombuffer(res[f].cpu().numpy().tobytes(), dtype=icp4r.RESULT_DTYPE) for f in (0, 1)}
        # the stages' own times: one call with per-kernel events (after one that creates them)
        ctx.set_kernel_timing(True)
        stage = {}
        for f in (0, 1):
            timed(run[f])
            ctx.reset_timers()
            timed(run[f])
            stage[f] = {k: ctx.stage_time_ms(s)[0] for k, s in (("nn", icp4r.STAGE_NN), ("update", icp4r.STAGE_UPDATE))}
            if f:
                stage[f]["reciprocal"], stage[f]["reciprocal_launches"] = ctx.stage_time_ms(icp4r.STAGE_RECIPROCAL)
        ctx.set_kernel_timing(False)
        med = {f: float(np.median(ms[f])) for f in (0, 1)}
        emit(measurement=name + "_reciprocal_off_vs_on", pairs=P, points=n, iterations=a.iters, reps=a.reps,
             off=stats(ms[0]), on=stats(ms[1]), on_over_off=med[1] / med[0],
             pairs_per_s_off=P / (med[0] * 1e-3), pairs_per_s_on=P / (med[1] * 1e-3),
             stage_ms_per_launch_off=stage[0], stage_ms_per_launch_on=stage[1],
             kept_share_last_iteration=float(rows[1]["n_correspondences"].mean() / n),
             status_ok=bool((rows[0]["status"] == 0).all() and (rows[1]["status"] == 0).all()),
             plan_flag_off=icp4r.plan(P, n, n, ctx=ctx))

    only = a.only.split(",")
    if "C3" in only:
        measure("C3", a.pairs, 0)
    if "C2" in only:
        measure("C2", 1, 1)
    ctx.close()
    if a.append:
        with open(a.append, "a") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
