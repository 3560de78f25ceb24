"""Voxelized GICP against GICP on the scan-to-map call, one build, one session.

    python tools/bench_vgicp.py [--steps 9] [--warmup 3] [--pairs 256] [--out profiles/vgicp/bench_vgicp.jsonl]

Cases:
  map    the §6d map call: one 8k-point scan, associated to the map frame with a slightly wrong odometry
         prediction, against a 65k-point submap (synth.make_map_pair), k = 5 — through VGICP at resolution
         1.0 / DIRECT1 and through GICP
  batch  --pairs independent 8k/8k pairs, k = 5, one device batch, both ways

The two sides alternate call by call on one context; a time is the median over --steps calls after --warmup
of each, by the device events around a whole registration (ICP4R_STAGE_BATCH), without per-stage events.
A second pass with per-stage events (each costs device time between kernels) splits a VGICP call into the
covariances (ICP4R_STAGE_GICP_COV), the iterations (ICP4R_STAGE_UPDATE: lookup, linearisation and trials)
and the map build — the device time of a call with max_iterations = 0 and no fitness pass less its
covariances, so it carries that call's validation and result kernels too.  The pose each side reaches is
compared with the scene's true pose.  No threshold: the line records what one run measured.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "icp-4dradar_amd"), os.path.join(ROOT, "tests")]


def _pad4(x):
    out = np.zeros((len(x), 4), np.float32)
    out[:, :3] = x[:, :3]
    return out


def _pose_err(T, Tgt):
    T, Tgt = np.asarray(T, np.float64), np.asarray(Tgt, np.float64)
    M = T[:3, :3].T @ Tgt[:3, :3]
    ang = np.arctan2(np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2, (np.trace(M) - 1) / 2)
    return float(np.linalg.norm(T[:3, 3] - Tgt[:3, 3])), float(ang)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--neighbor-search", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgicp", "bench_vgicp.jsonl"))
    a = ap.parse_args()
    import torch

    import icp4r
    from icp4r import gicp, synth, vgicp

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    ctx = icp4r.Context(0)
    side = torch.cuda.Stream(dev)

    def device_batch(pairs):
        src = np.concatenate([_pad4(s) for s, _ in pairs])
        tgt = np.concatenate([_pad4(t) for _, t in pairs])
        sn = np.array([len(s) for s, _ in pairs], np.int32)
        tn = np.array([len(t) for _, t in pairs], np.int32)
        so = np.concatenate([[0], np.cumsum(sn)[:-1]]).astype(np.int64)
        to = np.concatenate([[0], np.cumsum(tn)[:-1]]).astype(np.int64)
        ts = {n: torch.from_numpy(v).to(dev) for n, v in dict(src=src, tgt=tgt, sn=sn, tn=tn, so=so, to=to).items()}
        ts["res"] = torch.zeros(len(pairs) * icp4r.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        b = icp4r.Batch()
        b.src, b.tgt = ts["src"].data_ptr(), ts["tgt"].data_ptr()
        b.src_off, b.src_n, b.tgt_off, b.tgt_n = ts["so"].data_ptr(), ts["sn"].data_ptr(), ts["to"].data_ptr(), ts["tn"].data_ptr()
        b.npairs, b.max_src_n, b.max_tgt_n = len(pairs), int(sn.max()), int(tn.max())
        return b, ts

    def one(call, b, ts, p):
        """One timed call: (device ms of the registration, its stage times)."""
        torch.cuda.synchronize()
        ctx.reset_timers()
        call(b, p, ts["res"].data_ptr(), stream=side.cuda_stream, ctx=ctx)
        torch.cuda.synchronize()
        st = {n: ctx.stage_time_ms(s) for n, s in (("cov", icp4r.STAGE_GICP_COV), ("nn", icp4r.STAGE_NN),
                                                   ("iter", icp4r.STAGE_UPDATE), ("batch", icp4r.STAGE_BATCH))}
        return st["batch"][0], st

    def measure(name, pairs, truths):
        b, ts = device_batch(pairs)
        pg = gicp.default_params(k_correspondences=5)
        pv = vgicp.default_params(k_correspondences=5, voxel_resolution=a.resolution, neighbor_search=a.neighbor_search)
        sides = {"vgicp": (vgicp.align_batch_device, pv), "gicp": (gicp.align_batch_device, pg)}
        ctx.set_kernel_timing(False)
        times = {k: [] for k in sides}
        rows = {}
        for it in range(a.warmup + a.steps):
            for k, (call, p) in sides.items():  # the sides alternate
                ms, _ = one(call, b, ts, p)
                if it >= a.warmup:
                    times[k].append(ms)
                rows[k] = np.frombuffer(ts["res"].cpu().numpy().tobytes(), icp4r.RESULT_DTYPE).copy()
        line = {"measurement": f"vgicp_{name}", "pairs": len(pairs), "src_points": int(b.max_src_n),
                "tgt_points": int(b.max_tgt_n), "k": 5, "resolution": a.resolution, "neighbor_search": a.neighbor_search,
                "steps": a.steps, "warmup": a.warmup}
        for k in sides:
            r = rows[k]
            errs = [_pose_err(r[i]["T"].reshape(4, 4).T, truths[i]) for i in range(len(pairs))]
            line[k] = {"device_ms_median": float(np.median(times[k])), "device_ms_min": float(np.min(times[k])),
                       "device_ms_max": float(np.max(times[k])), "iterations_mean": float((r["iterations"] + 1).mean()),
                       "converged": int(r["converged"].sum()), "correspondences_mean": float(r["n_correspondences"].mean()),
                       "pose_err_m_median": float(np.median([e[0] for e in errs])),
                       "pose_err_m_max": float(np.max([e[0] for e in errs])),
                       "pose_err_rad_median": float(np.median([e[1] for e in errs])),
                       "pose_err_rad_max": float(np.max([e[1] for e in errs]))}
        line["vgicp_over_gicp"] = line["vgicp"]["device_ms_median"] / line["gicp"]["device_ms_median"]
        # the stage split (per-stage events on: the totals are larger than above)
        ctx.set_kernel_timing(True)
        for k, (call, p) in sides.items():
            one(call, b, ts, p)
            _, st = one(call, b, ts, p)
            line[k]["stages_with_events"] = {n: {"avg_ms": v[0], "launches": v[1]} for n, v in st.items()}
        p0 = vgicp.default_params(k_correspondences=5, voxel_resolution=a.resolution, neighbor_search=a.neighbor_search,
                                  max_iterations=0, compute_fitness=0)
        one(vgicp.align_batch_device, b, ts, p0)
        build = []
        for _ in range(a.steps):
            ms, st = one(vgicp.align_batch_device, b, ts, p0)
            build.append(ms - st["cov"][0])
        line["vgicp"]["map_build_ms_median"] = float(np.median(build))
        ctx.set_kernel_timing(False)
        return line

    lines = []
    pr = synth.make_map_pair(0, n_src=a.points)
    yaw = np.deg2rad(1.0)
    err = np.array([[np.cos(yaw), -np.sin(yaw), 0.0, 0.3], [np.sin(yaw), np.cos(yaw), 0.0, -0.2],
                    [0.0, 0.0, 1.0, 0.05], [0.0, 0.0, 0.0, 1.0]])
    Tp = pr.T_gt @ err
    src_map = pr.src.copy()
    src_map[:, :3] = (pr.src[:, :3].astype(np.float64) @ Tp[:3, :3].T + Tp[:3, 3]).astype(np.float32)
    # the scan sits at (T_gt err) src and belongs at T_gt src: the true answer is T_gt err⁻¹ T_gt⁻¹
    lines.append(measure("map", [(src_map, pr.tgt)], [pr.T_gt @ np.linalg.inv(err) @ np.linalg.inv(pr.T_gt)]))
    pairs, truths = [], []
    for i in range(a.pairs):
        q = synth.make_pair(i % 64, a.points)
        pairs.append((q.src, q.tgt))
        truths.append(q.T_gt)
    lines.append(measure("batch", pairs, truths))
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
