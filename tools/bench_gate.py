"""The Doppler gate on one GPU (include/icp4r/icp4r_gate.h): what gating costs on top of
the ego-velocity batch, how far the compaction is from a plain copy, and the one-call sequence entry
against the host route it replaces.  Default shape: 1024 scans x 8192 points, dynamic = 0.1
(synth.make_sequence), every scan with its own RANSAC seed.

  (a) icp4r_static_clouds_batch_device against icp4r_ego_velocity_batch_device alone on the same
      device-resident data: the difference is what the gate adds (the guard, the xyzi write of the
      parse, the three compaction launches);
  (b) the compaction alone (icp4r_compact_by_mask_batch_device on the mask (a) left) against a
      device-to-device hipMemcpyAsync of nscans * max_n * 16 bytes, its floor;
  (c) register_static_sequence (strict pairing and the node's) against the host route built from the
      entries that existed before: the ego batch on uploaded records, a mask download, a numpy
      compaction, align_batch_host.  Host clocks around calls that end in a synchronise.

(a) and (b) are timed with device events on one stream, the two sides alternating, after warm-ups;
median, min and max of --reps.  A first measurement: no threshold.  One JSON line per measurement;
--append PATH also appends them to PATH.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("icp-4dradar_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import icp4r  # noqa: E402
from icp4r import ego, synth  # noqa: E402


def loaded_hip():
    """The HIP runtime this process already runs on (torch's), for hipMemcpyAsync."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--dynamic", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seq-reps", type=int, default=3)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    hip = loaded_hip()
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = icp4r.Context(0)
    lines = []

    def emit(**kw):
        kw.update(scans=a.scans, points=a.points, dynamic=a.dynamic)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    frames, _ = synth.make_sequence(77, frames=a.scans, n=a.points, dynamic=a.dynamic)
    ns, max_n = a.scans, a.points
    rec = np.concatenate(frames)
    cnt = np.full(ns, max_n, np.int32)
    off = (np.arange(ns, dtype=np.int64) * max_n)
    rec_d = torch.from_numpy(rec).to(dev)
    off_d, cnt_d = torch.from_numpy(off).to(dev), torch.from_numpy(cnt).to(dev)
    res_d = torch.zeros((ns, 72), dtype=torch.uint8, device=dev)
    mask_d = torch.zeros(ns * max_n, dtype=torch.uint8, device=dev)
    clouds_d = torch.zeros((ns * max_n, 4), dtype=torch.float32, device=dev)
    copy_d = torch.zeros((ns * max_n, 4), dtype=torch.float32, device=dev)
    poff_d = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    pn_d = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
    xyzi_d = torch.from_numpy(np.ascontiguousarray(rec[:, :4])).to(dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    p = ego.default_params(seed=2025)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def ego_alone():
        ego.ego_velocity_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n, res_d.data_ptr(),
                                      params=p, mask_ptr=mask_d.data_ptr(), ctx=ctx, stream=st)

    def ego_gate():
        ego.static_clouds_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n, res_d.data_ptr(),
                                       clouds_d.data_ptr(), poff_d.data_ptr(), pn_d.data_ptr(), params=p,
                                       mask_ptr=mask_d.data_ptr(), ctx=ctx, stream=st)

    def gate_alone():
        ego.compact_by_mask_batch_device(xyzi_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), mask_d.data_ptr(), ns,
                                         max_n, clouds_d.data_ptr(), poff_d.data_ptr(), pn_d.data_ptr(), ctx=ctx, stream=st)

    nbytes = ns * max_n * 16

    def d2d():
        rc = hip.hipMemcpyAsync(copy_d.data_ptr(), xyzi_d.data_ptr(), nbytes, 3, st)  # hipMemcpyDeviceToDevice
        assert rc == 0, rc

    def ab(f, g):
        for _ in range(2):
            timed(f)
            timed(g)
        tf, tg = [], []
        for _ in range(a.reps):
            tf.append(timed(f))
            tg.append(timed(g))
        return tf, tg

    # (a)
    t_ego, t_both = ab(ego_alone, ego_gate)
    kept = int(pn_d.cpu().numpy()[1:].sum())
    emit(measurement="a_ego_plus_gate_vs_ego", reps=a.reps, ego=stats(t_ego), ego_plus_gate=stats(t_both),
         gate_adds_ms=float(np.median(t_both) - np.median(t_ego)),
         ratio=float(np.median(t_both) / np.median(t_ego)), kept_points=kept, kept_share=kept / (ns * max_n))
    # (b)
    t_gate, t_copy = ab(gate_alone, d2d)
    moved = ns * max_n * 2 + kept * 32  # mask read twice, kept points read and written
    emit(measurement="b_gate_vs_d2d_copy", reps=a.reps, gate=stats(t_gate), d2d_copy=stats(t_copy), copy_bytes=nbytes,
         ratio=float(np.median(t_gate) / np.median(t_copy)), gate_bytes_by_own_account=moved,
         gate_tb_per_s=moved / (np.median(t_gate) * 1e-3) / 1e12, copy_tb_per_s=2 * nbytes / (np.median(t_copy) * 1e-3) / 1e12)

    # (c)
    def host_route():
        r_d = torch.from_numpy(np.concatenate(frames)).to(dev)  # the one-call entry packs the frames too
        ego.ego_velocity_batch_device(r_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n, res_d.data_ptr(),
                                      params=p, mask_ptr=mask_d.data_ptr(), ctx=ctx)
        ctx.synchronize()
        m = mask_d.cpu().numpy().astype(bool)
        pts = rec[:, :4][m]
        n = m.reshape(ns, max_n).sum(1).astype(np.int32)
        first = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
        prev = np.concatenate([[0], np.arange(ns - 1)])
        return ctx.align_batch_host(pts, first, n, pts, first[prev], n[prev])

    for pairing, name in ((ego.PAIR_STRICT, "strict"), (ego.PAIR_NODE, "node")):
        one = lambda: ego.register_static_sequence(frames, pairing=pairing, ego_params=p, ctx=ctx)  # noqa: E731
        t_one, t_host, same = [], [], None
        for r in range(1 + a.seq_reps):
            t0 = time.perf_counter()
            got = one()
            t1 = time.perf_counter()
            ref = host_route()
            t2 = time.perf_counter()
            if r:
                t_one.append((t1 - t0) * 1e3)
                t_host.append((t2 - t1) * 1e3)
            same = got[1].tobytes() == ref.tobytes()
        emit(measurement="c_register_static_sequence_vs_host_route", pairing=name, reps=a.seq_reps, one_call=stats(t_one),
             host_route=stats(t_host), ratio=float(np.median(t_one) / np.median(t_host)), identical_results=bool(same))
    ctx.close()
    if a.append:
        os.makedirs(os.path.dirname(os.path.abspath(a.append)), exist_ok=True)
        with open(a.append, "a") as f:
            for rec_ in lines:
                f.write(json.dumps(rec_) + "\n")


if __name__ == "__main__":
    main()
