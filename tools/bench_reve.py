"""The 3D Doppler ego-velocity estimator on one GPU (include/icp4r/icp4r_reve.h): what
a batch of scans costs, what packing the inlier scans adds, how that compares with the sine route over
the same records, and how far all of it is from one pass over the records.  Default shape: 1024 scans x
8192 points, dynamic = 0.1, elevations within +-30 degrees (synth.make_sequence), every scan with its
own RANSAC seed (16 distinct scans taken in turn).

  estimator          icp4r_reve_batch_device (results and the inlier mask)
  estimator_pack     icp4r_reve_inlier_clouds_batch_device (the same, then the gate's compaction)
  sine_route         icp4r_static_clouds_batch_device on the same device-resident records
  d2d_copy           hipMemcpyAsync, device to device, of nscans * max_n * 20 bytes: the floor

Timed with device events on one stream, the four sides taking turns, after two warm-up rounds; median,
min and max of --reps.  A first measurement: no threshold.  The ratio to the copy says how many passes
over the records the kernel's time is worth; it is reported beside the kernel's own account of the bytes
it moves (20 B read and 1 B of mask written per record; packing adds the 16-B xyzi copy, two reads of the
mask and 32 B per kept point).  One JSON line per measurement; --append PATH also appends them to PATH.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("icp-4dradar_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import icp4r  # noqa: E402
from icp4r import ego, reve, synth  # noqa: E402


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
    ap.add_argument("--el-deg", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=10)
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
        kw.update(scans=a.scans, points=a.points, dynamic=a.dynamic, el_deg=a.el_deg)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    # 16 distinct frames taken in turn: a longer drive leaves the synthetic scene behind the sensor, where the
    # azimuth filter drops every point
    base, _ = synth.make_sequence(77, frames=min(16, a.scans), n=a.points, dynamic=a.dynamic, el_deg=a.el_deg)
    frames = [base[s % len(base)] for s in range(a.scans)]
    ns, max_n = a.scans, a.points
    rec = np.concatenate(frames)
    cnt = np.full(ns, max_n, np.int32)
    off = np.arange(ns, dtype=np.int64) * max_n
    rec_d = torch.from_numpy(rec).to(dev)
    copy_d = torch.zeros_like(rec_d)
    off_d, cnt_d = torch.from_numpy(off).to(dev), torch.from_numpy(cnt).to(dev)
    res_d = torch.zeros((ns, 88), dtype=torch.uint8, device=dev)
    ego_res_d = torch.zeros((ns, 72), dtype=torch.uint8, device=dev)
    mask_d = torch.zeros(ns * max_n, dtype=torch.uint8, device=dev)
    clouds_d = torch.zeros((ns * max_n, 4), dtype=torch.float32, device=dev)
    poff_d = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    pn_d = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    p = reve.default_params(seed=2025)
    pe = ego.default_params(seed=2025)
    nbytes = ns * max_n * 20

    def estimator():
        reve.estimate_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n, res_d.data_ptr(),
                                   params=p, mask_ptr=mask_d.data_ptr(), ctx=ctx, stream=st)

    def estimator_pack():
        reve.inlier_clouds_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n, res_d.data_ptr(),
                                        clouds_d.data_ptr(), poff_d.data_ptr(), pn_d.data_ptr(), params=p,
                                        mask_ptr=mask_d.data_ptr(), ctx=ctx, stream=st)

    def sine_route():
        ego.static_clouds_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n,
                                       ego_res_d.data_ptr(), clouds_d.data_ptr(), poff_d.data_ptr(), pn_d.data_ptr(),
                                       params=pe, mask_ptr=mask_d.data_ptr(), ctx=ctx, stream=st)

    def d2d_copy():
        rc = hip.hipMemcpyAsync(copy_d.data_ptr(), rec_d.data_ptr(), nbytes, 3, st)  # hipMemcpyDeviceToDevice
        assert rc == 0, rc

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    sides = [("estimator", estimator), ("estimator_pack", estimator_pack), ("sine_route", sine_route),
             ("d2d_copy", d2d_copy)]
    for _ in range(2):
        for _, fn in sides:
            timed(fn)
    t = {name: [] for name, _ in sides}
    for _ in range(a.reps):
        for name, fn in sides:
            t[name].append(timed(fn))
    timed(estimator_pack)  # leave the estimator's own counts in pair_n / res
    res = np.frombuffer(res_d.cpu().numpy().tobytes(), dtype=reve.REVE_RESULT_DTYPE)
    kept = int(pn_d.cpu().numpy()[1:].sum())
    assert kept == int(res["n_inliers"].sum())
    med = {k: float(np.median(v)) for k, v in t.items()}
    records = ns * max_n
    own = records * 21
    own_pack = records * (21 + 16 + 2) + kept * 32
    emit(measurement="reve_batch", reps=a.reps, **{k: stats(v) for k, v in t.items()},
         pack_adds_ms=med["estimator_pack"] - med["estimator"],
         estimator_over_copy=med["estimator"] / med["d2d_copy"],
         estimator_pack_over_copy=med["estimator_pack"] / med["d2d_copy"],
         estimator_pack_over_sine_route=med["estimator_pack"] / med["sine_route"],
         copy_bytes=nbytes, copy_tb_per_s=2 * nbytes / (med["d2d_copy"] * 1e-3) / 1e12,
         estimator_bytes_by_own_account=own, estimator_tb_per_s=own / (med["estimator"] * 1e-3) / 1e12,
         estimator_pack_bytes_by_own_account=own_pack,
         estimator_pack_tb_per_s=own_pack / (med["estimator_pack"] * 1e-3) / 1e12,
         iterations=int(res["iterations"].max()), accepted_mean=float(res["accepted"].mean()),
         success_share=float(res["success"].mean()), valid_share=float(res["n_valid"].sum()) / records,
         kept_points=kept, kept_share=kept / records)
    ctx.close()
    if a.append:
        os.makedirs(os.path.dirname(os.path.abspath(a.append)), exist_ok=True)
        with open(a.append, "a") as f:
            for rec_ in lines:
                f.write(json.dumps(rec_) + "\n")


if __name__ == "__main__":
    main()
