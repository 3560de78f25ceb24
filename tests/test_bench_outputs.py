"""bench.py's plain run, ``--full`` and ``--dump-outputs``: the options (CPU) and one small plain run
on the GPU whose dumped rows are compared with the same pairs registered through the host-batch call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_ONLY = ("roofline", "incl_upload", "cpu_baseline", "parity_check", "parity_ok", "c1", "c2", "c5",
             "cache_test_kernel")


def test_options():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d", "--no-c3"])
    assert a.full and a.dump_outputs == "d"
    for bad in (["--steps", "0"], ["--no-c3"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_rows(tmp_path, gpu_ctx):
    import icp4r
    from icp4r import synth

    P, n, iters = 6, 700, 5
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--pairs", str(P), "--points", str(n), "--iters", str(iters), "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(P * 1e3 / line["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]

    # the same pairs through the host-batch call: the library is bit-exact across its entry points
    src = np.concatenate([synth.make_pair(k, n).src_xyzi() for k in range(P)])
    tgt = np.concatenate([synth.make_pair(k, n).tgt_xyzi() for k in range(P)])
    off, cnt = np.arange(P, dtype=np.int64) * n, np.full(P, n, np.int32)
    params = icp4r.default_params(max_iterations=iters, mse_threshold_absolute=-1.0, transformation_epsilon=-1.0)
    ref = gpu_ctx.align_batch_host(src, off, cnt, tgt, off, cnt, params=params)
    T = np.load(tmp_path / "T.npy")
    assert T.dtype == np.float32 and T.shape == (P, 4, 4)
    assert (T == ref["T"].reshape(P, 4, 4).transpose(0, 2, 1)).all()
    fit = np.load(tmp_path / "fitness.npy")
    assert fit.dtype == np.float64 and (fit == ref["fitness"]).all()
    for name in ("iterations", "converged", "status", "convergence_state", "n_correspondences"):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float64 and (a == ref[name]).all(), name
    assert (np.load(tmp_path / "status.npy") == 0).all() and (np.load(tmp_path / "iterations.npy") == iters).all()
