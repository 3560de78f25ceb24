"""Helpers of the voxel-grid tests: compiling and running tests/cpp/voxel_host_check.cpp (the C++
restatement) and tests/cpp/voxel_callsite.cpp (the node's call text against the facade)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB = os.path.join(ROOT, "icp-4dradar_amd", "icp4r", "_lib")
F = np.float32


def compile_host_check(out_dir) -> str:
    exe = os.path.join(str(out_dir), "voxel_host_check")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
           os.path.join(CPP, "voxel_host_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def read_result(path):
    """-> (K, 4) float32, or None on grid overflow (K = -1)."""
    raw = open(path, "rb").read()
    k = int(np.frombuffer(raw[:8], np.int64)[0])
    if k < 0:
        return None
    return np.frombuffer(raw[8:], F).reshape(k, 4).copy()


def run_host_check(exe, work_dir, cloud, leaf, downsample_all_data=True, min_points_per_voxel=0):
    """cloud: (N, 4) float32.  -> (result or None on overflow, the filter's wall time in ms)."""
    src, dst = os.path.join(str(work_dir), "in.bin"), os.path.join(str(work_dir), "out.bin")
    np.ascontiguousarray(cloud, F).tofile(src)
    leaf = np.broadcast_to(np.asarray(leaf, F).reshape(-1), (3,))
    cmd = [exe, src, dst, *[f"{float(v):.9g}" for v in leaf], str(int(bool(downsample_all_data))),
           str(int(min_points_per_voxel))]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return read_result(dst), float(r.stdout.split()[0])


def callsite_command(out_dir, pcl18: bool):
    exe = os.path.join(str(out_dir), "voxel_callsite_pcl18" if pcl18 else "voxel_callsite")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *([f"-I{CPP}/pcl18"] if pcl18 else []), f"-I{ROOT}/include",
           "-o", exe, os.path.join(CPP, "voxel_callsite.cpp"), f"-L{LIB}", "-licp4r", f"-Wl,-rpath,{LIB}"]
    return exe, cmd


def compile_callsite(out_dir, pcl18: bool) -> str:
    exe, cmd = callsite_command(out_dir, pcl18)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def same_bits(a, b) -> bool:
    """Whole arrays: count, order and bits."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
