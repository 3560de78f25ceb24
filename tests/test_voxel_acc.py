"""The incremental voxel grid on the CPU: the dictionary twin (tests/voxel_acc_twin.py) against the full
filter's twin (tests/voxel_grid_twin.py) on the concatenation, bit for bit after every add; the new
header against the Python layer's symbol list and the library's exports; the facade program compiling.
The library itself is compared with both twins on the GPU (tests/test_voxel_acc_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_acc_twin as acc_twin
import voxel_grid_twin as twin
import voxel_tools as tools
from voxel_tools import same_bits

ROOT = tools.ROOT
F = np.float32


def shifted(cloud, dx=0.0, dy=0.0, dz=0.0):
    c = np.array(cloud, F)
    c[:, :3] += np.array([dx, dy, dz], F)
    return c


def sequences():
    """name -> six adds."""
    radar = [twin.radar_cloud(700 + 300 * s, seed=40 + s) for s in range(6)]
    crowded = np.array_split(twin.crowded_cloud(), 6)
    negative = [shifted(twin.radar_cloud(500, seed=50 + s), dx=-35.0 * s, dy=-20.0 * s, dz=-3.0 * s) for s in range(6)]
    bad = [twin.radar_cloud(400, seed=60 + s) for s in range(6)]
    bad[1] = np.full((50, 4), np.nan, F)
    bad[2][7, 1] = np.inf
    bad[3][[0, 5, 399], [0, 2, 1]] = [np.nan, -np.inf, np.inf]
    zero = [np.array([[-0.0, -0.0, -0.0, -0.0]], F), np.array([[-0.0, 0.1, -0.0, 2.0], [0.2, -0.0, 0.1, -0.0]], F),
            np.array([[-0.3, -0.0, 0.2, 1.0]], F), np.array([[-0.0, -0.0, -0.0, -0.0]] * 3, F),
            np.array([[0.4, 0.4, 0.4, 5.0]], F), np.array([[-0.0, 0.0, -0.0, 0.0]], F)]
    return {"radar": radar, "crowded": crowded, "negative": negative, "non_finite": bad, "negative_zero": zero}


SEQS = sequences()
PARAMS = [(0.5, True, 0), ((0.3, 0.7, 1.1), True, 0), (0.5, True, 2), (0.5, False, 3), ((0.3, 0.7, 1.1), False, 2)]


@pytest.mark.parametrize("name", sorted(SEQS))
@pytest.mark.parametrize("leaf, all_data, min_pts", PARAMS)
def test_twin_equals_the_full_filter_after_every_add(name, leaf, all_data, min_pts):
    acc = acc_twin.VoxelAccumulatorTwin(leaf, all_data, min_pts)
    seen = np.zeros((0, 4), F)
    for scan in SEQS[name]:
        acc.add(scan)
        seen = np.concatenate([seen, twin.as_xyzi(scan)])
        want = twin.voxel_filter(seen, leaf, all_data, min_pts)
        assert same_bits(acc.filter(), want), name
        assert acc.filter().tobytes() == acc.filter().tobytes()
    assert acc.size()[1] == len(seen)


def test_negative_zero_first_member_gives_positive_zero():
    acc = acc_twin.VoxelAccumulatorTwin(1.0)
    acc.add(np.array([[-0.0, 0.25, 0.25, -0.0]], F))
    assert acc.filter().view(np.uint32)[0, [0, 3]].tolist() == [0, 0]


def test_overflow_reached_by_a_later_add():
    """tests/test_voxel.py's two overflow clouds, each as two adds: fine after the first point, refused
    after the second, by both twins; the state itself is undamaged."""
    from test_voxel import OVERFLOW_DIV, OVERFLOW_PCL

    for c in (OVERFLOW_PCL, OVERFLOW_DIV):
        acc = acc_twin.VoxelAccumulatorTwin(1.0)
        acc.add(c[:1])
        assert same_bits(acc.filter(), twin.voxel_filter(c[:1], 1.0))
        acc.add(c[1:])
        with pytest.raises(twin.GridOverflow):
            acc.filter()
        with pytest.raises(twin.GridOverflow):
            twin.voxel_filter(c, 1.0)
        assert acc.size() == (2, 2)


def test_range_rule():
    acc = acc_twin.VoxelAccumulatorTwin(0.5)
    first = twin.radar_cloud(100, seed=70)
    acc.add(first)
    far = shifted(first, dx=0.5 * 2**20 + 100.0)
    with pytest.raises(acc_twin.RangeError):
        acc.add(far)
    assert same_bits(acc.filter(), twin.voxel_filter(first, 0.5)) and acc.size()[1] == 100
    inside = shifted(first[:10], dx=-0.5 * 2**20 + 200.0)  # down to offset -2^20 + about 400
    acc.add(inside)
    assert acc.size()[1] == 110


# ---- header, Python layer, library
def test_header_declares_and_library_exports_the_entries():
    import icp4r

    hdr = open(os.path.join(ROOT, "include", "icp4r", "icp4r_voxel_acc.h")).read()
    decl = re.findall(r"^\s*int\s+(icp4r_\w+)\s*\(", hdr, re.M)
    want = sorted(["icp4r_voxel_acc_create", "icp4r_voxel_acc_destroy", "icp4r_voxel_acc_clear", "icp4r_voxel_acc_reserve",
                   "icp4r_voxel_acc_add", "icp4r_voxel_acc_add_device", "icp4r_voxel_acc_add_map", "icp4r_voxel_acc_filter",
                   "icp4r_voxel_acc_filter_device", "icp4r_voxel_acc_size"])
    assert sorted(decl) == want and sorted(icp4r.VOXEL_ACC_EXPORTED_SYMBOLS) == want
    L = icp4r.load()
    out = subprocess.run(["nm", "-D", "--defined-only", icp4r.library_path], capture_output=True, text=True).stdout
    for name in want:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}$", out, re.M), name  # unmangled: C linkage
        assert getattr(L, name).argtypes is not None, name
    assert L.icp4r_abi_version() == 6
    # the filter's header declares what it declared
    vox = open(os.path.join(ROOT, "include", "icp4r", "icp4r_voxel.h")).read()
    assert sorted(re.findall(r"^\s*int\s+(icp4r_\w+)\s*\(", vox, re.M)) == sorted(icp4r.VOXEL_EXPORTED_SYMBOLS)
    assert len(icp4r.VOXEL_EXPORTED_SYMBOLS) == 7 and "voxel_acc" not in vox
    assert '#include "icp4r/icp4r_voxel.h"' in hdr


def test_python_layer():
    from icp4r import voxel

    for name in ("add", "add_device", "add_map", "filter", "filter_device", "size", "clear", "reserve", "close"):
        assert callable(getattr(voxel.VoxelAccumulator, name)), name
    assert C.sizeof(voxel.VoxelParams) == 20


@pytest.mark.parametrize("pcl18", [False, True])
def test_facade_program_compiles(tmp_path, pcl18):
    """tests/cpp/voxel_acc_callsite.cpp against voxel_acc_compat.hpp, with the facade's own point types
    and with the PCL-1.8-shaped include tree."""
    compile_acc_callsite(tmp_path, pcl18)
    text = open(os.path.join(tools.CPP, "voxel_acc_callsite.cpp")).read()
    for line in ("icp4r::IncrementalVoxelGrid<pcl::PointXYZI> grid;", "grid.setLeafSize(0.5f, 0.5f, 0.5f);",
                 "grid.addCloud(scan);", "grid.filter(*downSizeFilterMap);"):
        assert line in text


def compile_acc_callsite(out_dir, pcl18: bool) -> str:
    """voxel_tools.callsite_command's command, for tests/cpp/voxel_acc_callsite.cpp."""
    exe, cmd = tools.callsite_command(out_dir, pcl18)
    exe = exe.replace("voxel_callsite", "voxel_acc_callsite")
    cmd = [exe if a.endswith(("voxel_callsite", "voxel_callsite_pcl18")) else a.replace("voxel_callsite.cpp", "voxel_acc_callsite.cpp")
           for a in cmd]
    assert exe in cmd and any(a.endswith("voxel_acc_callsite.cpp") for a in cmd)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe
