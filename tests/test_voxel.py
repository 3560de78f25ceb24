"""Voxel-grid downsampling on the CPU: the contract's numpy twin (tests/voxel_grid_twin.py) against
hand-computed answers and, bit for bit, against the independently written C++ restatement of PCL's
loop (tests/cpp/voxel_host_check.cpp, compiled here with g++ -O2 -ffp-contract=off); the new header
against the Python layer's symbol list and the library's exports; the node's call text compiling
against the facade.  The library itself is compared with the twin on the GPU (tests/test_voxel_gpu.py).
Every comparison is of whole arrays: count, order and bits."""
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_grid_twin as twin
import voxel_tools as tools
from voxel_tools import same_bits

ROOT = tools.ROOT
F = np.float32


def pts(*rows):
    return np.array(rows, F).reshape(-1, 4)


# ---- the twin against known answers
def test_one_point_is_its_own_centroid():
    c = pts([1.2, 3.4, -5.6, 7.0])
    assert same_bits(twin.voxel_filter(c, 0.5), c)


def test_two_points_in_one_voxel():
    c = pts([0.25, 0.25, 0.25, 2.0], [0.75, 0.5, 0.25, 4.0])
    assert same_bits(twin.voxel_filter(c, 1.0), pts([0.5, 0.375, 0.25, 3.0]))


def test_points_on_leaf_faces_belong_to_the_upper_cell():
    """x = k * leaf lies in cell k, for both signs; the float just below 0.5 is still cell 0."""
    xs = [1.0, -0.5, 0.0, 0.5, -1.0]
    c = pts(*[[x, 0.1, 0.1, float(i)] for i, x in enumerate(xs)])
    out = twin.voxel_filter(c, 0.5)
    assert same_bits(out, c[[4, 1, 2, 3, 0]])  # five voxels, ascending x
    below = np.nextafter(F(0.5), F(0.0))
    c2 = pts([0.0, 0.1, 0.1, 1.0], [below, 0.1, 0.1, 3.0], [0.5, 0.1, 0.1, 5.0])
    want = pts([(F(0.0) + below) / F(2), (F(0.1) + F(0.1)) / F(2), (F(0.1) + F(0.1)) / F(2), 2.0], [0.5, 0.1, 0.1, 5.0])
    assert same_bits(twin.voxel_filter(c2, 0.5), want)


def test_negative_zero_sums_to_positive_zero():
    """s = +0.0f; s += -0.0f is +0.0f: the centroid of a lone -0.0 is +0.0."""
    c = pts([-0.0, 0.25, 0.25, -0.0])
    out = twin.voxel_filter(c, 1.0)
    assert out.view(np.uint32).tolist() == [[0, F(0.25).view(np.uint32), F(0.25).view(np.uint32), 0]]


def test_negative_coordinates_use_floor_not_truncation():
    c = pts([0.25, 0.25, 0.25, 1.0], [-0.25, 0.25, 0.25, 2.0])  # truncation would put both in cell 0
    assert same_bits(twin.voxel_filter(c, 1.0), c[[1, 0]])


SIZES = pts(*([[0.5, 0.5, 0.5, 1.0]] * 1 + [[1.5, 0.5, 0.5, 2.0]] * 2 + [[2.5, 0.5, 0.5, 3.0]] * 5))


@pytest.mark.parametrize("min_pts, want", [(0, [1.0, 2.0, 3.0]), (1, [1.0, 2.0, 3.0]), (2, [2.0, 3.0]), (5, [3.0]), (6, [])])
def test_min_points_per_voxel(min_pts, want):
    out = twin.voxel_filter(SIZES, 1.0, min_points_per_voxel=min_pts)
    assert out[:, 3].tolist() == want and out.shape == (len(want), 4)


def test_downsample_all_data_off_zeroes_the_intensity():
    c = pts([0.25, 0.25, 0.25, 2.0], [0.75, 0.5, 0.25, 4.0])
    assert same_bits(twin.voxel_filter(c, 1.0, downsample_all_data=False), pts([0.5, 0.375, 0.25, 0.0]))


def test_non_finite_points_are_skipped():
    c = pts([0.25, 0.25, 0.25, 2.0], [np.nan, 0.25, 0.25, 9.0], [0.75, 0.5, 0.25, 4.0], [0.3, 0.3, np.inf, 9.0],
            [0.3, -np.inf, 0.3, 9.0])
    assert same_bits(twin.voxel_filter(c, 1.0), pts([0.5, 0.375, 0.25, 3.0]))
    assert twin.voxel_filter(np.full((7, 4), np.nan, F), 1.0).shape == (0, 4)
    assert twin.voxel_filter(np.zeros((0, 4), F), 1.0).shape == (0, 4)


def test_anisotropic_leaf_with_inexact_inverse():
    """leaf (0.3, 0.5, 1.0): inv0 = fl(1 / 0.3f) is inexact; cells by floorf(p * inv)."""
    leaf = np.array([0.3, 0.5, 1.0], F)
    inv0 = F(1.0) / leaf[0]
    assert np.floor(F(0.29) * inv0) == 0 and np.floor(F(0.31) * inv0) == 1
    c = pts([0.31, 0.51, 1.01, 5.0], [0.01, 0.01, 0.01, 1.0], [0.29, 0.49, 0.99, 3.0])
    mean = [(F(a) + F(b)) / F(2) for a, b in ((0.01, 0.29), (0.01, 0.49), (0.01, 0.99), (1.0, 3.0))]
    assert same_bits(twin.voxel_filter(c, leaf), pts(mean, [0.31, 0.51, 1.01, 5.0]))
    # a 12-byte point has intensity 0
    assert same_bits(twin.voxel_filter(c[:, :3], leaf)[:, 3], np.zeros(2, F))


OVERFLOW_PCL = pts([0.0, 0.0, 0.0, 1.0], [1300.0, 1300.0, 1300.0, 2.0])       # d = 1301^3: PCL's own check
OVERFLOW_DIV = pts([0.9, 0.9, 0.9, 1.0], [1290.1, 1290.1, 1290.1, 2.0])       # d = 1290^3 passes, div = 1291^3


def test_grid_overflow_examples():
    for c in (OVERFLOW_PCL, OVERFLOW_DIV):
        with pytest.raises(twin.GridOverflow):
            twin.voxel_filter(c, 1.0)
    # the second example passes PCL's check and overflows div only
    lo, hi = OVERFLOW_DIV[0, :3], OVERFLOW_DIV[1, :3]
    d = [int((h - l) * F(1.0)) + 1 for l, h in zip(lo, hi)]
    div = [int(np.floor(h)) - int(np.floor(l)) + 1 for l, h in zip(lo, hi)]
    assert d == [1290] * 3 and 1290**3 <= 2**31 - 1 and div == [1291] * 3 and 1291**3 > 2**31 - 1
    # just inside: 1290^3 cells
    ok = pts([0.1, 0.1, 0.1, 1.0], [1289.9, 1289.9, 1289.9, 2.0])
    assert same_bits(twin.voxel_filter(ok, 1.0), ok)


# ---- the twin against the C++ restatement of PCL's loop, bit for bit
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return tools.compile_host_check(tmp_path_factory.mktemp("voxel_host_check"))


def with_non_finite(c, seed=3):
    c = c.copy()
    r = np.random.default_rng(seed)
    rows = r.choice(len(c), len(c) // 50, replace=False)
    c[rows, r.integers(0, 3, len(rows))] = np.array([np.nan, np.inf, -np.inf], F)[r.integers(0, 3, len(rows))]
    return c


@pytest.mark.parametrize("n", [1, 2, 4097, 20011])
def test_twin_equals_host_check_on_radar_clouds(host_check, tmp_path, n):
    c = twin.radar_cloud(n, seed=n)
    for leaf, all_data, min_pts in ((0.5, True, 0), ((0.3, 0.5, 1.0), False, 2), (2.0, True, 5)):
        got, _ = tools.run_host_check(host_check, tmp_path, c, leaf, all_data, min_pts)
        assert same_bits(got, twin.voxel_filter(c, leaf, all_data, min_pts)), (n, leaf)
    if n > 100:
        cn = with_non_finite(c)
        got, _ = tools.run_host_check(host_check, tmp_path, cn, 0.5)
        want = twin.voxel_filter(cn, 0.5)
        assert same_bits(got, want) and 0 < len(want) < n


def test_twin_equals_host_check_on_crowded_voxels(host_check, tmp_path):
    """50 sites x 40 jittered copies: centroids of many members, where the member order reaches the bits
    (reversing the input changes them, so a restatement with another order would not pass)."""
    c = twin.crowded_cloud()
    want = twin.voxel_filter(c, 0.5)
    got, _ = tools.run_host_check(host_check, tmp_path, c, 0.5)
    assert same_bits(got, want) and len(want) <= 50 and len(want) >= 40
    rev = twin.voxel_filter(c[::-1], 0.5)
    assert rev.shape == want.shape and (rev.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum() > len(want) // 4


def test_host_check_reports_both_overflows(host_check, tmp_path):
    for c in (OVERFLOW_PCL, OVERFLOW_DIV):
        got, _ = tools.run_host_check(host_check, tmp_path, c, 1.0)
        assert got is None


# ---- header, Python layer, library
def test_header_declares_and_library_exports_the_entries():
    import icp4r

    hdr = open(os.path.join(ROOT, "include", "icp4r", "icp4r_voxel.h")).read()
    decl = re.findall(r"^\s*int\s+(icp4r_\w+)\s*\(", hdr, re.M)
    want = sorted(["icp4r_voxel_params_default", "icp4r_voxel_filter", "icp4r_voxel_filter_device",
                   "icp4r_map_voxel_filter", "icp4r_map_voxel_filter_device", "icp4r_voxel_time_ms",
                   "icp4r_voxel_time_reset"])
    assert sorted(decl) == want and sorted(icp4r.VOXEL_EXPORTED_SYMBOLS) == want
    L = icp4r.load()
    out = subprocess.run(["nm", "-D", "--defined-only", icp4r.library_path], capture_output=True, text=True).stdout
    for name in want:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}$", out, re.M), name  # unmangled: C linkage
        assert getattr(L, name).argtypes is not None, name
    assert L.icp4r_abi_version() == 6
    # the map headers' entry lists are as they were
    for h in ("icp4r_map.h", "icp4r_map_knn.h"):
        assert "voxel" not in open(os.path.join(ROOT, "include", "icp4r", h)).read()


def test_params_default_and_python_layer():
    from icp4r import mapstore, voxel

    p = voxel.voxel_params()
    assert list(p.leaf) == [0.0, 0.0, 0.0] and p.downsample_all_data == 1 and p.min_points_per_voxel == 0
    import ctypes as C
    assert C.sizeof(voxel.VoxelParams) == 20
    for name in ("setInputCloud", "setLeafSize", "setDownsampleAllData", "setMinimumPointsNumberPerVoxel", "filter",
                 "filter_device"):
        assert callable(getattr(voxel.VoxelGrid, name)), name
    for name in ("voxel_filter", "voxel_filter_device"):
        assert callable(getattr(mapstore.KD_TREE, name)), name


@pytest.mark.parametrize("pcl18", [False, True])
def test_reference_call_text_compiles(tmp_path, pcl18):
    """tests/cpp/voxel_callsite.cpp — the node's four lines — against voxel_compat.hpp, with the facade's
    own point types and with the PCL-1.8-shaped include tree."""
    tools.compile_callsite(tmp_path, pcl18)
    text = open(os.path.join(tools.CPP, "voxel_callsite.cpp")).read()
    for line in ("pcl::VoxelGrid<pcl::PointXYZI> sor;", "sor.setInputCloud(RadarCloudMap);",
                 "sor.setLeafSize(0.5f, 0.5f, 0.5f);", "sor.filter(*downSizeFilterMap);"):
        assert line in text
