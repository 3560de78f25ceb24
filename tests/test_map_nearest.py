"""Nearest_Search on the CPU: the contract's numpy twin (tests/map_nearest_twin.py) against what the
reference's own ikd-Tree answered (tests/golden/ikd_nearest.npz, make_ikd_nearest_golden.md), known
answers of the twin, and the reference's call text compiling against the facade.  The store itself
is compared with the twin on the GPU (tests/test_map_nearest_gpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import map_nearest_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB = os.path.join(ROOT, "icp-4dradar_amd", "icp4r", "_lib")
F = np.float32
CASES = "abc"


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "ikd_nearest.npz"))


def searches(g):
    return [(int(k), float(md)) for k, md in zip(g["searches_k"], g["searches_max_dist"])]


@pytest.mark.parametrize("case", CASES)
def test_twin_matches_reference_fixture(fixture, case):
    """Distances bit-equal and found equal for every query; indices equal for every untied query."""
    g = fixture
    store, queries = g[f"{case}_store"], g[f"{case}_queries"]
    for s, (k, md) in enumerate(searches(g)):
        _, dist, idx, found = twin.nearest_search(store, queries, k, md)
        assert (found == g[f"{case}_found_{s}"]).all(), (case, s)
        assert (dist.view(np.uint32) == g[f"{case}_dist_{s}"].view(np.uint32)).all(), (case, s)
        untied = np.array([not twin.tied(store, q, k) for q in queries])
        assert (idx[untied] == g[f"{case}_index_{s}"][untied]).all(), (case, s)


def test_fixture_conditions(fixture):
    """What make_ikd_nearest_golden.md promises of the recording: the cases' sizes, the searches, queries
    outside the map, rows with 0, with fewer than k and with k answers, and at most 1e-3 of the queries per
    case tied (their count recorded by the generator, recounted here)."""
    g = fixture
    assert searches(g) == [(20, np.inf), (20, 3.0), (20, 0.7), (5, np.inf), (1, np.inf)]
    assert len(g["a_store"]) == 1400 and len(g["b_store"]) < 14000 and 1400 < len(g["c_store"]) < 4400
    for case in CASES:
        store, queries = g[f"{case}_store"], g[f"{case}_queries"]
        assert queries.shape == (300, 3) and (np.abs(queries[:, :2]).max(axis=1) > 50).any()
        ids = store[:, 3]
        assert (np.diff(ids) > 0).all()  # survivors in insertion order
        for s, (k, md) in enumerate(searches(g)):
            ties = sum(twin.tied(store, q, k) for q in queries)
            assert ties == g[f"{case}_ties"][s] and ties <= 1e-3 * len(queries)
            found, idx = g[f"{case}_found_{s}"], g[f"{case}_index_{s}"]
            assert ((idx >= 0).sum(axis=1) == found).all()
        f3, f07 = g[f"{case}_found_1"], g[f"{case}_found_2"]
        assert (f3 == 0).any() and ((f3 > 0) & (f3 < 20)).any() and (f07 == 0).any()
        assert (g[f"{case}_found_0"] == 20).all()
    assert (g["b_found_1"] == 20).any()
    # case b deleted something and case c downsampled something away
    assert len(g["b_store"]) < 5000 + 3 * 3000 and len(g["c_store"]) < 1400 + 3000


def test_twin_known_answers():
    store = np.array([[3, 4, 0, 7], [0, 0, 12, 8], [100, 0, 0, 9]], F)
    q = np.zeros((1, 3), F)
    # a 3-4-5 lattice point with max_dist = 5 is kept (25 <= 25.0), one ulp below it is dropped
    _, d, i, f = twin.nearest_search(store, q, 2, 5.0)
    assert f[0] == 1 and i[0, 0] == 0 and d[0, 0] == 25.0 and i[0, 1] == -1 and np.isinf(d[0, 1])
    _, d, i, f = twin.nearest_search(store, q, 2, np.nextafter(5.0, 0.0))
    assert f[0] == 0
    # a negative max_dist acts as its magnitude (the reference squares it), NaN finds nothing
    p, d, i, f = twin.nearest_search(store, q, 3, -13.0)
    assert f[0] == 2 and i[0].tolist() == [0, 1, -1] and d[0, :2].tolist() == [25.0, 144.0]
    assert (p[0, 1] == store[1]).all() and (p[0, 2] == 0).all()
    assert twin.nearest_search(store, q, 3, np.nan)[3][0] == 0
    # a distance that overflows to +inf is a candidate of an infinite max_dist only
    far = np.array([[3e38, 0, 0, 1], [1, 0, 0, 2]], F)
    qq = np.array([[-3e38, 0, 0]], F)
    _, d, i, f = twin.nearest_search(far, qq, 2, np.inf)
    assert f[0] == 2 and np.isinf(d[0]).all() and i[0].tolist() == [0, 1]
    assert twin.nearest_search(far, qq, 2, 1e150)[3][0] == 0  # 1e300 in double: finite
    # stored points and queries with a non-finite coordinate
    bad = np.array([[np.nan, 0, 0, 1], [np.inf, 0, 0, 2], [1, 1, 1, 3]], F)
    _, d, i, f = twin.nearest_search(bad, q, 3)
    assert f[0] == 1 and i[0].tolist() == [2, -1, -1]
    assert twin.nearest_search(store, np.array([[0, np.nan, 0]], F), 1)[3][0] == 0
    # ties resolve to the lowest index; an empty store
    same = np.ones((5, 4), F)
    assert twin.nearest_search(same, q, 3)[2][0].tolist() == [0, 1, 2]
    assert twin.nearest_search(np.zeros((0, 4), F), q, 3)[3][0] == 0


def test_twin_is_the_unfused_float_expression():
    """calc_dist rounds after every operation: a case where the fused and the double results differ."""
    rng = np.random.default_rng(5)
    store = np.concatenate([rng.uniform(-50, 50, (4000, 3)), np.zeros((4000, 1))], axis=1).astype(F)
    q = rng.uniform(-50, 50, 3).astype(F)
    d = twin.calc_dist(q, store)
    dd = ((q.astype(np.float64) - store[:, :3].astype(np.float64)) ** 2).sum(axis=1)
    assert (d != dd.astype(F)).any()  # double then rounded is another number somewhere
    e = (q - store[:, :3]).astype(F)
    ref = np.array([F(F(F(a * a) + F(b * b)) + F(c * c)) for a, b, c in e], F)
    assert (d.view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("pcl18", [False, True])
def test_reference_call_text_compiles(tmp_path, pcl18):
    """tests/cpp/nearest_callsite.cpp — the reference's Nearest_Search call text — against ikd_compat.hpp,
    with the facade's own point types and with the PCL-1.8-shaped include tree."""
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *([f"-I{CPP}/pcl18"] if pcl18 else []), f"-I{ROOT}/include",
           "-o", str(tmp_path / "nearest_callsite"), os.path.join(CPP, "nearest_callsite.cpp"), f"-L{LIB}", "-licp4r",
           f"-Wl,-rpath,{LIB}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_python_layer_names_the_reference_call():
    from icp4r import mapstore

    for name in ("Nearest_Search", "nearest_search", "nearest_search_device", "index_build", "index_stats"):
        assert callable(getattr(mapstore.KD_TREE, name)), name
    assert mapstore.KNN_MAX_K == 32 and mapstore.KNN_BRUTE == 1


def test_header_declares_and_library_exports_the_entries():
    """include/icp4r/icp4r_map_knn.h (included by icp4r_map.h) declares the four entries, the Python
    layer lists and prototypes them, the library exports them with C linkage, and the ABI version stays."""
    import re

    import icp4r

    hdr = os.path.join(ROOT, "include", "icp4r")
    decl = re.findall(r"^\s*int\s+(icp4r_\w+)\s*\(", open(os.path.join(hdr, "icp4r_map_knn.h")).read(), re.M)
    want = ["icp4r_map_index_build", "icp4r_map_index_stats", "icp4r_map_nearest_search",
            "icp4r_map_nearest_search_device"]
    assert sorted(decl) == want and sorted(icp4r.MAP_KNN_EXPORTED_SYMBOLS) == want
    assert re.search(r'^#include "icp4r/icp4r_map_knn.h"', open(os.path.join(hdr, "icp4r_map.h")).read(), re.M)
    L = icp4r.load()
    out = subprocess.run(["nm", "-D", "--defined-only", icp4r.library_path], capture_output=True, text=True).stdout
    for name in want:
        assert hasattr(L, name), name
        assert re.search(rf"\bT {name}$", out, re.M), name
        assert getattr(L, name).argtypes is not None, name
    assert L.icp4r_abi_version() == 6
