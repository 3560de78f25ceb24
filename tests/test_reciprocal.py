"""Reciprocal correspondences (setUseReciprocalCorrespondences) — what needs no GPU: the C ABI field, the
facades' getter / setter, and the numpy twin the GPU tests compare with (tests/reciprocal_twin.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_twin as tw
import reciprocal_twin as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icp-4dradar_amd", "icp4r", "_lib")
PARAMS_BYTES = 112  # sizeof(icp4r_params) of ABI 6, before and after the field


def _pair(seed, n, m):
    from icp4r import synth

    p = synth.make_pair(seed, n, m)
    return p.src_xyzi(), p.tgt_xyzi()


def dup_pair():
    """A 400 x 300 pair with 50 duplicated sources and 40 duplicated targets appended."""
    s, t = _pair(4100, 400, 300)
    return np.concatenate([s, s[:50]]), np.concatenate([t, t[:40]])


def test_default_is_off_and_abi_unchanged():
    import icp4r

    p = icp4r.default_params()
    assert p.use_reciprocal_correspondences == 0
    assert icp4r.load().icp4r_abi_version() == 6


def test_struct_size_unchanged():
    """icp4r_params_default clears exactly sizeof(icp4r_params) bytes: the field came out of reserved[]."""
    import icp4r

    assert C.sizeof(icp4r.Params) == PARAMS_BYTES
    buf = (C.c_ubyte * 256)(*([0xAB] * 256))
    icp4r.load().icp4r_params_default(C.cast(buf, C.POINTER(icp4r.Params)))
    raw = bytes(buf)
    assert raw[PARAMS_BYTES:] == b"\xab" * (256 - PARAMS_BYTES)
    assert raw[PARAMS_BYTES - 24:PARAMS_BYTES] == b"\0" * 24  # the flag and reserved[5]
    assert icp4r.Params.use_reciprocal_correspondences.offset == PARAMS_BYTES - 24
    assert icp4r.Params.reserved.size == 20


@pytest.mark.parametrize("value", [2, -1, 256])
def test_invalid_value_is_refused_without_a_device(value):
    import icp4r

    ctx = icp4r.Context(icp4r.NO_DEVICE)
    try:
        s, t = _pair(4000, 16, 16)
        with pytest.raises(icp4r.ICP4RError) as e:
            ctx.align(s, t, icp4r.default_params(use_reciprocal_correspondences=value))
        assert e.value.code == icp4r.E_INVALID
        with pytest.raises(icp4r.ICP4RError) as e:
            ctx.align_batch_host(s, [0], [16], t, [0], [16], icp4r.default_params(use_reciprocal_correspondences=value))
        assert e.value.code == icp4r.E_INVALID
    finally:
        ctx.close()


def test_python_facade_getter_and_setter():
    import icp4r

    icp = icp4r.IterativeClosestPoint()
    assert icp.getUseReciprocalCorrespondences() is False
    icp.setUseReciprocalCorrespondences(True)
    assert icp.getUseReciprocalCorrespondences() is True and icp.params().use_reciprocal_correspondences == 1
    icp.setUseReciprocalCorrespondences(False)
    assert icp.getUseReciprocalCorrespondences() is False and icp.params().use_reciprocal_correspondences == 0


def test_cpp_facade_getter_and_setter(tmp_path):
    """pcl_compat.hpp: the flag set and read back (no device: the context is created at align)."""
    src = tmp_path / "recip_facade.cpp"
    src.write_text(
        '#include <icp4r/pcl_compat.hpp>\n'
        'int main() {\n'
        '    pcl::IterativeClosestPoint<pcl::PointXYZI, pcl::PointXYZI> icp;\n'
        '    if (icp.getUseReciprocalCorrespondences()) return 1;\n'
        '    icp.setUseReciprocalCorrespondences(true);\n'
        '    if (!icp.getUseReciprocalCorrespondences()) return 2;\n'
        '    icp.setUseReciprocalCorrespondences(false);\n'
        '    if (icp.getUseReciprocalCorrespondences()) return 3;\n'
        '    icp4r_params p;\n'
        '    icp4r_params_default(&p);\n'
        '    return p.use_reciprocal_correspondences == 0 && sizeof(p) == %d ? 0 : 4;\n'
        '}\n' % PARAMS_BYTES)
    exe = tmp_path / "recip_facade"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/include", "-o", str(exe), str(src),
                        f"-L{LIB}", "-licp4r", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert subprocess.run([str(exe)], timeout=60).returncode == 0


@pytest.mark.parametrize("seed,n,m", [(4000, 700, 650), (4002, 600, 900)])
def test_twin_with_the_flag_off_is_numpy_twin(seed, n, m):
    s, t = _pair(seed, n, m)
    a = rt.icp(s, t, reciprocal=False)
    b = tw.icp(s, t, numerics="f32")
    assert (a["T"].view(np.uint32) == b["T"].view(np.uint32)).all()
    assert a["fitness"] == b["fitness"]
    assert (a["iterations"], a["converged"], a["state"]) == (b["iterations"], b["converged"], b["state"])
    assert a["ncorr"] == [tr["ncorr"] for tr in b["trace"]]


def test_direct_definition_equals_the_key_form_on_duplicates():
    """The reverse-search definition and "no source has a smaller (d2, index) key at the target", on
    every iteration of a pair with 50 duplicated sources and 40 duplicated targets; a duplicated source
    keeps only its lowest index."""
    s, t = dup_pair()
    o = rt.icp(s, t, max_iterations=6, check_forms=True)
    assert o["iterations"] >= 1 and o["ncorr"][0] >= 3
    X, T = s[:, :3], t[:, :3]
    idx, d2 = tw.nearest(X, T)
    keep = rt.reciprocal_keep(X, T, idx, d2, rt.DBL_MAX)
    assert (keep == rt.reciprocal_keep_by_key(X, T, idx, d2, rt.DBL_MAX)).all()
    assert not keep[400:].any()  # the copies of sources 0..49 carry the higher index


def test_the_synthetic_pairs_really_reject():
    """Seeds 4000-4005 (the GPU tests' inputs): the first iteration keeps between 50 % and 95 % of the
    sources and at least 3 — fixed with the twin alone, so a drift of icp4r.synth cannot hollow the GPU
    tests out."""
    shapes = [(700, 650), (1024, 1024), (600, 900), (2048, 1500), (900, 2048), (900, 2048)]
    for k, (n, m) in enumerate(shapes):
        s, t = _pair(4000 + k, n, m)
        X, T = s[:, :3], t[:, :3]
        idx, d2 = tw.nearest(X, T)
        kept = int(rt.reciprocal_keep(X, T, idx, d2, rt.DBL_MAX).sum())
        assert kept >= 3 and 0.50 * n <= kept <= 0.95 * n, (4000 + k, n, m, kept)
