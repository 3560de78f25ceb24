"""Reciprocal correspondences (setUseReciprocalCorrespondences) — what needs no GPU: the C ABI field, the
facades' getter / setter, and the numpy twin the GPU tests compare with (tests/reciprocal_twin.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_twin as tw
import reciprocal_twin as rt
from helpers import pose_err
from test_reciprocal_gpu import PARAMS, SHAPES, _lattice_pair as lattice_pair  # the GPU tests' own inputs

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


# ---- the C oracle's flag (oracle_params.use_reciprocal_correspondences) against the twin, both ways

def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _u64(x):
    return np.float64(x).view(np.uint64)


def assert_oracle_equals_twin(o, t, what=""):
    """F32: every reported field equal, T, fitness and the aligned xyz in bits."""
    got = (o["status"], o["iterations"], o["converged"], o["convergence_state"], o["n_correspondences"])
    want = (t["status"], t["iterations"], t["converged"], t["state"], t["n_correspondences"])
    assert got == want, (what, got, want, t["ncorr"])
    assert (_u32(o["T"]) == _u32(t["T"])).all(), (what, np.abs(o["T"] - t["T"]).max())
    assert _u64(o["fitness"]) == _u64(t["fitness"]), (what, o["fitness"], t["fitness"])
    assert (_u32(o["aligned"][:, :3]) == _u32(t["aligned"])).all(), what


def _oracle_on(oracle_mod, s, t, **kw):
    kw.setdefault("numerics", oracle_mod.NUM_F32)
    return oracle_mod.align(s, t, aligned=True, use_reciprocal_correspondences=1, **kw)


def test_oracle_params_layout(oracle_mod):
    """The flag is appended (with a pad) behind the fields every earlier caller sets, and is off by
    default."""
    P = oracle_mod.OracleParams
    assert P.use_reciprocal_correspondences.offset == P.eigen_gebp_mr.offset + 4
    assert C.sizeof(P) == P.use_reciprocal_correspondences.offset + 8
    assert oracle_mod.default_params().use_reciprocal_correspondences == 0


@pytest.mark.parametrize("kw", PARAMS, ids=["defaults", "iters7", "maxdist1"])
@pytest.mark.parametrize("seed,n,m", SHAPES)
def test_oracle_f32_equals_twin(oracle_mod, seed, n, m, kw):
    s, t = _pair(seed, n, m)
    tw_row = rt.icp(s, t, **kw)
    assert sum(tw_row["rejected"]) > 0
    for nn in (oracle_mod.NN_KDTREE, oracle_mod.NN_BRUTE):
        assert_oracle_equals_twin(_oracle_on(oracle_mod, s, t, nn=nn, **kw), tw_row, (seed, kw, nn))
    off = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, **kw)
    assert off["n_correspondences"] > tw_row["n_correspondences"]  # (the flag is what made the rows differ)


def test_oracle_f32_equals_twin_on_edge_pairs(oracle_mod):
    """Duplicated points (ties to the lowest index), five sources against one target (|C| = 1), one
    and two sources."""
    s, t = _pair(4100, 400, 300)
    for name, (ps, pt) in {"dup": dup_pair(), "5x1": (s[:5], t[:1]), "n1": (s[:1], t), "n2": (s[:2], t)}.items():
        tw_row = rt.icp(ps, pt)
        assert_oracle_equals_twin(_oracle_on(oracle_mod, ps, pt), tw_row, name)
        if name != "dup":
            assert (tw_row["status"], tw_row["state"], tw_row["iterations"]) == (-3, 5, 0), name
    assert rt.icp(s[:5], t[:1])["ncorr"] == [1]
    assert rt.icp(*dup_pair())["rejected"][0] >= 50


def test_oracle_lattice_pair_flag_on_equals_flag_off(oracle_mod):
    s, t = lattice_pair()
    tw_row = rt.icp(s, t)
    assert tw_row["iterations"] >= 2 and sum(tw_row["rejected"]) == 0
    on = _oracle_on(oracle_mod, s, t, trace=True)
    off = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, aligned=True, trace=True)
    assert_oracle_equals_twin(on, tw_row, "lattice")
    assert_oracle_equals_twin(off, tw_row, "lattice, flag off")
    assert (on["trace"]["ncorr"] == 1000).all() and (on["trace"]["ncorr"] == off["trace"]["ncorr"]).all()
    assert on["trace"]["T_inc"].tobytes() == off["trace"]["T_inc"].tobytes()


@pytest.mark.parametrize("huber", [np.inf, 0.5])
@pytest.mark.parametrize("seed,n,m", [(4000, 700, 650), (4001, 1024, 1024), (4003, 2048, 1500)])
def test_oracle_f64_matches_twin(oracle_mod, seed, n, m, huber):
    """F64 numerics, with and without Huber weights: equal counts, pose and fitness within the bars of
    test_oracle.test_icp_f64_matches_numpy_twin (2e-6 m / rad, 1e-9 relative to max(1, fitness))."""
    s, t = _pair(seed, n, m)
    tw_row = rt.icp(s, t, numerics="f64", huber_delta=huber)
    assert sum(tw_row["rejected"]) > 0
    rows = [_oracle_on(oracle_mod, s, t, numerics=oracle_mod.NUM_F64, huber_delta=huber, nn=nn, trace=True)
            for nn in (oracle_mod.NN_KDTREE, oracle_mod.NN_BRUTE)]
    o = rows[0]
    assert (o["status"], o["iterations"], o["converged"], o["convergence_state"]) == \
        (tw_row["status"], tw_row["iterations"], tw_row["converged"], tw_row["state"])
    assert o["n_correspondences"] == tw_row["n_correspondences"]
    assert list(o["trace"]["ncorr"]) == tw_row["ncorr"]
    dt, dr = pose_err(o["T"], tw_row["T"])
    assert dt < 2e-6 and dr < 2e-6, (dt, dr)
    assert abs(o["fitness"] - tw_row["fitness"]) <= 1e-9 * max(1.0, tw_row["fitness"])
    assert rows[0]["T"].tobytes() == rows[1]["T"].tobytes() and rows[0]["fitness"] == rows[1]["fitness"]
    assert rows[0]["aligned"].tobytes() == rows[1]["aligned"].tobytes()


@pytest.mark.parametrize("kw", [{}, {"max_correspondence_distance": 1.0}], ids=["defaults", "maxdist1"])
def test_oracle_guess_is_a_moved_source(oracle_mod, kw):
    """A guess G (the twin has none): the registration of (s, G) is the registration of G s without a
    guess: the same iterations, per-iteration |C| and increments in bits; only the accumulated T
    carries G."""
    s, t = _pair(4000, 700, 650)
    a = np.deg2rad(2.0)
    G = np.eye(4, dtype=np.float32)
    G[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    G[:3, 3] = (0.3, -0.2, 0.05)
    moved = s.copy()
    moved[:, :3] = tw.transform(G, s[:, :3])
    g = _oracle_on(oracle_mod, s, t, guess=G, trace=True, **kw)
    m = _oracle_on(oracle_mod, moved, t, trace=True, **kw)
    plain = _oracle_on(oracle_mod, s, t, trace=True, **kw)
    for k in ("status", "iterations", "converged", "convergence_state", "n_correspondences"):
        assert g[k] == m[k], k
    assert g["status"] == 0 and g["iterations"] >= 2
    assert (g["trace"]["ncorr"] == m["trace"]["ncorr"]).all() and (g["trace"]["ncorr"] < len(s)).all()
    assert g["trace"]["T_inc"].tobytes() == m["trace"]["T_inc"].tobytes()
    assert g["trace"]["mse"].tobytes() == m["trace"]["mse"].tobytes()
    assert not (g["T"] == m["T"]).all()
    assert g["trace"]["T_inc"][0].tobytes() != plain["trace"]["T_inc"][0].tobytes()  # (the guess matters)


@pytest.mark.parametrize("seed,n,m", [(4000, 700, 650), (4003, 2048, 1500)])
def test_votes_beyond_the_threshold_cannot_win(seed, n, m):
    """The key form with a threshold (1.0): a source whose own d2 exceeds max_d2 is no candidate, and
    its key (d2_i, i) at its target is larger than that of every candidate there, so whether it takes
    part in the election of a target's smallest key or not, the same candidates win (the device's vote
    leaves such sources out only to save the atomic).  The winners that then lose the bounded search
    are lost to a source that is nearer to the target than to its own."""
    s, t = _pair(seed, n, m)
    X, T = s[:, :3], t[:, :3]
    idx, d2 = tw.nearest(X, T)
    max_d2 = 1.0
    cand = d2.astype(np.float64) <= max_d2
    assert 0.1 * n < cand.sum() < 0.9 * n
    key = rt._key(d2, np.arange(n))

    def winners(voters):
        win = np.full(m, np.iinfo(np.uint64).max, np.uint64)
        np.minimum.at(win, idx[voters], key[voters])
        return cand & (win[idx] == key)

    with_all, with_cand = winners(np.ones(n, bool)), winners(cand)
    assert (with_all == with_cand).all()
    keep = rt.reciprocal_keep(X, T, idx, d2, max_d2)
    assert (keep <= with_cand).all() and keep.sum() < with_cand.sum()  # (the search rejects some winners)
    assert (keep == rt.reciprocal_keep_by_key(X, T, idx, d2, max_d2)).all()
