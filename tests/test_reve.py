"""The 3D Doppler ego-velocity estimator, the parts that need no GPU (include/icp4r/icp4r_reve.h): the
ABI of the new header, the node's settings, the two pure-host entries against the twin
(tests/reve_twin.py), the twin's own arithmetic against numpy's eigenvalues and solver, the twin's
known answers on the synthetic sequences (recorded here; tests/test_reve_gpu.py holds the device to
them), the facade's call-site program and the host arithmetic under ASan + UBSan as a stand-alone
program."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import reve_twin
from icp4r import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REVE_HEADER = os.path.join(ROOT, "include", "icp4r", "icp4r_reve.h")
E_INVALID, E_TOO_LARGE = -1, -8


def header_functions(path):
    return sorted(set(re.findall(r"^\s*(?:int32_t|int|void)\s+(icp4r_\w+)\s*\(", open(path).read(), re.M)))


def test_reve_abi():
    import icp4r
    from icp4r import reve

    L = icp4r.load()
    decl = header_functions(REVE_HEADER)
    for name in ("icp4r_reve_params_default", "icp4r_reve_ransac_iterations", "icp4r_reve_draw",
                 "icp4r_reve_batch_device", "icp4r_reve_inlier_clouds_batch_device", "icp4r_reve_estimate",
                 "icp4r_reve_inlier_cloud"):
        assert name in decl
    assert sorted(icp4r.REVE_EXPORTED_SYMBOLS) == decl
    assert L.icp4r_abi_version() == 6
    out = subprocess.run(["nm", "-D", "--defined-only", icp4r.library_path], capture_output=True, text=True).stdout
    for name in decl:
        assert re.search(rf"\bT {name}$", out, re.M), name  # unmangled: C linkage
    # nothing of the new header is in another header's list
    for other in (icp4r.EXPORTED_SYMBOLS, icp4r.EGO_EXPORTED_SYMBOLS, icp4r.GATE_EXPORTED_SYMBOLS):
        assert not set(decl) & set(other)
    # the mirrors have the sizes the header states
    text = open(REVE_HEADER).read()
    assert "} icp4r_reve_params; /* 272 bytes */" in text and "} icp4r_reve_result; /* 88 bytes */" in text
    import ctypes as C

    assert C.sizeof(reve.ReveParams) == 272 and C.sizeof(reve.ReveResult) == reve.REVE_RESULT_DTYPE.itemsize == 88
    # one field per setting, same names, in the header and in the facade
    facade = open(os.path.join(ROOT, "include", "icp4r", "reve_compat.hpp")).read()
    for k in reve_twin.DEFAULTS:
        assert re.search(rf"\b{k}\b", text), k
        if k not in ("seed", "use_z_filter"):
            assert re.search(rf"\b{k}\b", facade), k


def test_params_default_are_the_nodes():
    """config_init, src/radar_odometry.cpp:576-610 of the reference."""
    from icp4r import reve

    want = dict(min_dist=0.25, max_dist=100, min_db=0, elevation_thresh_deg=60, azimuth_thresh_deg=60, filter_min_z=-3,
                filter_max_z=3, doppler_velocity_correction_factor=1.0, thresh_zero_velocity=0.05,
                allowed_outlier_percentage=0.25, sigma_zero_velocity_x=0.025, sigma_zero_velocity_y=0.025,
                sigma_zero_velocity_z=0.025, sigma_offset_radar_x=0.05, sigma_offset_radar_y=0.025,
                sigma_offset_radar_z=0.05, max_sigma_x=0.2, max_sigma_y=0.2, max_sigma_z=0.2, max_r_cond=1000,
                use_cholesky_instead_of_bdcsvd=1, use_ransac=1, outlier_prob=0.4, success_prob=0.9999, N_ransac_points=3,
                inlier_thresh=0.15, use_odr=1, sigma_v_d=0.125, min_speed_odr=4.0, model_noise_offset_deg=2.0,
                model_noise_scale_deg=10.0)
    got = reve.default_params().as_dict()
    assert len(want) == 31
    for k, v in want.items():
        assert got[k] == v, k
    assert got["use_z_filter"] == 0
    assert set(got) == set(want) | {"seed", "use_z_filter"}
    assert got == reve_twin.params()  # the twin's defaults are the library's, seed included
    p = reve.default_params()
    assert bytes(p)[-28:] == bytes(28)  # reserved words are zero


def test_ransac_iterations():
    from icp4r import reve

    assert reve.ransac_iterations() == 37 == reve_twin.ransac_iterations(reve_twin.params())
    for sp, op in ((0.99, 0.5), (0.999, 0.2)):
        want = int(math.log(1 - sp) / math.log(1 - (1 - op) ** 3))
        assert reve.ransac_iterations(reve.default_params(success_prob=sp, outlier_prob=op)) == want
        assert reve_twin.ransac_iterations(reve_twin.params(success_prob=sp, outlier_prob=op)) == want
    assert (int(math.log(0.01) / math.log(0.875)), int(math.log(0.001) / math.log(1 - 0.512))) == (34, 9)
    assert reve.ransac_iterations(reve.default_params(success_prob=1.0)) == -1
    assert reve.ransac_iterations(reve.default_params(success_prob=0.0)) == 0


@pytest.mark.parametrize("n_valid", [3, 4, 8192])
def test_draw_is_the_twins_and_distinct(n_valid):
    import icp4r
    from icp4r import reve

    seen = set()
    for seed in (0, 0x4E7E5EED, 0x4E7E5EED + (5 << 32), 2 ** 64 - 3):
        for k in range(128):
            d = reve.draw(seed, k, n_valid)
            assert d == reve_twin.draw(seed, k, n_valid), (seed, k)
            assert len(set(d)) == 3 and all(0 <= i < n_valid for i in d)
            seen.add(d)
    assert len(seen) == 6 if n_valid == 3 else len(seen) > 20  # every order of 3 occurs; no stuck stream
    with pytest.raises(icp4r.ICP4RError) as e:
        reve.draw(0, 0, 2)
    assert e.value.code == E_INVALID


def test_device_entries_refuse_what_is_not_built():
    """Settings are validated before any device call: a context without a device is enough."""
    import icp4r
    from icp4r import reve

    ctx = icp4r.Context(icp4r.NO_DEVICE)
    try:
        for kw, code in ((dict(N_ransac_points=4), E_INVALID), (dict(use_ransac=0), E_INVALID),
                         (dict(allowed_outlier_percentage=1.5), E_INVALID), (dict(inlier_thresh=float("nan")), E_INVALID),
                         (dict(success_prob=1.0), E_INVALID), (dict(success_prob=1 - 1e-15, outlier_prob=0.9), E_TOO_LARGE)):
            with pytest.raises(icp4r.ICP4RError) as e:
                reve.estimate_batch_device(8, 8, 8, 1, 16, 8, params=reve.default_params(**kw), ctx=ctx)
            assert e.value.code == code, kw
            with pytest.raises(icp4r.ICP4RError) as e:
                reve.inlier_clouds_batch_device(8, 8, 8, 1, 16, 8, 16, 8, 8, params=reve.default_params(**kw), ctx=ctx)
            assert e.value.code == code, kw
        with pytest.raises(icp4r.ICP4RError) as e:
            reve.estimate_batch_device(8, 8, 8, 1, reve.MAX_POINTS + 1, 8, ctx=ctx)
        assert e.value.code == E_TOO_LARGE
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- the twin itself
def test_twin_cond_and_solve_against_numpy():
    """The fixed-sweep Jacobi cond and the cofactor solve against numpy's eigvalsh / solve on HtH of random
    direction triples and of whole scans: 8 sweeps converge (relative 1e-12 at cond <= 1e6)."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for trial in range(300):
        rows = 3 if trial < 200 else 50
        h = rng.normal(size=(rows, 3)) * [1.0, 1.0, 10.0 ** -rng.uniform(0, 2)]
        h /= np.linalg.norm(h, axis=1, keepdims=True)
        M = h.T @ h
        m6 = [M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]]
        w = np.linalg.eigvalsh(M)
        ref = w[-1] / w[0]
        if not ref < 1e6:
            continue
        with np.errstate(all="ignore"):
            c = reve_twin.jacobi_cond(m6)
        worst = max(worst, abs(c - ref) / ref * min(1.0, 1e3 / ref))
        g = rng.normal(size=3)
        with np.errstate(all="ignore"):
            _, v = reve_twin.solve3(m6, g)
        assert np.allclose(np.array(v, float), np.linalg.solve(M, g), rtol=1e-9 * ref, atol=0)
    assert worst < 1e-12, worst
    with np.errstate(all="ignore"):
        assert not abs(reve_twin.jacobi_cond([2.0, 0.0, 0.0, 1.0, 0.0, 0.0])) < 1000  # planar: inf


def _scan(kind):
    if kind == "seq0":
        return synth.make_sequence(0, n=2048, el_deg=30.0)[0][0]
    if kind == "movers1":
        return synth.make_sequence_movers(1, n=2048, el_deg=30.0)[0][0]
    if kind == "still":
        return synth.make_sequence(0, n=2048, el_deg=30.0, speed=0.0)[0][0]
    if kind == "el3":
        return synth.make_sequence(0, n=2048)[0][0]
    if kind == "planar":
        rec = synth.make_sequence(0, n=2048, el_deg=30.0)[0][0].copy()
        rec[:, 2] = 0.0
        return rec
    raise KeyError(kind)


# the twin's answers at the default seed, recorded: (n_valid, n_inliers, accepted, best, zero_velocity, success)
KNOWN = {
    "seq0": (2048, 1825, 32, 2, 0, 1),
    "movers1": (2047, 1535, 33, 1, 0, 1),
    "still": (2048, 1792, 0, -1, 1, 1),
    "el3": (2048, 1825, 1, 20, 0, 1),
    "planar": (2048, 0, 0, -1, 0, 0),
}


@pytest.mark.parametrize("kind", sorted(KNOWN))
def test_twin_known_answers(kind):
    rec = _scan(kind)
    r = reve_twin.estimate(rec)
    got = (r["n_valid"], r["n_inliers"], r["accepted"], r["best"], r["zero_velocity"], r["success"])
    assert got == KNOWN[kind]
    assert int(r["mask"].sum()) == r["n_inliers"] and r["n"] == 2048
    if kind == "seq0":
        # 10 % dynamic points: 1825 of 2048 stay; +v_sensor because y = -doppler
        assert np.abs(r["v"] - [5.0, 0.0, 0.0]).max() < 1e-3
        assert r["iterations"] == 37 and len(r["conds"]) == 37
        assert (r["sigma"] < 0.2).all() and (r["sigma"] > [0.05, 0.025, 0.05]).all()
    if kind == "movers1":
        # the mover's quarter (512 points) is gone
        assert 1450 <= r["n_inliers"] <= 1560 and np.abs(r["v"] - [5.0, 0.0, 0.0]).max() < 2e-3
    if kind == "still":
        assert (r["v"] == 0).all() and (r["sigma"] == 0.025).all() and r["iterations"] == 0
        d = np.abs(rec[:, 4].astype(np.float64))
        assert r["n_inliers"] == int((d < 0.05).sum())
    if kind == "el3":
        # elevations within +-3 degrees: v is still recovered, but few triples are well conditioned
        assert 1 <= r["accepted"] <= 8 and np.abs(r["v"] - [5.0, 0.0, 0.0]).max() < 5e-3
        assert sum(c < 1000 for c in r["conds"]) == r["accepted"]
    if kind == "planar":
        assert r["iterations"] == 37 and not r["mask"].any() and (r["v"] == 0).all()


def test_twin_filters_and_small_scans():
    """Each filter alone, the 2 / 3 valid-target edge, and the two sum orders of the refit."""
    good = np.array([[10, 1, 1, 5, -3.0], [12, -2, 0.5, 5, -3.1], [9, 3, -1, 5, -2.9], [15, 0, 2, 5, -3.0]], np.float32)
    bad = np.array([[0.25, 0, 0, 5, 1], [0.1, 0, 0, 5, 1], [100, 0, 0, 5, 1], [150, 0, 0, 5, 1], [10, 1, 1, 0, 1],
                    [5, 10, 0, 5, 1], [-5, 1, 0, 5, 1], [5, 0, 10, 5, 1], [5, 0, -10, 5, 1], [np.nan, 1, 1, 5, 1],
                    [10, np.inf, 1, 5, 1], [10, 1, 1, 5, np.nan], [10, 1, 1, 5, np.inf], [10, 1, 1, np.nan, 1]], np.float32)
    p = reve_twin.params()
    assert reve_twin.valid_mask(good, p).all() and not reve_twin.valid_mask(bad, p).any()
    assert reve_twin.valid_mask([[5, 0, 2.9, 5, 1]], reve_twin.params(use_z_filter=1)).all()
    assert not reve_twin.valid_mask([[5, 0, 3.0, 5, 1]], reve_twin.params(use_z_filter=1)).any()
    assert reve_twin.valid_mask([[5, 0, 3.0, 5, 1]], p).all()
    r = reve_twin.estimate(np.concatenate([good[:2], bad]))
    assert (r["n_valid"], r["n_inliers"], r["iterations"], r["best"], r["success"]) == (2, 0, 0, -1, 0)
    r = reve_twin.estimate(np.concatenate([bad[:5], good[:3], bad[5:]]))
    assert (r["n_valid"], r["iterations"]) == (3, 37)
    a = reve_twin.estimate(_scan("seq0"))
    b = reve_twin.estimate(_scan("seq0"), reverse=True)
    assert (a["mask"] == b["mask"]).all() and a["best"] == b["best"]
    assert 0 < np.abs(a["v"] - b["v"]).max() < 1e-12 and np.abs(a["sigma"] - b["sigma"]).max() < 1e-12


def test_twin_batch_seeds_and_refusal():
    rec = np.concatenate([_scan("seq0")[:300], _scan("seq0")[:300]])
    res = reve_twin.estimate_batch(rec, [0, 300, 0], [300, 300, 301], 300)
    assert res[2] is None
    assert res[0]["best"] != res[1]["best"] or res[0]["accepted"] != res[1]["accepted"]  # scan s draws with seed + (s << 32)
    one = reve_twin.estimate(rec[:300], seed=reve_twin.DEFAULTS["seed"] + (1 << 32))
    assert (one["mask"] == res[1]["mask"]).all() and one["best"] == res[1]["best"]


# ------------------------------------------------------------------------------------- programs
def test_reve_callsite_compiles_against_the_facade():
    """tests/cpp/reve_callsite.cpp sets every setting by name and calls estimate() through reve_compat.hpp."""
    text = open(os.path.join(ROOT, "tests", "cpp", "reve_callsite.cpp")).read()
    for k in reve_twin.DEFAULTS:
        if k not in ("seed", "use_z_filter"):
            assert re.search(rf"\bc\.{k} =", text), k
    assert "radar_ego_velocity.estimate(radar_scan, v_r, sigma_v_r," in text
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "reve_callsite")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "reve_callsite.mk"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(exe)


def test_reve_host_check_under_sanitizers():
    """tests/cpp/reve_host_check: the draw, the hypothesis count, the Jacobi cond and the solve, built with
    -fsanitize=address,undefined and run as a program."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "reve_host_check.mk"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "_build", "reve_host_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "12220 draws, 0 mismatches" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
