"""Voxelized GICP on the device (include/icp4r/icp4r_vgicp.h) against the numpy twin tests/vgicp_twin.py.

Bars, those of tests/test_gicp.py: poses within 1e-5 (rad / m), iterations, converged and n_correspondences
identical, the fitness within 1e-6 relative.  The twin is fed the device's own covariances
(icp4r_gicp_covariances: the same kernels as inside align, bit-identical neighbour sets), so only the order
of the Gauss-Newton sums differs.  The voxel map sums sequentially in ascending point index on both sides:
coordinates, order and num_points are equal and mean and cov are bit-equal.
"""
import ctypes as C

import numpy as np
import pytest

import vgicp_twin as tw
from helpers import pose_err
from test_gicp import _scene
from test_gicp_paths import _far_guess
from test_vgicp import crafted_clouds, random_spd


def _vgicp():
    from icp4r import vgicp

    return vgicp


def _assert_map_equal(got, vm):
    coords, num, mean, cov = got
    np.testing.assert_array_equal(coords, vm.coords)
    np.testing.assert_array_equal(num, vm.num)
    np.testing.assert_array_equal(mean, vm.mean)
    np.testing.assert_array_equal(cov, vm.cov)


# ------------------------------------------------------------------------------- the voxel map
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(crafted_clouds()))
def test_gpu_voxel_map_crafted(gpu_ctx, name):
    vgicp = _vgicp()
    pts, res = crafted_clouds()[name]
    Cv = random_spd(np.random.default_rng(5), len(pts))
    _assert_map_equal(vgicp.voxel_map(pts, res, cov=Cv, ctx=gpu_ctx), tw.voxel_map(pts, Cv, res))


@pytest.mark.gpu
@pytest.mark.parametrize("n,res", [(2049, 1.0), (20011, 0.3)])
def test_gpu_voxel_map_sizes(gpu_ctx, n, res):
    """More than one sort block and compaction block; at 20011 points many voxels of one point and some of
    dozens (a dense core inside a sparse box)."""
    vgicp = _vgicp()
    rng = np.random.default_rng(n)
    pts = np.concatenate([rng.uniform(-12, 12, (n - n // 4, 3)), rng.normal(0, 0.4, (n // 4, 3))]).astype(np.float32)
    pts = pts[rng.permutation(n)]
    Cv = random_spd(rng, n)
    vm = tw.voxel_map(pts, Cv, res)
    assert vm.num.max() > 8 and (vm.num == 1).any()
    _assert_map_equal(vgicp.voxel_map(pts, res, cov=Cv, ctx=gpu_ctx), vm)


@pytest.mark.gpu
def test_gpu_voxel_map_knn_covariances_cap_and_range(gpu_ctx):
    import icp4r
    from icp4r import gicp

    vgicp = _vgicp()
    src, _, _ = _scene(3, 700)
    # cov_in = NULL: the k-NN covariances with k and the regularisation
    for k, reg in ((5, gicp.REG_PLANE), (20, gicp.REG_MIN_EIG)):
        Cv = gicp.covariances(src, k, reg, ctx=gpu_ctx)
        _assert_map_equal(vgicp.voxel_map(src, 1.0, k=k, regularization=reg, ctx=gpu_ctx), tw.voxel_map(src, Cv, 1.0))
    # the cap: one voxel short is ICP4R_E_INVALID with n_voxels set and nothing written; exact room is fine
    Cv = gicp.covariances(src, 5, gicp.REG_PLANE, ctx=gpu_ctx)
    vm = tw.voxel_map(src, Cv, 1.0)
    V = len(vm.coords)
    c, n, cs = icp4r._cloud(src)
    c9 = np.ascontiguousarray(Cv.reshape(n, 9))
    coords = np.full((V, 3), 777, np.int32)
    nv = C.c_int32(-1)
    rc = vgicp._lib().icp4r_vgicp_voxel_map(gpu_ctx.handle, icp4r._ptr(c), n, cs, icp4r._ptr(c9), 5, 3, 1.0, V - 1,
                                            icp4r._ptr(coords), None, None, None, C.byref(nv))
    assert rc == icp4r.E_INVALID and nv.value == V and (coords == 777).all()
    _assert_map_equal(vgicp.voxel_map(src, 1.0, cov=Cv, cap=V, ctx=gpu_ctx), vm)
    # a coordinate past +-2^20 cells: refused; the last cell inside is kept
    far = src.copy()
    far[5, 1] = np.float32(2.0 ** 20)
    with pytest.raises(icp4r.ICP4RError) as ei:
        vgicp.voxel_map(far, 1.0, cov=Cv, ctx=gpu_ctx)
    assert ei.value.code == icp4r.E_INVALID
    far[5, 1] = np.float32(-(2.0 ** 20))
    _assert_map_equal(vgicp.voxel_map(far, 1.0, cov=Cv, ctx=gpu_ctx), tw.voxel_map(far, Cv, 1.0))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(icp4r.ICP4RError):
            vgicp.voxel_map(src, bad, cov=Cv, ctx=gpu_ctx)


# ------------------------------------------------------------------------------- align vs the twin
def _centred(src, tgt):
    c = tgt.mean(0).astype(np.float32)
    return np.ascontiguousarray(src - c), np.ascontiguousarray(tgt - c)


# name -> (seed, source points, target points, VgicpParams fields, guess, centred)
ALIGN_CASES = {
    "n1_m512_direct1": (0, 1, 512, dict(k_correspondences=5), None, False),
    "n255_m512_direct7_reg_none": (1, 255, 512, dict(k_correspondences=20, neighbor_search=1, regularization=0), None, False),
    "n256_m2048_res0p3_direct27_reg_min_eig": (2, 256, 2048, dict(k_correspondences=5, voxel_resolution=0.3,
                                                                 neighbor_search=2, regularization=1), None, False),
    "n257_m2048_direct27_reg_norm_min_eig": (3, 257, 2048, dict(k_correspondences=5, neighbor_search=2,
                                                               regularization=2), None, False),
    "n1500_m2048_res0p3_reg_frobenius": (4, 1500, 2048, dict(k_correspondences=5, voxel_resolution=0.3,
                                                            regularization=4), None, False),
    "n1500_m512_direct7_guess": (5, 1500, 512, dict(k_correspondences=5, neighbor_search=1), "near", False),
    "far_guess_direct7": (0, 1500, 2048, dict(k_correspondences=5, neighbor_search=1), "far", False),
    "max_iterations_0": (0, 1500, 2048, dict(k_correspondences=5, max_iterations=0), "far", False),
    "max_iterations_1": (0, 1500, 2048, dict(k_correspondences=5, max_iterations=1), "far", False),
    "lm_failure": (0, 1500, 2048, dict(k_correspondences=5, lm_max_iterations=0), "far", False),
    "straddles_origin_res0p3_direct7": (6, 1500, 2048, dict(k_correspondences=5, voxel_resolution=0.3,
                                                           neighbor_search=1), None, True),
    "no_fitness": (7, 1500, 2048, dict(k_correspondences=5, compute_fitness=0), None, False),
}


def _near_guess():
    g = np.eye(4, dtype=np.float32)
    c, s = np.cos(0.05), np.sin(0.05)
    g[:2, :2] = [[c, -s], [s, c]]
    g[:3, 3] = [0.1, -0.05, 0.02]
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ALIGN_CASES))
def test_gpu_align_matches_twin(gpu_ctx, name):
    from icp4r import gicp

    vgicp = _vgicp()
    seed, n, m, fields, guess, centred = ALIGN_CASES[name]
    src, tgt, _ = _scene(seed, max(n, m))
    src, tgt = np.ascontiguousarray(src[:n]), np.ascontiguousarray(tgt[:m])
    if centred:
        src, tgt = _centred(src, tgt)
        assert tgt.min() < -1 and tgt.max() > 1
    G = {"near": _near_guess(), "far": _far_guess(), None: None}[guess]
    p = vgicp.default_params(**fields)
    r, aligned = vgicp.align(src, tgt, p, guess=G, want_aligned=True, ctx=gpu_ctx)
    assert r.status == 0
    CA = gicp.covariances(src, p.gicp.k_correspondences, p.gicp.regularization, ctx=gpu_ctx)
    CB = gicp.covariances(tgt, p.gicp.k_correspondences, p.gicp.regularization, ctx=gpu_ctx)
    o = tw.align(src, tgt, CA, CB, resolution=p.voxel_resolution, mode=p.neighbor_search, guess=G,
                 max_iterations=p.gicp.max_iterations, lm_max_iterations=p.gicp.lm_max_iterations)
    dt, dr = pose_err(r.matrix(), o["T"])
    print(f"{name}: dt {dt:.3e} dr {dr:.3e} iterations {r.iterations}/{o['iterations']} converged "
          f"{r.converged}/{o['converged']} correspondences {r.n_correspondences}/{o['n_valid']} fitness {r.fitness:.6e}")
    assert dt < 1e-5 and dr < 1e-5, (dt, dr)
    assert r.iterations == o["iterations"] and bool(r.converged) == o["converged"]
    assert r.n_correspondences == o["n_valid"]
    if name == "lm_failure":
        assert o["lm_failed"] and not r.converged
        np.testing.assert_array_equal(r.matrix(), G)
    if name == "max_iterations_0":
        assert r.n_correspondences == 0 and not r.converged
        np.testing.assert_array_equal(r.matrix(), G)
    # align's output = transformPointCloud(input, final): float, Eigen's order
    Tg = r.matrix()
    want = np.empty_like(src)
    for rr in range(3):
        v = Tg[rr, 0] * src[:, 0]
        v = v + Tg[rr, 1] * src[:, 1]
        v = v + Tg[rr, 2] * src[:, 2]
        want[:, rr] = v + Tg[rr, 3]
    np.testing.assert_array_equal(aligned[:, :3], want)
    if p.gicp.compute_fitness:
        fit = tw.fitness(src, tgt, Tg)
        assert abs(r.fitness - fit) <= 1e-6 * max(fit, 1e-12), (r.fitness, fit)
    else:
        assert r.fitness == np.finfo(np.float64).max


@pytest.mark.gpu
def test_gpu_identity_and_out_of_reach(gpu_ctx):
    vgicp = _vgicp()
    src, _, _ = _scene(1, 800)
    p = vgicp.default_params(k_correspondences=5)
    r, _ = vgicp.align(src, src, p, ctx=gpu_ctx)
    assert r.converged and r.iterations == 0 and r.n_correspondences == len(src)
    G = np.eye(4, dtype=np.float32)
    G[:3, 3] = [0.25, -0.5, 0.125]
    for mode in (vgicp.DIRECT1, vgicp.DIRECT27):
        p = vgicp.default_params(k_correspondences=5, neighbor_search=mode)
        r, _ = vgicp.align(src, src + np.float32(100.0), p, guess=G, ctx=gpu_ctx)
        assert r.status == 0 and r.converged and r.iterations == 0 and r.n_correspondences == 0
        np.testing.assert_array_equal(r.matrix(), G)


@pytest.mark.gpu
def test_gpu_lm_trials_and_grid_do_not_change_results(gpu_ctx, plan):
    """Speculative trials or one by one (gicp_spec), any spread of the slices over workgroups (gicp_grid),
    a 17k-point source (512-point slices): bit-identical."""
    vgicp = _vgicp()
    cases = []
    src, tgt, _ = _scene(3, 2000)
    cases.append((src, tgt, _far_guess(), vgicp.default_params(k_correspondences=5, neighbor_search=1)))
    cases.append((src, tgt, _far_guess(), vgicp.default_params(k_correspondences=5, lm_init_lambda_factor=1e-2)))
    src, tgt, _ = _scene(9, 17000)
    cases.append((src, tgt, None, vgicp.default_params(k_correspondences=5)))
    for src, tgt, guess, p in cases:
        runs = []
        for spec, grid in ((0, 2048), (1, 3), (2, 1), (2, 2048)):
            plan(gicp_spec=spec, gicp_grid=grid)
            r, aligned = vgicp.align(src, tgt, p, guess=guess, want_aligned=True, ctx=gpu_ctx)
            runs.append((r.matrix(), r.iterations, r.converged, r.fitness, r.status, r.n_correspondences, aligned))
        for other in runs[:3]:
            np.testing.assert_array_equal(other[0], runs[3][0])
            assert other[1:6] == runs[3][1:6]
            np.testing.assert_array_equal(other[6], runs[3][6])


# ------------------------------------------------------------------------------- the batch
GUARD = 64  # guard floats on each side


def _guarded_batch(pairs, guesses):
    """The icp4r_batch of the pairs with guard floats around the results and the aligned clouds."""
    import torch

    import icp4r

    src = np.concatenate([np.pad(p[0], ((0, 0), (0, 1))) for p in pairs]).astype(np.float32)
    tgt = np.concatenate([np.pad(p[1], ((0, 0), (0, 1))) for p in pairs]).astype(np.float32)
    sn = np.array([len(p[0]) for p in pairs], np.int32)
    tn = np.array([len(p[1]) for p in pairs], np.int32)
    so = np.concatenate([[0], np.cumsum(sn)[:-1]]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tn)[:-1]]).astype(np.int64)
    arrays = dict(src=src, tgt=tgt, sn=sn, tn=tn, so=so, to=to,
                  guess=np.stack([np.asarray(g, np.float32).T.reshape(16) for g in guesses]))
    dev = torch.device("cuda:0")
    ts = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    rfloats = len(pairs) * icp4r.RESULT_DTYPE.itemsize // 4
    ts["res"] = torch.full((GUARD + rfloats + GUARD,), -7.5, dtype=torch.float32, device=dev)
    ts["aligned"] = torch.full((GUARD + 4 * len(src) + GUARD,), -7.5, dtype=torch.float32, device=dev)
    b = icp4r.Batch()
    b.src, b.tgt = ts["src"].data_ptr(), ts["tgt"].data_ptr()
    b.src_off, b.src_n, b.tgt_off, b.tgt_n = ts["so"].data_ptr(), ts["sn"].data_ptr(), ts["to"].data_ptr(), ts["tn"].data_ptr()
    b.guess = ts["guess"].data_ptr()
    b.aligned = ts["aligned"].data_ptr() + 4 * GUARD
    b.npairs, b.max_src_n, b.max_tgt_n = len(pairs), int(sn.max()), int(tn.max())
    return b, ts, ts["res"].data_ptr() + 4 * GUARD, so, sn


def _run_batch(gpu_ctx, vgicp, pairs, guesses, p):
    import torch

    import icp4r

    b, ts, res_ptr, so, sn = _guarded_batch(pairs, guesses)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    vgicp.align_batch_device(b, p, res_ptr, stream=stream.cuda_stream, ctx=gpu_ctx)
    stream.synchronize()
    res, al = ts["res"].cpu().numpy(), ts["aligned"].cpu().numpy()
    for buf in (res, al):
        assert (buf[:GUARD] == -7.5).all() and (buf[-GUARD:] == -7.5).all()
    rows = np.frombuffer(res[GUARD:-GUARD].tobytes(), icp4r.RESULT_DTYPE)
    body = al[GUARD:-GUARD].reshape(-1, 4)
    return rows, [body[so[i]:so[i] + sn[i]] for i in range(len(pairs))]


@pytest.mark.gpu
def test_gpu_batch_of_19_ragged_pairs(gpu_ctx, plan):
    """19 ragged pairs, among them an empty source, an empty target, a non-finite coordinate, a target
    coordinate outside the key range and a pair with no overlap: each healthy pair's row and aligned cloud
    are bit-identical to its single call and to the batch without the bad pairs, for gicp_grid 1, 2 and the
    default, on a caller's stream, with guard floats around results and aligned."""
    import icp4r

    vgicp = _vgicp()
    pairs, guesses, kind = [], [], []
    for s in range(19):
        src, tgt, T = _scene(s, 300 + 50 * s)
        g, what = np.eye(4, dtype=np.float32), "ok"
        if s == 2:
            src, what = src[:0].copy(), "empty_source"
        elif s == 4:
            tgt, what = tgt[:0].copy(), "empty_target"
        elif s == 6:
            src = src.copy()
            src[17, 2] = np.nan
            what = "nonfinite"
        elif s == 9:
            src, what = src + np.float32(100.0), "no_overlap"
        elif s == 12:
            tgt = tgt.copy()
            tgt[3, 0] = np.float32(2.0 ** 21)
            what = "out_of_range"
        elif s == 8:
            g = _far_guess()
        elif s == 14:
            g = T.astype(np.float32)
        pairs.append((src, tgt))
        guesses.append(g)
        kind.append(what)
    p = vgicp.default_params(k_correspondences=5, neighbor_search=vgicp.DIRECT7)
    fields = ("T", "iterations", "converged", "fitness", "n_correspondences", "status")
    runs = []
    for grid in (1, 2, None):
        if grid is not None:
            plan(gicp_grid=grid)
        else:
            gpu_ctx.reset_plan_options()
        runs.append(_run_batch(gpu_ctx, vgicp, pairs, guesses, p))
    for rows, al in runs[:2]:
        for f in fields:
            np.testing.assert_array_equal(rows[f], runs[2][0][f], err_msg=f)
        for i in range(19):
            np.testing.assert_array_equal(al[i], runs[2][1][i])
    rows, al = runs[2]
    status = {"ok": 0, "empty_source": 0, "no_overlap": 0, "empty_target": icp4r.E_EMPTY,
              "nonfinite": icp4r.E_NONFINITE, "out_of_range": icp4r.E_INVALID}
    for i in range(19):
        assert rows[i]["status"] == status[kind[i]], (i, kind[i])
        if status[kind[i]] != 0:  # nothing computed, nothing written
            assert not rows[i]["converged"] and (al[i] == -7.5).all(), (i, kind[i])
    assert rows[2]["converged"] and rows[2]["iterations"] == 0 and rows[2]["n_correspondences"] == 0
    assert rows[9]["converged"] and rows[9]["iterations"] == 0 and rows[9]["n_correspondences"] == 0
    healthy = [i for i in range(19) if kind[i] in ("ok", "no_overlap")]
    for i in healthy:
        r, a1 = vgicp.align(pairs[i][0], pairs[i][1], p, guess=guesses[i], want_aligned=True, ctx=gpu_ctx)
        np.testing.assert_array_equal(rows[i]["T"], np.array(r.T, np.float32), err_msg=f"pair {i}")
        assert rows[i]["iterations"] == r.iterations and rows[i]["converged"] == r.converged, i
        assert rows[i]["fitness"] == r.fitness and rows[i]["n_correspondences"] == r.n_correspondences, i
        np.testing.assert_array_equal(al[i][:, :3], a1[:, :3], err_msg=f"pair {i}")
    assert len(set(rows["iterations"][healthy].tolist())) >= 2
    rows2, al2 = _run_batch(gpu_ctx, vgicp, [pairs[i] for i in healthy], [guesses[i] for i in healthy], p)
    for j, i in enumerate(healthy):
        for f in fields:
            np.testing.assert_array_equal(rows2[j][f], rows[i][f], err_msg=f"{f} pair {i}")
        np.testing.assert_array_equal(al2[j], al[i])


# ------------------------------------------------------------------------------- the C++ facade
@pytest.mark.gpu
def test_gpu_fast_vgicp_cpp_callsite(gpu_ctx, tmp_path):
    """tests/cpp/vgicp_callsite.cpp: a FastVGICP block through include/icp4r/fast_gicp_compat.hpp — the same
    bits as the Python entry on the same inputs; a refused mode reports no convergence and does not throw."""
    import os
    import subprocess

    from icp4r import synth

    vgicp = _vgicp()
    src, tgt, _ = _scene(4, 1500)
    rec = lambda xyz: np.concatenate([xyz, np.ones((len(xyz), 1), np.float32), np.zeros((len(xyz), 1), np.float32)], 1)
    a, b = tmp_path / "scan_map.bin", tmp_path / "submap.bin"
    synth.write_bin(a, rec(src))
    synth.write_bin(b, rec(tgt))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "_build", "vgicp_callsite")
    r = subprocess.run([exe, str(a), str(b), "7", "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    head, tl = r.stdout.strip().split("\n")[:2]
    conv, score, iters, nout = head.split()
    Tc = np.array([float(v) for v in tl.split()], np.float32).reshape(4, 4).T  # column-major
    p = vgicp.default_params(k_correspondences=5, neighbor_search=vgicp.DIRECT7, voxel_resolution=0.5)
    res, _ = vgicp.align(src, tgt, p, ctx=gpu_ctx)
    assert (Tc == res.matrix()).all()
    assert int(conv) == int(res.converged) == 1 and int(iters) == res.iterations and int(nout) == len(src)
    assert float(score) == res.fitness
    r = subprocess.run([exe, str(a), str(b), "radius"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[0] == "0" and "DIRECT" in r.stderr


# ------------------------------------------------------------------------------- parameters
@pytest.mark.gpu
def test_gpu_invalid_parameters_and_refused_modes(gpu_ctx):
    import icp4r

    vgicp = _vgicp()
    src, tgt, _ = _scene(0, 300)
    bad = [dict(voxel_resolution=0.0), dict(voxel_resolution=-1.0), dict(voxel_resolution=float("nan")),
           dict(voxel_resolution=float("inf")), dict(neighbor_search=vgicp.DIRECT_RADIUS), dict(neighbor_search=-1),
           dict(voxel_accumulation=vgicp.ADDITIVE_WEIGHTED), dict(voxel_accumulation=vgicp.MULTIPLICATIVE),
           dict(k_correspondences=0), dict(k_correspondences=33), dict(max_iterations=-1), dict(regularization=5)]
    for kw in bad:
        with pytest.raises(icp4r.ICP4RError) as ei:
            vgicp.align(src, tgt, vgicp.default_params(**kw), ctx=gpu_ctx)
        assert ei.value.code == icp4r.E_INVALID, kw
    # max_correspondence_distance is accepted and changes nothing: VGICP has no distance gate
    a, _ = vgicp.align(src, tgt, vgicp.default_params(k_correspondences=5), ctx=gpu_ctx)
    b, _ = vgicp.align(src, tgt, vgicp.default_params(k_correspondences=5, max_correspondence_distance=1e-3), ctx=gpu_ctx)
    np.testing.assert_array_equal(a.matrix(), b.matrix())
    assert (a.iterations, a.n_correspondences, a.fitness) == (b.iterations, b.n_correspondences, b.fitness)
    r, _ = vgicp.align(src, tgt[:0], ctx=gpu_ctx)
    assert r.status == icp4r.E_EMPTY and not r.converged
    f = vgicp.FastVGICP(gpu_ctx)
    f.setResolution(0.5)
    f.setNeighborSearchMethod(vgicp.DIRECT7)
    f.setCorrespondenceRandomness(5)
    f.setInputTarget(tgt)
    f.setInputSource(src)
    out = f.align()
    assert f.hasConverged() and out.shape == src.shape and f.getFitnessScore() < 1.0
