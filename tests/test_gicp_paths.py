"""Generalized ICP, the branches tests/test_gicp.py does not reach (bars: that file's header).

  A  the k-NN walk of clouds with more than 64 superblocks (n > 8192; the scan-to-map submap's case)
  B  every instantiated list length (K = 5, 8, 16, 20, 32) in both covariance kernels
  D  degenerate clouds (identical points, collinear, an exact lattice, duplicated clusters)
  E  the covariances a registration computed itself (source: its own index on the aux stream;
     target: the plan's index, the multi-workgroup Morton sort past 8192 points), read back
  F  batches of more than 8 pairs, workgroups sharing a pair's slices, pairs stopping apart
  G  a distance gate that rejects some correspondences and keeps the others
  H  a failed Levenberg-Marquardt step and max_iterations = 0 against the oracle

(C, clouds of fewer than k points, extends test_gicp.py::test_gpu_small_clouds_fewer_points_than_k.)

Every oracle covariance is computed once per (cloud, k, regularisation) and shared.
"""
import numpy as np
import pytest

from helpers import pose_err
from icp4r import synth

REGS = (0, 1, 2, 3, 4)  # NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS
REG_NONE, REG_PLANE, REG_FROBENIUS = 0, 3, 4


def _gicp():
    from icp4r import gicp

    return gicp


def _scene(seed, n=1500):
    """A pair with a known rigid transform: synth's structured scene, no clutter."""
    p = synth.make_pair(seed, n, clutter=0.0, noise=0.005)
    xyz = lambda rec: np.ascontiguousarray(rec[:, :3], np.float32)
    return xyz(p.src), xyz(p.tgt), p.T_gt


def _far_guess():
    """The far initial pose of test_gicp.py's LM-trials test."""
    c, s = np.cos(0.6), np.sin(0.6)
    g = np.eye(4, dtype=np.float32)
    g[:2, :2] = [[c, -s], [s, c]]
    g[:3, 3] = [0.8, -0.5, 0.3]
    return g


_clouds = {}


def _cloud(name):
    """The named clouds of this module, built once."""
    if name not in _clouds:
        rng = np.random.default_rng(2024)
        if name == "scene8193":  # 65 superblocks of 128 points: the second group of 64 holds one
            c = _scene(10, 8193)[1]
        elif name == "scene20011":  # 157 superblocks: three groups, the last partial
            c = _scene(11, 20011)[1]
        elif name == "src3000":  # the first 3000 source points of scene20011's pair
            c = _scene(11, 20011)[0][:3000].copy()
        elif name == "lattice22":  # 22³ exact lattice: ties at every k-th neighbour
            g = np.stack(np.meshgrid(*[np.arange(22)] * 3, indexing="ij"), -1).reshape(-1, 3)
            c = (g * 0.5).astype(np.float32)[rng.permutation(len(g))]
        elif name == "twice5000":  # every point twice, indices 5000 apart
            c = _scene(12, 5000)[1]
            c = np.concatenate([c, c])
        else:
            raise KeyError(name)
        _clouds[name] = np.ascontiguousarray(c, np.float32)
    return _clouds[name]


_oracle_cov = {}


def _want_cov(oracle_mod, key, cloud, k, reg):
    """oracle.gicp_covariances, once per (key, k, reg); the stored array is read-only."""
    kk = (key, k, reg)
    if kk not in _oracle_cov:
        c = oracle_mod.gicp_covariances(cloud, k, reg)
        c.setflags(write=False)
        _oracle_cov[kk] = c
    return _oracle_cov[kk]


_oracle_align = {}


def _want_align(oracle_mod, key, src, tgt, k):
    """oracle.gicp_align from the identity, once per key."""
    if key not in _oracle_align:
        _oracle_align[key] = oracle_mod.gicp_align(src, tgt, k=k)
    return _oracle_align[key]


def _assert_cov_close(got, want, what):
    """The covariance bar: within 1e-9 of max(1, |C|max)."""
    err = float(np.abs(got - want).max())
    bar = 1e-9 * max(1.0, float(np.abs(want).max()))
    assert err <= bar, (what, err, bar)


def _device_batch(pairs, guesses=None):
    """The icp4r_batch of (src, tgt) pairs in device memory (the layout of
    test_gicp.py::test_gpu_batch_device_equals_single); returns (batch, tensors kept alive)."""
    import torch

    import icp4r

    src = np.concatenate([np.pad(p[0], ((0, 0), (0, 1))) for p in pairs]).astype(np.float32)
    tgt = np.concatenate([np.pad(p[1], ((0, 0), (0, 1))) for p in pairs]).astype(np.float32)
    sn = np.array([len(p[0]) for p in pairs], np.int32)
    tn = np.array([len(p[1]) for p in pairs], np.int32)
    so = np.concatenate([[0], np.cumsum(sn)[:-1]]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tn)[:-1]]).astype(np.int64)
    arrays = dict(src=src, tgt=tgt, sn=sn, tn=tn, so=so, to=to)
    if guesses is not None:  # column-major 4x4 per pair
        arrays["guess"] = np.stack([np.asarray(g, np.float32).T.reshape(16) for g in guesses])
    dev = torch.device("cuda:0")
    ts = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    ts["res"] = torch.zeros(len(pairs) * icp4r.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    b = icp4r.Batch()
    b.src, b.tgt = ts["src"].data_ptr(), ts["tgt"].data_ptr()
    b.src_off, b.src_n, b.tgt_off, b.tgt_n = ts["so"].data_ptr(), ts["sn"].data_ptr(), ts["to"].data_ptr(), ts["tn"].data_ptr()
    if guesses is not None:
        b.guess = ts["guess"].data_ptr()
    b.npairs, b.max_src_n, b.max_tgt_n = len(pairs), int(sn.max()), int(tn.max())
    return b, ts


def _batch_results(ts):
    import icp4r

    return np.frombuffer(ts["res"].cpu().numpy().tobytes(), icp4r.RESULT_DTYPE)


# ------------------------------------------------------------------------------- A: large-cloud walk
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene8193", "scene20011", "lattice22", "twice5000"])
def test_gpu_large_cloud_knn_equals_brute_force(gpu_ctx, plan, name):
    """Clouds of more than 8192 points (more than 64 superblocks) take gicp_knn_cov_kernel's walk over
    groups of 64 superblocks: its neighbour sets are exactly brute force's, covariances bit-identical,
    for every number of lanes per query — with one superblock in the second group, three groups with
    a partial last one, an exact lattice (ties at every k-th neighbour) and a cloud doubled 5000
    indices apart (every distance tie resolved by index across far-apart blocks)."""
    gicp = _gicp()
    cloud = _cloud(name)
    assert len(cloud) > 8192
    for k in (5, 20):
        plan(gicp_cov_brute=1, gicp_knn_lanes=1)
        brute = gicp.covariances(cloud, k, REG_PLANE, ctx=gpu_ctx)
        for lanes in (1, 2, 4, 8):
            plan(gicp_cov_brute=0, gicp_knn_lanes=lanes)
            got = gicp.covariances(cloud, k, REG_PLANE, ctx=gpu_ctx)
            np.testing.assert_array_equal(got, brute, err_msg=f"{name} k={k} L={lanes}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene8193", "scene20011"])
def test_gpu_large_cloud_covariances_match_oracle(gpu_ctx, oracle_mod, name):
    gicp = _gicp()
    cloud = _cloud(name)
    for k in (5, 20):
        for reg in (REG_NONE, REG_PLANE):
            got = gicp.covariances(cloud, k, reg, ctx=gpu_ctx)
            _assert_cov_close(got, _want_cov(oracle_mod, name, cloud, k, reg), (name, k, reg))


# ------------------------------------------------------------------------------- B: list lengths
@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 1003])
def test_gpu_every_list_length_matches_oracle(gpu_ctx, oracle_mod, plan, n):
    """k = 1, 6, 8, 9, 16, 17 reach the lists of 5, 8, 16 and 20 slots at both ends (k = 6..8 and the
    16-slot list are reached by no other test), under every regularisation: 300 points through the
    brute-force kernel (the plan does not prune below 512), 1003 through the pruned one (a partial
    last block), whose sets must also be brute force's."""
    import icp4r

    gicp = _gicp()
    cloud = _scene(13, n)[1]
    assert icp4r.plan(1, n, n, ctx=gpu_ctx)["pruned"] == (n >= 512)
    for k in (1, 6, 8, 9, 16, 17):
        for reg in REGS:
            got = gicp.covariances(cloud, k, reg, ctx=gpu_ctx)
            _assert_cov_close(got, _want_cov(oracle_mod, f"b{n}", cloud, k, reg), (n, k, reg))
        if n >= 512:
            pruned = gicp.covariances(cloud, k, REG_NONE, ctx=gpu_ctx)
            plan(gicp_cov_brute=1, gicp_knn_lanes=1)
            brute = gicp.covariances(cloud, k, REG_NONE, ctx=gpu_ctx)
            plan(gicp_cov_brute=0, gicp_knn_lanes=0)
            np.testing.assert_array_equal(pruned, brute, err_msg=f"k={k}")


# ------------------------------------------------------------------------------- D: degenerate clouds
def _degenerate(shape, n):
    rng = np.random.default_rng(7)
    if shape == "identical":
        c = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (n, 1))
    elif shape == "collinear":  # exact multiples of 0.25 along (1, 1, 0): both neighbours of a point tie
        i = rng.permutation(n).astype(np.float32) * np.float32(0.25)
        c = np.stack([i, i, np.zeros_like(i)], 1)
    elif shape == "flat_lattice":  # an exact 32-wide lattice in z = 0, no jitter
        i = rng.permutation(n)
        c = np.stack([(i % 32) * 0.5, (i // 32) * 0.5, np.zeros(n)], 1)
    elif shape == "dup_clusters":  # 40 tight clusters, each point one of 4 exact positions
        centre = rng.uniform(-20, 20, (40, 3)).astype(np.float32)
        offs = np.array([[0, 0, 0], [0.0078125, 0, 0], [0, 0.0078125, 0], [0, 0, 0.0078125]], np.float32)
        c = centre[rng.integers(0, 40, n)] + offs[rng.integers(0, 4, n)]
    else:
        raise KeyError(shape)
    return np.ascontiguousarray(c, np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["identical", "collinear", "flat_lattice", "dup_clusters"])
def test_gpu_degenerate_clouds_knn(gpu_ctx, oracle_mod, plan, shape):
    """Degenerate clouds through the GICP k-NN (as test_kd_index_degenerate_clouds does for the ICP
    1-NN): the pruned walk, at 1 and 8 lanes per query, returns brute force's bits under every
    regularisation. Against the oracle only NONE and FROBENIUS are compared: the eigenvector-based
    methods are ill-conditioned on the repeated eigenvalues these clouds produce (a rank-0 or rank-1
    scatter matrix), where a last-bit difference may legitimately pick other axes on the two sides."""
    gicp = _gicp()
    for n in (600, 1003):
        cloud = _degenerate(shape, n)
        for k in (5, 20):
            for reg in REGS:
                plan(gicp_cov_brute=1, gicp_knn_lanes=1)
                brute = gicp.covariances(cloud, k, reg, ctx=gpu_ctx)
                for lanes in (1, 8):
                    plan(gicp_cov_brute=0, gicp_knn_lanes=lanes)
                    got = gicp.covariances(cloud, k, reg, ctx=gpu_ctx)
                    np.testing.assert_array_equal(got, brute, err_msg=f"{shape} n={n} k={k} reg={reg} L={lanes}")
                if reg in (REG_NONE, REG_FROBENIUS):
                    _assert_cov_close(brute, oracle_mod.gicp_covariances(cloud, k, reg), (shape, n, k, reg))
            plan(gicp_cov_brute=0, gicp_knn_lanes=0)


@pytest.mark.gpu
def test_gpu_align_identical_points_onto_themselves(gpu_ctx, oracle_mod):
    gicp = _gicp()
    cloud = _degenerate("identical", 600)
    r, _ = gicp.align(cloud, cloud, gicp.default_params(k_correspondences=5), ctx=gpu_ctx)
    o = oracle_mod.gicp_align(cloud, cloud, k=5)
    assert o["converged"] and o["iterations"] == 0 and np.abs(o["T"] - np.eye(4)).max() == 0.0
    assert r.status == 0 and r.iterations == 0 and bool(r.converged)
    np.testing.assert_array_equal(r.matrix(), np.eye(4, dtype=np.float32))


# ------------------------------------------------------------------------------- E: read-back
def _check_pair_covariances(gicp, gpu_ctx, oracle_mod, pairs, names, got, k, reg):
    """got[i] = (source covariances, target covariances) a registration computed for pair i: the bits of
    gicp.covariances of the same cloud (the same neighbour sets summed in key order; only the index
    that found them differs), and the oracle's within the covariance bar."""
    for i, (s, t) in enumerate(pairs):
        for which, (cloud, name) in enumerate(((s, names[i][0]), (t, names[i][1]))):
            np.testing.assert_array_equal(got[i][which], gicp.covariances(cloud, k, reg, ctx=gpu_ctx),
                                          err_msg=f"pair {i} {'source' if which == 0 else 'target'}")
            _assert_cov_close(got[i][which], _want_cov(oracle_mod, name, cloud, k, reg), (i, which))


@pytest.mark.gpu
@pytest.mark.parametrize("mwg", [1, 0])
def test_gpu_align_covariances_read_back_single_pair(gpu_ctx, oracle_mod, plan, mwg):
    """The covariances inside align — the 3000-point source's over its own index on the aux stream, the
    20,011-point target's over the plan's index (morton_mwg = 1: the multi-workgroup Morton sort;
    0: one workgroup) — equal the public covariances call's and the oracle's; the registration equals
    the oracle's."""
    import icp4r

    gicp = _gicp()
    src, tgt = _cloud("src3000"), _cloud("scene20011")
    plan(morton_mwg=mwg)
    pl = icp4r.plan(1, len(src), len(tgt), ctx=gpu_ctx)
    assert pl["pruned"] and not pl["lds"]
    k, reg = 5, REG_PLANE
    r, _ = gicp.align(src, tgt, gicp.default_params(k_correspondences=k), ctx=gpu_ctx)
    got = [(gicp.last_align_covariances(0, 0, len(src), ctx=gpu_ctx),
            gicp.last_align_covariances(0, 1, len(tgt), ctx=gpu_ctx))]
    _check_pair_covariances(gicp, gpu_ctx, oracle_mod, [(src, tgt)], [("src3000", "scene20011")], got, k, reg)
    o = _want_align(oracle_mod, ("src3000", "scene20011", k), src, tgt, k)
    assert r.status == 0 and r.iterations == o["iterations"] and bool(r.converged) == o["converged"]
    assert r.n_correspondences == o["n_valid"]
    dt, dr = pose_err(r.matrix(), o["T"])
    assert dt < 1e-5 and dr < 1e-5, (dt, dr)


@pytest.mark.gpu
@pytest.mark.parametrize("mwg", [1, 0])
def test_gpu_align_covariances_read_back_batch(gpu_ctx, oracle_mod, plan, mwg):
    """The same for a device batch of three pairs with targets of 8193, 20,011 and 600 points on one
    set of strides (the 600-point target indexed and walked on the strides of the 20,011-point one)."""
    import icp4r

    gicp = _gicp()
    s8, t8, _ = _scene(10, 8193)
    s6, t6, _ = _scene(14, 600)
    pairs = [(s8[:3000].copy(), _cloud("scene8193")), (_cloud("src3000"), _cloud("scene20011")), (s6, t6)]
    names = [("src3000_8193", "scene8193"), ("src3000", "scene20011"), ("src600", "tgt600")]
    plan(morton_mwg=mwg)
    pl = icp4r.plan(len(pairs), 3000, 20011, ctx=gpu_ctx)
    assert pl["pruned"] and not pl["lds"]
    k, reg = 5, REG_PLANE
    p = gicp.default_params(k_correspondences=k)
    b, ts = _device_batch(pairs)
    gicp.align_batch_device(b, p, ts["res"].data_ptr(), ctx=gpu_ctx)
    got = [(gicp.last_align_covariances(i, 0, len(s), ctx=gpu_ctx), gicp.last_align_covariances(i, 1, len(t), ctx=gpu_ctx))
           for i, (s, t) in enumerate(pairs)]
    out = _batch_results(ts)
    _check_pair_covariances(gicp, gpu_ctx, oracle_mod, pairs, names, got, k, reg)
    for i, (s, t) in enumerate(pairs):
        o = _want_align(oracle_mod, names[i] + (k,), s, t, k)
        assert out[i]["status"] == 0 and out[i]["iterations"] == o["iterations"], i
        assert bool(out[i]["converged"]) == o["converged"] and out[i]["n_correspondences"] == o["n_valid"], i
        dt, dr = pose_err(out[i]["T"].reshape(4, 4).T, o["T"])
        assert dt < 1e-5 and dr < 1e-5, (i, dt, dr)


@pytest.mark.gpu
def test_gpu_covariance_read_back_arguments(gpu_ctx):
    """The read-back hook refuses what it cannot answer: a pair or a count outside the last
    registration, and any call after icp4r_gicp_covariances reused the source's buffer."""
    import icp4r

    gicp = _gicp()
    src, tgt, _ = _scene(14, 600)
    gicp.align(src, tgt, gicp.default_params(k_correspondences=5), ctx=gpu_ctx)
    assert gicp.last_align_covariances(0, 0, 600, ctx=gpu_ctx).shape == (600, 3, 3)
    for pair, which, n in ((1, 0, 600), (-1, 1, 600), (0, 2, 600), (0, 1, 601), (0, 0, 0), (0, 0, 100000)):
        with pytest.raises(icp4r.ICP4RError) as e:
            gicp.last_align_covariances(pair, which, n, ctx=gpu_ctx)
        assert e.value.code == icp4r.E_INVALID, (pair, which, n)
    gicp.covariances(src, 5, ctx=gpu_ctx)
    with pytest.raises(icp4r.ICP4RError) as e:
        gicp.last_align_covariances(0, 0, 600, ctx=gpu_ctx)
    assert e.value.code == icp4r.E_INVALID


# ------------------------------------------------------------------------------- F: batches past 8 pairs
@pytest.mark.gpu
def test_gpu_batch_of_19_pairs_equals_single_calls(gpu_ctx, oracle_mod, plan):
    """19 pairs (gicp_block's second and third rows of 8, the last one partial) of 300..1200 points,
    with a pair that stops at iteration 0 (source = target), one from a far guess (many iterations)
    and one of 12 source points at k = 20: the batch is bit-identical for one workgroup per pair
    (gicp_grid = 19), two sharing a pair's slices (40: the q += W stride) and one per slice (default),
    and to 19 single calls; pairs 0, 8 and 18 match the oracle."""
    gicp = _gicp()
    pairs, guesses = [], []
    for s in range(19):
        src, tgt, T = _scene(s, 300 + 50 * s)
        guesses.append(np.eye(4, dtype=np.float32))
        if s == 5:
            src = tgt.copy()  # converges at once
        elif s == 8:
            guesses[-1] = _far_guess()
        elif s == 11:
            src = src[:12].copy()
        elif s == 14:
            guesses[-1] = T.astype(np.float32)  # starts at the answer
        pairs.append((src, tgt))
    p = gicp.default_params(k_correspondences=20)
    fields = ("T", "iterations", "converged", "fitness", "n_correspondences", "status")
    runs = []
    for grid in (19, 40, None):
        if grid is not None:
            plan(gicp_grid=grid)
        else:
            gpu_ctx.reset_plan_options()
        b, ts = _device_batch(pairs, guesses)
        gicp.align_batch_device(b, p, ts["res"].data_ptr(), ctx=gpu_ctx)
        gpu_ctx.synchronize()
        runs.append(_batch_results(ts))
    for other in runs[:2]:
        for f in fields:
            np.testing.assert_array_equal(other[f], runs[2][f], err_msg=f)
    out = runs[2]
    for i, (s, t) in enumerate(pairs):
        r, _ = gicp.align(s, t, p, guess=guesses[i], ctx=gpu_ctx)
        np.testing.assert_array_equal(out[i]["T"], np.array(r.T, np.float32), err_msg=f"pair {i}")
        assert out[i]["iterations"] == r.iterations and out[i]["converged"] == r.converged, i
        assert out[i]["fitness"] == r.fitness and out[i]["n_correspondences"] == r.n_correspondences, i
        assert out[i]["status"] == r.status == 0, i
    assert out[5]["iterations"] == 0 and out[5]["converged"]
    assert len(set(out["iterations"].tolist())) >= 2
    for i in (0, 8, 18):
        o = oracle_mod.gicp_align(pairs[i][0], pairs[i][1], guess=guesses[i], k=20)
        assert out[i]["iterations"] == o["iterations"] and bool(out[i]["converged"]) == o["converged"], i
        assert out[i]["n_correspondences"] == o["n_valid"], i
        dt, dr = pose_err(out[i]["T"].reshape(4, 4).T, o["T"])
        assert dt < 1e-5 and dr < 1e-5, (i, dt, dr)
    assert out[8]["iterations"] > out[0]["iterations"]


# ------------------------------------------------------------------------------- G: partial gate
@pytest.mark.gpu
def test_gpu_distance_gate_rejects_some_correspondences(gpu_ctx, oracle_mod, plan):
    """A 1 m gate over 1500 inliers (nearest-neighbour distances at the true pose <= 0.02 m) and 300
    outliers 500 m above the scene, interleaved in every slice: exactly the inliers count, in the
    linearisation and in every LM trial (speculative or one by one), and the pose is the oracle's.
    No distance lies near the gate, so the count cannot flip on rounding."""
    gicp = _gicp()
    src, tgt, _ = _scene(4, 1500)
    rng = np.random.default_rng(44)
    outliers = (rng.uniform(-20.0, 20.0, (300, 3)) + [0.0, 0.0, 500.0]).astype(np.float32)
    src = np.ascontiguousarray(np.concatenate([src, outliers])[rng.permutation(1800)])
    p = gicp.default_params(k_correspondences=5, max_correspondence_distance=1.0)
    o = oracle_mod.gicp_align(src, tgt, k=5, max_correspondence_distance=1.0)
    runs = []
    for spec in (0, 2):
        plan(gicp_spec=spec)
        r, aligned = gicp.align(src, tgt, p, want_aligned=True, ctx=gpu_ctx)
        runs.append((r.matrix(), r.iterations, r.converged, r.fitness, r.status, r.n_correspondences, aligned))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert runs[0][1:6] == runs[1][1:6]
    np.testing.assert_array_equal(runs[0][6], runs[1][6])
    T, iterations, converged, _, status, ncorr, _ = runs[1]
    assert ncorr == 1500 == o["n_valid"]
    assert status == 0 and iterations == o["iterations"] and bool(converged) == o["converged"]
    dt, dr = pose_err(T, o["T"])
    assert dt < 1e-5 and dr < 1e-5, (dt, dr)


# ------------------------------------------------------------------------------- H: LM failure, no iteration
@pytest.mark.gpu
def test_gpu_lm_failure_and_zero_iterations_match_oracle(gpu_ctx, oracle_mod):
    """From the far guess of the LM-trials test: no LM trial allowed (step_lm fails in iteration 0: not
    converged, the guess returned), one trial per iteration, and no iteration at all (the guess, no
    correspondences) — each as the oracle reports it."""
    gicp = _gicp()
    src, tgt, _ = _scene(0, 2000)
    guess = _far_guess()
    r, _ = gicp.align(src, tgt, gicp.default_params(k_correspondences=5, lm_max_iterations=0), guess=guess, ctx=gpu_ctx)
    o = oracle_mod.gicp_align(src, tgt, guess=guess, k=5, lm_max_iterations=0)
    assert o["lm_failed"] and not o["converged"] and o["iterations"] == 0
    np.testing.assert_array_equal(o["T"], guess.astype(np.float64))
    assert not r.converged and r.iterations == 0
    np.testing.assert_array_equal(r.matrix(), guess)

    r, _ = gicp.align(src, tgt, gicp.default_params(k_correspondences=5, lm_max_iterations=1), guess=guess, ctx=gpu_ctx)
    o = oracle_mod.gicp_align(src, tgt, guess=guess, k=5, lm_max_iterations=1)
    assert r.iterations == o["iterations"] and bool(r.converged) == o["converged"]
    dt, dr = pose_err(r.matrix(), o["T"])
    assert dt < 1e-5 and dr < 1e-5, (dt, dr)

    r, _ = gicp.align(src, tgt, gicp.default_params(k_correspondences=5, max_iterations=0), guess=guess, ctx=gpu_ctx)
    o = oracle_mod.gicp_align(src, tgt, guess=guess, k=5, max_iterations=0)
    assert o["n_valid"] == 0 and not o["converged"] and o["iterations"] == 0
    np.testing.assert_array_equal(o["T"], guess.astype(np.float64))
    assert not r.converged and r.n_correspondences == 0
    np.testing.assert_array_equal(r.matrix(), guess)


# ------------------------------------------------------------------------------- oracle (no GPU)
def test_oracle_no_iteration_reports_no_correspondences(oracle_mod):
    """max_iterations = 0: the oracle never linearises, and reports 0 valid correspondences (its list
    starts at 'none', not unwritten memory)."""
    src, tgt, _ = _scene(4, 400)
    for _ in range(3):
        o = oracle_mod.gicp_align(src, tgt, guess=_far_guess(), k=5, max_iterations=0)
        assert o["n_valid"] == 0 and not o["converged"] and o["iterations"] == 0 and not o["lm_failed"]
        np.testing.assert_array_equal(o["T"], _far_guess().astype(np.float64))


def test_oracle_fewer_points_than_k_divides_by_cloud_size(oracle_mod):
    """The n < k rule (oracle/gicp_oracle.h): the whole cloud is the neighbour set and the divisor is
    its size — every point gets the cloud's covariance about its mean."""
    src, _, _ = _scene(7, 200)
    for n in (1, 2, 4, 12):
        c = src[:n].astype(np.float64)
        d = c - c.mean(0)
        want = d.T @ d / n
        got = oracle_mod.gicp_covariances(src[:n], 20, REG_NONE)
        np.testing.assert_allclose(got, np.broadcast_to(want, got.shape), rtol=1e-10, atol=1e-12)
