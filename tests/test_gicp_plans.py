"""Generalized ICP on every search plan it can take, its stop criteria and options against the oracle,
and invalid pairs among healthy ones in one batch (bars: tests/test_gicp.py's header, nothing new).

run_gicp borrows the ICP core's make_plan / setup_work / nn_pass; tests/test_gicp.py and
tests/test_gicp_paths.py reach only the plans small pairs and small batches pick by themselves.

  A  search plans: the batched LDS search forced (9 ragged pairs) and natural (256 pairs), declined for
     a source past 8192 points, the streamed pruned search, the tiled search's run lengths, brute force
     and the 511 / 512-target plan switch, leaf = 32
  B  rotation / transformation epsilon, iteration caps 1..7, the five regularisations inside align,
     compute_fitness = 0, byte strides of icp4r_gicp_align, per-kernel timing
  C  a mixed batch: empty, non-finite, gated, tiny and empty-source pairs beside healthy ones

Between plans and options every result row and aligned cloud is bit-identical (every search is exact
with ties to the lowest index, and a pair's sums depend on its own size only).  Against the oracle:
identical iterations, converged and valid correspondences, pose within 1e-5 (1e-4 for a cloud of
fewer than k points).  The oracle's answers are computed once per (pair, parameters) and shared.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import pose_err
from test_gicp_paths import _device_batch, _far_guess, _scene

K = 5
GUARD = 64                       # guard rows before and after a results array and an aligned cloud
GUARD_BYTE = 0xA5
SENTINEL = np.float32(-12345.5)  # what an unwritten aligned point holds
DBL_MAX = float(np.finfo(np.float64).max)
EYE = np.eye(4, dtype=np.float32)


def _gicp():
    from icp4r import gicp

    return gicp


# ------------------------------------------------------------------------------------------ helpers
_scenes = {}


def _pair(seed, n, m=None):
    """The first n source and m target points of _scene(seed, max(n, m)) (the scene's points come in
    random order, so a prefix is a uniform subsample) and its transform; each scene is made once."""
    m = n if m is None else m
    key = (seed, max(n, m))
    if key not in _scenes:
        _scenes[key] = _scene(seed, max(n, m))
    s, t, T = _scenes[key]
    return np.ascontiguousarray(s[:n]), np.ascontiguousarray(t[:m]), T


_oracle_rows = {}


def _want(oracle_mod, key, src, tgt, guess=None, **kw):
    """oracle.gicp_align once per (key, parameters); k = 5 unless given."""
    kw.setdefault("k", K)
    kk = (key, tuple(sorted(kw.items())))
    if kk not in _oracle_rows:
        _oracle_rows[kk] = oracle_mod.gicp_align(src, tgt, guess=guess, **kw)
    return _oracle_rows[kk]


def _params(**kw):
    """icp4r_gicp_params from the oracle's parameter names (k -> k_correspondences)."""
    kw = dict(kw)
    kw["k_correspondences"] = kw.pop("k", K)
    return _gicp().default_params(**kw)


def _row(result):
    import icp4r

    return np.frombuffer(bytes(result), icp4r.RESULT_DTYPE)[0]


def _singles(ctx, pairs, p, guesses=None, aligned=True):
    """Every pair through icp4r_gicp_align: (rows, aligned clouds)."""
    import icp4r

    rows = np.zeros(len(pairs), icp4r.RESULT_DTYPE)
    clouds = []
    for i, (s, t) in enumerate(pairs):
        r, al = _gicp().align(s, t, p, guess=None if guesses is None else guesses[i], want_aligned=aligned, ctx=ctx)
        rows[i] = _row(r)
        clouds.append(al)
    return rows, clouds


def _prepare(pairs, guesses=None, aligned=False):
    """A device batch whose results array (and aligned cloud, if asked for) lies between GUARD guard
    rows; everything uploaded before it returns."""
    import torch

    b, ts = _device_batch(pairs, guesses)
    dev = ts["src"].device
    ts["res"] = torch.full(((len(pairs) + 2 * GUARD) * 96,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    ts["res_ptr"] = ts["res"].data_ptr() + GUARD * 96
    if aligned:
        ts["aligned"] = torch.full((ts["src"].shape[0] + 2 * GUARD, 4), float(SENTINEL), dtype=torch.float32, device=dev)
        b.aligned = ts["aligned"].data_ptr() + GUARD * 16
    torch.cuda.synchronize()
    return b, ts


def _collect(ctx, ts, pairs):
    """(rows, aligned clouds or None) of a queued batch; the guard rows must be as they were."""
    import icp4r

    ctx.synchronize()
    n = len(pairs)
    raw = ts["res"].cpu().numpy()
    assert (raw[:GUARD * 96] == GUARD_BYTE).all() and (raw[(GUARD + n) * 96:] == GUARD_BYTE).all(), "results guards"
    rows = np.frombuffer(raw[GUARD * 96:(GUARD + n) * 96].tobytes(), icp4r.RESULT_DTYPE)
    if "aligned" not in ts:
        return rows, None
    al = ts["aligned"].cpu().numpy()
    assert (al[:GUARD] == SENTINEL).all() and (al[-GUARD:] == SENTINEL).all(), "aligned guards"
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in pairs])])
    return rows, [al[GUARD + off[i]:GUARD + off[i + 1]].copy() for i in range(n)]


def _batch(ctx, pairs, p, guesses=None, aligned=True):
    b, ts = _prepare(pairs, guesses, aligned)
    _gicp().align_batch_device(b, p, ts["res_ptr"], ctx=ctx)
    return _collect(ctx, ts, pairs)


def _same(got, want, what, skip=()):
    """Result rows bit for bit (every field but those in `skip`), and aligned clouds if both are given."""
    (grows, gal), (wrows, wal) = got, want
    assert len(grows) == len(wrows), what
    for f in grows.dtype.names:
        if f in skip:
            continue
        a = np.ascontiguousarray(grows[f])
        b = np.ascontiguousarray(wrows[f])
        bad = [i for i in range(len(grows)) if a[i].tobytes() != b[i].tobytes()]
        assert not bad, (what, f, bad, a[bad[0]], b[bad[0]])
    if gal is not None and wal is not None:
        for i, (x, y) in enumerate(zip(gal, wal)):
            if x is None or y is None:
                continue
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, "aligned cloud", i)


def _sub(run, ix):
    rows, al = run
    return rows[list(ix)], None if al is None else [al[i] for i in ix]


def _assert_oracle(row, o, what, tol=1e-5):
    """The bars of tests/test_gicp.py: iterations, converged and valid correspondences identical, the
    pose within tol."""
    dt, dr = pose_err(row["T"].reshape(4, 4).T, o["T"])
    print(f"{what}: iterations {row['iterations']}/{o['iterations']} converged {row['converged']}/{int(o['converged'])} "
          f"valid {row['n_correspondences']}/{o['n_valid']} dt {dt:.3e} dr {dr:.3e}")
    assert row["status"] == 0, what
    assert row["iterations"] == o["iterations"] and bool(row["converged"]) == o["converged"], what
    assert row["n_correspondences"] == o["n_valid"], what
    assert dt < tol and dr < tol, (what, dt, dr)


def _state(o, cap):
    """convergence_state as gicp_trial_kernel writes it: 2 converged, 1 the last allowed iteration ran
    without converging, 0 otherwise (a failed LM step)."""
    return 2 if o["converged"] else 0 if o["lm_failed"] else 1 if o["iterations"] + 1 >= cap else 0


def _options(ctx, plan, **options):
    """Exactly these plan options, through the plan fixture (which restores the defaults)."""
    ctx.reset_plan_options()
    plan(**options)


# ------------------------------------------------------------------------------- A1: forced LDS plan
# (source, target) sizes: sources across the 256-point slice edges, targets at the plan's edges (512 the
# pruned minimum, 8192 the LDS maximum); 9 pairs: gicp_block's second row of 8 holds one
LDS_SIZES = ((255, 512), (256, 513), (257, 1000), (1024, 4097), (1300, 8192), (2049, 600), (1024, 1000), (600, 600),
             (300, 2000))
LDS_ORACLE = (0, 4, 6)


def _lds_pairs():
    pairs, guesses = [], []
    for i, (n, m) in enumerate(LDS_SIZES):
        s, t, _ = _pair(20 + i, n, m)
        pairs.append((t.copy(), t) if i == 7 else (s, t))  # pair 7: source = target, stops at iteration 0
        guesses.append(_far_guess() if i == 6 else EYE)
    return pairs, guesses


def test_oracle_lds_pairs_stop_apart(oracle_mod):
    """The forced-LDS batch's oracle pairs: the far guess iterates longest, the identical pair (not an
    oracle pair of the GPU test, checked here) stops at iteration 0."""
    pairs, guesses = _lds_pairs()
    o = [_want(oracle_mod, ("lds", i), *pairs[i], guess=guesses[i]) for i in LDS_ORACLE + (7,)]
    assert all(r["rc"] == 0 and not r["lm_failed"] for r in o)
    assert o[3]["converged"] and o[3]["iterations"] == 0
    assert o[2]["iterations"] > max(o[0]["iterations"], o[1]["iterations"]) > 0


@pytest.mark.gpu
def test_gpu_forced_lds_plan(gpu_ctx, oracle_mod, plan):
    """nn_lds_kernel without the cached-neighbour test (GICP forces cache = false) under the GICP
    iteration kernels, which read the keys by source index: 9 ragged pairs with nn_lds = 1 equal the
    tiled search (nn_lds = 0), the same plan with src_order = 0 and with kd = 0 (Morton indices), and 9
    single calls, bit for bit; three pairs match the oracle."""
    import icp4r

    pairs, guesses = _lds_pairs()
    p = _params()
    mn, mm = max(len(s) for s, _ in pairs), max(len(t) for _, t in pairs)
    runs = {}
    for name, options in (("lds", dict(nn_lds=1)), ("tiled", dict(nn_lds=0)), ("lds, src_order = 0", dict(nn_lds=1, src_order=0)),
                          ("lds, kd = 0", dict(nn_lds=1, kd=0))):
        _options(gpu_ctx, plan, **options)
        pl = icp4r.plan(len(pairs), mn, mm, ctx=gpu_ctx)
        assert pl["pruned"] and bool(pl["lds"]) == (options["nn_lds"] == 1), (name, pl)
        runs[name] = _batch(gpu_ctx, pairs, p, guesses)
    gpu_ctx.reset_plan_options()
    for name in runs:
        _same(runs[name], runs["lds"], name)
    _same(_singles(gpu_ctx, pairs, p, guesses), runs["lds"], "single calls")
    rows = runs["lds"][0]
    assert (rows["status"] == 0).all() and rows[7]["iterations"] == 0 and rows[7]["converged"]
    for i in LDS_ORACLE:
        _assert_oracle(rows[i], _want(oracle_mod, ("lds", i), *pairs[i], guess=guesses[i]), f"pair {i}")
    assert rows[6]["iterations"] > rows[0]["iterations"]


# ------------------------------------------------------------------------------ A2: natural LDS plan
def _natural_pairs():
    """256 pairs of 290..310 source and 512..600 target points cut from 16 scenes of 600."""
    pairs = []
    for i in range(256):
        s, t, _ = _pair(40 + i % 16, 600)
        n, m = 290 + (7 * i) % 21, 512 + (11 * i) % 89
        o = (13 * i) % (600 - n)
        pairs.append((np.ascontiguousarray(s[o:o + n]), np.ascontiguousarray(t[:m])))
    return pairs


@pytest.mark.gpu
def test_gpu_natural_lds_plan(gpu_ctx, oracle_mod, plan):
    """256 pairs (kLdsMinPairs) take the batched LDS search with no option set: the batch equals itself
    on the tiled search and, for the shared pairs, the 255-pair batch (whose plan is not LDS), bit for
    bit; pairs 0, 127 and 255 equal single calls and the oracle."""
    import icp4r

    pairs = _natural_pairs()
    p = _params()
    mn, mm = max(len(s) for s, _ in pairs), max(len(t) for _, t in pairs)
    gpu_ctx.reset_plan_options()
    assert icp4r.plan(256, mn, mm, ctx=gpu_ctx)["lds"] == 1
    assert icp4r.plan(255, mn, mm, ctx=gpu_ctx)["lds"] == 0
    natural = _batch(gpu_ctx, pairs, p)
    short = _batch(gpu_ctx, pairs[:255], p)
    _options(gpu_ctx, plan, nn_lds=0)
    assert icp4r.plan(256, mn, mm, ctx=gpu_ctx)["lds"] == 0
    tiled = _batch(gpu_ctx, pairs, p)
    gpu_ctx.reset_plan_options()
    _same(tiled, natural, "nn_lds = 0")
    _same(short, _sub(natural, range(255)), "255 pairs")
    ix = (0, 127, 255)
    _same(_singles(gpu_ctx, [pairs[i] for i in ix], p), _sub(natural, ix), "single calls")
    assert (natural[0]["status"] == 0).all() and len(set(natural[0]["iterations"].tolist())) >= 2
    for i in ix:
        _assert_oracle(natural[0][i], _want(oracle_mod, ("natural", i), *pairs[i]), f"pair {i}")


# --------------------------------------------------------------------------------- A3: LDS declined
@pytest.mark.gpu
def test_gpu_lds_declined_for_large_source(gpu_ctx, oracle_mod, plan):
    """An 8200-point source against 600 targets with nn_lds = 1: the ICP core's plan for the shape is
    the LDS search, but GICP's index strides cover the source too (8200 > the 8192 targets the search
    stages), so run_gicp passes allow_lds = false: the result equals nn_lds = 0 and the oracle."""
    import icp4r

    s, t, _ = _pair(65, 8200, 600)
    p = _params()
    _options(gpu_ctx, plan, nn_lds=1)
    assert icp4r.plan(1, len(s), len(t), ctx=gpu_ctx)["lds"] == 1
    forced = _singles(gpu_ctx, [(s, t)], p)
    batch = _batch(gpu_ctx, [(s, t)], p)
    _options(gpu_ctx, plan, nn_lds=0)
    plain = _singles(gpu_ctx, [(s, t)], p)
    gpu_ctx.reset_plan_options()
    _same(forced, plain, "nn_lds = 1 against 0")
    _same(batch, plain, "device batch, nn_lds = 1")
    _assert_oracle(forced[0][0], _want(oracle_mod, "declined", s, t), "8200 / 600")


# ------------------------------------------------------------------- A4, A5, A7: the unbatched plans
def _one_pair():
    s, t, _ = _pair(61, 2000)
    return [(s, t)]


def _two_tile_pair():
    s, t, _ = _pair(62, 3000, 8193)
    return [(s, t)]


def _three_pairs():
    """Targets of 600, 4097 and 8193 points on one set of strides (two target tiles; the streamed
    search cuts 8193 targets into 2 chunks of 64 superblocks or 5 of 16)."""
    return [_pair(63, 700, 600)[:2], _pair(64, 1500, 4097)[:2], _pair(62, 3000, 8193)[:2]]


_default_runs = {}


def _default_run(ctx, name, pairs, single):
    """The pairs on the default plan (one-tile / two-tile nn_tile_kernel), once per module."""
    if name not in _default_runs:
        ctx.reset_plan_options()
        _default_runs[name] = _singles(ctx, pairs, _params()) if single else _batch(ctx, pairs, _params())
    return _default_runs[name]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_sb", [16, 64])
@pytest.mark.parametrize("nn_q", [1, 4])
def test_gpu_streamed_pruned_search(gpu_ctx, oracle_mod, plan, chunk_sb, nn_q):
    """nn_tile = 0: the streamed pruned search at both chunk sizes and 1 and 4 queries per lane — a
    2000 / 2000 pair and a 3-pair batch with a multi-chunk target equal the default tiled plan."""
    single, three = _one_pair(), _three_pairs()
    want1, want3 = _default_run(gpu_ctx, "one", single, True), _default_run(gpu_ctx, "three", three, False)
    _options(gpu_ctx, plan, nn_tile=0, chunk_sb=chunk_sb, nn_q=nn_q)
    got1, got3 = _singles(gpu_ctx, single, _params()), _batch(gpu_ctx, three, _params())
    gpu_ctx.reset_plan_options()
    _same(got1, want1, "2000 / 2000")
    _same(got3, want3, "3-pair batch")
    assert (want1[0]["status"] == 0).all() and (want3[0]["status"] == 0).all()
    if (chunk_sb, nn_q) == (16, 1):
        _assert_oracle(want1[0][0], _want(oracle_mod, "one", *single[0]), "2000 / 2000")
        _assert_oracle(want3[0][2], _want(oracle_mod, "two-tile", *three[2]), "3000 / 8193")


@pytest.mark.gpu
@pytest.mark.parametrize("tile_run", [8, 16, 32, 64])
def test_gpu_tiled_search_run_lengths(gpu_ctx, plan, tile_run):
    """Every run length of nn_tile_kernel on a one-tile and a two-tile pair: bit-identical."""
    one, two = _one_pair(), _two_tile_pair()
    want1, want2 = _default_run(gpu_ctx, "one", one, True), _default_run(gpu_ctx, "two", two, True)
    _options(gpu_ctx, plan, tile_run=tile_run)
    got1, got2 = _singles(gpu_ctx, one, _params()), _singles(gpu_ctx, two, _params())
    gpu_ctx.reset_plan_options()
    _same(got1, want1, "one tile")
    _same(got2, want2, "two tiles")


@pytest.mark.gpu
def test_gpu_leaf_32(gpu_ctx, plan):
    """Plan option leaf = 32 (32-target blocks, the streamed search): the k-NN covariance walk reads
    16-target blocks only, so the covariances come from the brute-force kernel (the same neighbour
    sets) — a pruned single pair, the 3-pair batch and icp4r_gicp_covariances return ICP4R_OK and the
    bits of leaf = 16, and the next registrations on the context, options reset, equal their own
    earlier results.  (Before this was decided ahead of the aux-stream fork every such call failed
    with ICP4R_E_HIP, launch_gicp_knn_cov refusing the index.)"""
    import icp4r

    gicp = _gicp()
    one, three = _one_pair(), _three_pairs()
    cloud = _pair(65, 1003)[1]
    want1, want3 = _default_run(gpu_ctx, "one", one, True), _default_run(gpu_ctx, "three", three, False)
    gpu_ctx.reset_plan_options()
    wantc = gicp.covariances(cloud, K, ctx=gpu_ctx)
    _options(gpu_ctx, plan, leaf=32)
    pl = icp4r.plan(3, 3000, 8193, ctx=gpu_ctx)
    assert pl["pruned"] and pl["leaf"] == 32 and not pl["lds"]
    got1, got3 = _singles(gpu_ctx, one, _params()), _batch(gpu_ctx, three, _params())
    gotc = gicp.covariances(cloud, K, ctx=gpu_ctx)
    gpu_ctx.reset_plan_options()
    assert (got1[0]["status"] == 0).all() and (got3[0]["status"] == 0).all()
    _same(got1, want1, "2000 / 2000 at leaf = 32")
    _same(got3, want3, "3-pair batch at leaf = 32")
    np.testing.assert_array_equal(gotc, wantc)
    _same(_singles(gpu_ctx, one, _params()), want1, "2000 / 2000 after the reset")
    _same(_batch(gpu_ctx, three, _params()), want3, "3-pair batch after the reset")


# ------------------------------------------------------------------------------------ A6: brute plan
BRUTE_SOURCES = (300, 2100, 400, 511, 700, 2100, 300, 1000, 350)


def _brute_pairs():
    return [_pair(70 + i, n, 511)[:2] for i, n in enumerate(BRUTE_SOURCES)]


@pytest.mark.gpu
def test_gpu_brute_plan(gpu_ctx, oracle_mod, plan):
    """Targets of 511 points (below the pruned minimum): brute-force NN and covariances, 1 and 4 queries
    per lane, single calls and a 9-pair batch — all identical; the 300-point pair matches the oracle."""
    import icp4r

    pairs = _brute_pairs()
    p = _params()
    runs = {}
    for q in (1, 4):
        _options(gpu_ctx, plan, nn_q=q)
        for npairs, n in ((1, 300), (1, 2100), (9, 2100)):
            assert icp4r.plan(npairs, n, 511, ctx=gpu_ctx)["pruned"] == 0
        runs[q] = _batch(gpu_ctx, pairs, p), _singles(gpu_ctx, pairs[:2], p)
    gpu_ctx.reset_plan_options()
    singles = _singles(gpu_ctx, pairs, p)
    _same(runs[1][0], runs[4][0], "batch, nn_q 1 against 4")
    _same(runs[1][0], singles, "batch against single calls")
    for q in (1, 4):
        _same(runs[q][1], _sub(singles, (0, 1)), f"single calls, nn_q = {q}")
    assert (singles[0]["status"] == 0).all()
    _assert_oracle(singles[0][0], _want(oracle_mod, ("brute", 0), *pairs[0]), "300 / 511")


@pytest.mark.gpu
def test_gpu_plan_switch_at_512_targets(gpu_ctx, oracle_mod):
    """The same scene with 511 targets (brute force) and 512 (pruned): each matches the oracle."""
    import icp4r

    s, t, _ = _pair(79, 400, 512)
    gpu_ctx.reset_plan_options()
    for m in (511, 512):
        assert icp4r.plan(1, len(s), m, ctx=gpu_ctx)["pruned"] == (m == 512)
        rows, _ = _singles(gpu_ctx, [(s, t[:m])], _params())
        _assert_oracle(rows[0], _want(oracle_mod, ("switch", m), s, t[:m]), f"{m} targets")


# ----------------------------------------------------------------------------------- B8: epsilons
# One scene scaled to 1.6 m across, where a step's rotation and translation entries are of comparable
# size (on the 80 m scenes the translation decides alone), from a moderately wrong guess.
EPS_SCALE = np.float32(0.02)
EPS_SETTINGS = {
    "defaults": dict(rotation_epsilon=2e-3, transformation_epsilon=5e-4),
    "tightened": dict(rotation_epsilon=1e-5, transformation_epsilon=1e-6),
    "rotation loosened": dict(rotation_epsilon=2e-3, transformation_epsilon=1e-6),      # from tightened
    "translation loosened": dict(rotation_epsilon=1e-5, transformation_epsilon=5e-4),   # from tightened
}
# settings that differ in one epsilon only
EPS_ROTATION_ONLY = (("defaults", "translation loosened"), ("tightened", "rotation loosened"))
EPS_TRANSLATION_ONLY = (("defaults", "rotation loosened"), ("tightened", "translation loosened"))


def _yaw_guess(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    g = np.eye(4, dtype=np.float32)
    g[:2, :2] = [[c, -s], [s, c]]
    g[:3, 3] = t
    return g


def _eps_pairs():
    """The epsilon scene (pair 0) and three more for the batch: (pairs, guesses)."""
    pairs, guesses = [], []
    for seed, angle in ((3, 0.15), (0, 0.3), (4, 0.15), (1, -0.1)):
        s, t, _ = _pair(seed, 800)
        pairs.append((s * EPS_SCALE, t * EPS_SCALE))
        guesses.append(_yaw_guess(angle, np.array([0.3, -0.2, 0.1], np.float32) * EPS_SCALE))
    return pairs, guesses


def _eps_want(oracle_mod, i, kw):
    pairs, guesses = _eps_pairs()
    return _want(oracle_mod, ("eps", i), *pairs[i], guess=guesses[i], **kw)


def test_oracle_epsilons_each_decide(oracle_mod):
    """The oracle alone on the epsilon scene: the four settings stop at three or more different
    iterations; changing the rotation epsilon alone changes the count, and so does the translation
    epsilon alone; a setting with its two values swapped stops elsewhere (so swapped or ignored fields
    cannot pass the GPU test); and no count — of the scene or of the batch's other pairs — moves when
    the setting's epsilons are scaled by 1 +- 1e-6 (both sides decide in double; their summation orders
    differ by orders of magnitude less than that band)."""
    n = {name: _eps_want(oracle_mod, 0, kw)["iterations"] for name, kw in EPS_SETTINGS.items()}
    print(n)
    assert all(_eps_want(oracle_mod, 0, kw)["converged"] for kw in EPS_SETTINGS.values())
    assert len(set(n.values())) >= 3, n
    assert any(n[a] != n[b] for a, b in EPS_ROTATION_ONLY), n
    assert any(n[a] != n[b] for a, b in EPS_TRANSLATION_ONLY), n
    swapped = {name: _eps_want(oracle_mod, 0, dict(rotation_epsilon=kw["transformation_epsilon"],
                                                   transformation_epsilon=kw["rotation_epsilon"]))["iterations"]
               for name, kw in EPS_SETTINGS.items()}
    assert any(swapped[name] != n[name] for name in n), (n, swapped)
    for i in range(4):
        for name, kw in EPS_SETTINGS.items():
            at = _eps_want(oracle_mod, i, kw)
            for f in (1 - 1e-6, 1 + 1e-6):
                near = _eps_want(oracle_mod, i, {k: v * f for k, v in kw.items()})
                assert (near["iterations"], near["converged"]) == (at["iterations"], at["converged"]), (i, name, f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EPS_SETTINGS))
def test_gpu_epsilons_match_oracle(gpu_ctx, oracle_mod, name):
    """rotation_epsilon and transformation_epsilon through a single call and a 4-pair batch."""
    kw = EPS_SETTINGS[name]
    pairs, guesses = _eps_pairs()
    gpu_ctx.reset_plan_options()
    batch = _batch(gpu_ctx, pairs, _params(**kw), guesses)
    _same(_singles(gpu_ctx, pairs[:1], _params(**kw), guesses[:1]), _sub(batch, (0,)), "single call")
    for i in range(4):
        _assert_oracle(batch[0][i], _eps_want(oracle_mod, i, kw), f"{name}, pair {i}")


# ------------------------------------------------------------------------------ B9: iteration caps
CAPS = (1, 2, 3, 4, 5, 7)


def _cap_pairs():
    """The far-guess pair (still iterating at 7), a pair that converges at iteration 0 (source =
    target) and one that converges within the caps: (pairs, guesses)."""
    s, t, _ = _pair(0, 2000)
    s2, t2, _ = _pair(66, 1500)
    return [(s, t), (t2.copy(), t2), (s2, t2)], [_far_guess(), EYE, EYE]


def _cap_want(oracle_mod, i, cap):
    pairs, guesses = _cap_pairs()
    return _want(oracle_mod, ("cap", i), *pairs[i], guess=guesses[i], max_iterations=cap)


def test_oracle_caps_cut_the_far_guess_short(oracle_mod):
    """The oracle alone: from the far guess every cap up to 7 ends the registration unconverged at
    iteration cap - 1 (without a cap it converges later); the identical pair stops at iteration 0 and
    the third pair converges at an iteration some caps reach and others do not."""
    for cap in CAPS:
        o = _cap_want(oracle_mod, 0, cap)
        assert not o["converged"] and not o["lm_failed"] and o["iterations"] == cap - 1, cap
        assert _state(o, cap) == 1
        o = _cap_want(oracle_mod, 1, cap)
        assert o["converged"] and o["iterations"] == 0, cap
    free = _cap_want(oracle_mod, 0, 64)
    assert free["converged"] and free["iterations"] > 7
    third = _cap_want(oracle_mod, 2, 64)
    assert third["converged"] and CAPS[0] <= third["iterations"] + 1 < CAPS[-1], third["iterations"]
    assert {_cap_want(oracle_mod, 2, cap)["converged"] for cap in CAPS} == {False, True}


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
def test_gpu_iteration_caps_match_oracle(gpu_ctx, oracle_mod, cap):
    """max_iterations at odd and even values around the host's active-pair check (queued after every
    second iteration but the last, read one check late): iterations, converged, convergence_state (the
    it + 1 >= max_iterations branch of gicp_trial_kernel) and the pose as the oracle's; the 3-pair batch
    equals single calls bit for bit."""
    pairs, guesses = _cap_pairs()
    p = _params(max_iterations=cap)
    gpu_ctx.reset_plan_options()
    batch = _batch(gpu_ctx, pairs, p, guesses)
    _same(_singles(gpu_ctx, pairs, p, guesses), batch, "single calls")
    for i in range(3):
        o = _cap_want(oracle_mod, i, cap)
        _assert_oracle(batch[0][i], o, f"cap {cap}, pair {i}")
        assert batch[0][i]["convergence_state"] == _state(o, cap), (cap, i, batch[0][i]["convergence_state"])
    assert batch[0][0]["iterations"] == cap - 1 and batch[0][0]["convergence_state"] == 1


@pytest.mark.gpu
def test_gpu_capped_calls_back_to_back(gpu_ctx):
    """The 3-pair batch at caps 3 and 4, each queued twice with no synchronisation in between (as
    test_gicp.py::test_gpu_device_calls_back_to_back): every call's rows equal the synchronised run's."""
    gicp = _gicp()
    pairs, guesses = _cap_pairs()
    gpu_ctx.reset_plan_options()
    want = {cap: _batch(gpu_ctx, pairs, _params(max_iterations=cap), guesses) for cap in (3, 4)}
    queued = [(cap, *_prepare(pairs, guesses, True)) for cap in (3, 4, 3, 4)]
    for cap, b, ts in queued:
        gicp.align_batch_device(b, _params(max_iterations=cap), ts["res_ptr"], ctx=gpu_ctx)
    for k, (cap, b, ts) in enumerate(queued):
        _same(_collect(gpu_ctx, ts, pairs), want[cap], f"call {k}, cap {cap}")


# ------------------------------------------------------------------ B10: regularisations inside align
@pytest.mark.gpu
@pytest.mark.parametrize("reg", [0, 1, 2, 3, 4])
def test_gpu_align_every_regularisation(gpu_ctx, oracle_mod, reg):
    """NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE and FROBENIUS through align (tested so far in the
    covariance call only) on a 1500-point pair."""
    s, t, _ = _pair(67, 1500)
    gpu_ctx.reset_plan_options()
    rows, _ = _singles(gpu_ctx, [(s, t)], _params(regularization=reg))
    _assert_oracle(rows[0], _want(oracle_mod, "reg", s, t, regularization=reg), f"regularization {reg}")


# --------------------------------------------------------------------------- B11: compute_fitness = 0
@pytest.mark.gpu
def test_gpu_compute_fitness_off(gpu_ctx):
    """compute_fitness = 0, with and without an aligned cloud, single call and batch: everything but the
    fitness — pose, counts, flags and the aligned cloud (fitness_prep_kernel still runs for it) — is
    bit-identical to compute_fitness = 1, and the fitness is DBL_MAX, finish_kernel's value for "not
    computed" (r.fitness = (have && fcnt > 0) ? fsum / fcnt : DBL_MAX, have = ... compute_fitness ...)."""
    pairs = [_pair(63, 700, 600)[:2], _pair(67, 1500)[:2], _pair(61, 2000)[:2]]
    guesses = [EYE, _far_guess(), EYE]
    gpu_ctx.reset_plan_options()
    on = _batch(gpu_ctx, pairs, _params(), guesses)
    assert (on[0]["status"] == 0).all() and (on[0]["fitness"] != DBL_MAX).all()
    off = _params(compute_fitness=0)
    for aligned in (True, False):
        for what, got in (("batch", _batch(gpu_ctx, pairs, off, guesses, aligned)),
                          ("single calls", _singles(gpu_ctx, pairs, off, guesses, aligned))):
            _same(got, on, f"{what}, aligned {aligned}", skip=("fitness",))
            assert (got[0]["fitness"] == DBL_MAX).all(), (what, aligned, got[0]["fitness"])
            if aligned:
                assert all(a is not None for a in got[1])
    _same(_singles(gpu_ctx, pairs, _params(), guesses), on, "single calls, compute_fitness = 1")


# ------------------------------------------------------------------------------------ B12: strides
def _records(xyz, stride, fourth):
    """xyz as records of `stride` bytes: the 4th float (if any) from `fourth`, NaN guard floats in the
    rest of each record and in 8 floats after the last one."""
    f = stride // 4
    buf = np.full(len(xyz) * f + 8, np.nan, np.float32)
    rec = buf[:len(xyz) * f].reshape(len(xyz), f)
    rec[:, :3] = xyz
    if f >= 4:
        rec[:, 3] = fourth
    return buf


def _align_raw(ctx, sbuf, n, sstride, tbuf, m, tstride, p, obuf=None, ostride=16):
    import icp4r

    r = icp4r.Result()
    rc = _gicp()._lib().icp4r_gicp_align(ctx.handle, sbuf.ctypes.data, n, sstride, tbuf.ctypes.data, m, tstride, None,
                                         C.byref(p), C.byref(r), None if obuf is None else obuf.ctypes.data, ostride)
    return rc, r


@pytest.mark.gpu
def test_gpu_align_strides(gpu_ctx):
    """icp4r_gicp_align with source and target records of 12, 16, 20 and 32 bytes and aligned_out records
    of 12, 16 and 32: the registration is the packed call's bit for bit (NaN guard floats in every
    record's tail and after the last record are never read as coordinates), the output's guard floats
    stay untouched, and the 4th float travels only where both the source's and the output's records
    have one (a 12-byte source gives 0).  Strides below 12 or no multiple of 4 are ICP4R_E_INVALID."""
    import icp4r

    s, t, _ = _pair(67, 1500)
    n, m = len(s), len(t)
    p = _params()
    inten = np.arange(n, dtype=np.float32) + np.float32(0.25)
    tfourth = np.full(m, np.nan, np.float32)  # a target's 4th float is never a coordinate
    gpu_ctx.reset_plan_options()
    (want, ), (want_al, ) = _singles(gpu_ctx, [(s, t)], p)
    assert want["status"] == 0 and want["iterations"] > 0
    strides = (12, 16, 20, 32)
    for a, ss in enumerate(strides):
        for b, tstr in enumerate(strides):
            ostride = (12, 16, 32)[(a + b) % 3]
            sbuf, tbuf = _records(s, ss, inten), _records(t, tstr, tfourth)
            keep = sbuf.tobytes(), tbuf.tobytes()
            fo = ostride // 4
            obuf = np.full(n * fo + 8, SENTINEL, np.float32)
            rc, r = _align_raw(gpu_ctx, sbuf, n, ss, tbuf, m, tstr, p, obuf, ostride)
            what = (ss, tstr, ostride)
            assert rc == icp4r.OK, what
            assert bytes(r) == want.tobytes(), what
            assert (sbuf.tobytes(), tbuf.tobytes()) == keep, what
            rec = obuf[:n * fo].reshape(n, fo)
            assert rec[:, :3].tobytes() == np.ascontiguousarray(want_al[:, :3]).tobytes(), what
            if fo >= 4:
                np.testing.assert_array_equal(rec[:, 3], inten if ss >= 16 else np.zeros(n, np.float32), err_msg=str(what))
                assert (rec[:, 4:] == SENTINEL).all(), what
            assert (obuf[n * fo:] == SENTINEL).all(), what
    sbuf, tbuf = _records(s, 16, inten), _records(t, 16, tfourth)
    obuf = np.full(n * 8 + 8, SENTINEL, np.float32)
    for ss, tstr, ostride in ((8, 16, 16), (14, 16, 16), (16, 0, 16), (16, 18, 16), (16, 16, 8), (16, 16, 14), (-12, 16, 16)):
        rc, _ = _align_raw(gpu_ctx, sbuf, n, ss, tbuf, m, tstr, p, obuf, ostride)
        assert rc == icp4r.E_INVALID, (ss, tstr, ostride, rc)
    assert (obuf == SENTINEL).all()
    rc, r = _align_raw(gpu_ctx, sbuf, n, 16, tbuf, m, 16, p, None, 0)  # (no output: its stride is not looked at)
    assert rc == icp4r.OK and bytes(r) == want.tobytes()


# --------------------------------------------------------------------------- B13: per-kernel timing
def _iteration_launches(stop, cap):
    """Iteration launches run_gicp queues: a count of active pairs is queued after every second
    iteration except the last allowed one, and read only after the next count is queued (one check of
    lookahead); the loop ends when the count read is 0.  stop: the iteration after which no pair is
    active (None: some pair runs into the cap)."""
    prev = None
    for it in range(cap):
        if (it + 1) % 2 == 0 and it + 1 < cap:
            if prev is not None and stop is not None and stop <= prev:
                return it + 1
            prev = it
    return cap


def test_iteration_launch_count_rule():
    """The rule above at its edges: a pair stopping at iteration 0 of 64 still gets 4 launches (the
    first count, after iteration 1, is read after iteration 3); caps too short for two counts run out."""
    assert _iteration_launches(0, 64) == 4 and _iteration_launches(1, 64) == 4 and _iteration_launches(2, 64) == 6
    assert _iteration_launches(3, 64) == 6 and _iteration_launches(None, 64) == 64
    assert [_iteration_launches(0, cap) for cap in (1, 2, 3, 4, 5, 6)] == [1, 2, 3, 4, 4, 4]
    assert _iteration_launches(3, 6) == 6 and _iteration_launches(3, 7) == 6 and _iteration_launches(3, 8) == 6


@pytest.mark.gpu
def test_gpu_per_kernel_timing(gpu_ctx):
    """icp4r_set_kernel_timing(1): the registration is bit-identical, ICP4R_STAGE_GICP_COV reports one
    launch per call (both clouds' covariances between one pair of events) with a positive time, and the
    UPDATE stage one launch per iteration queued — which pins the host loop's check spacing and its
    one-check-late read at odd and even caps, for a single call and a batch."""
    import icp4r

    gicp = _gicp()
    pairs, guesses = _cap_pairs()
    gpu_ctx.reset_plan_options()
    caps = (64, 4, 5, 6, 7, 8)
    want = {cap: _batch(gpu_ctx, pairs, _params(max_iterations=cap), guesses) for cap in caps}
    assert want[64][0][2]["converged"] and 1 <= want[64][0][2]["iterations"] <= 5

    def stop(rows):
        running = [(not r["converged"]) and r["convergence_state"] == 1 for r in rows]
        return None if any(running) else int(max(r["iterations"] for r in rows))

    gpu_ctx.set_kernel_timing(True)
    try:
        for cap in caps:
            p = _params(max_iterations=cap)
            for what, ix in (("single", (2,)), ("batch", (0, 1, 2)), ("batch of stopping pairs", (1, 2))):
                ps, gs = [pairs[i] for i in ix], [guesses[i] for i in ix]
                gpu_ctx.reset_timers()
                got = _singles(gpu_ctx, ps, p, gs) if what == "single" else _batch(gpu_ctx, ps, p, gs)
                gpu_ctx.synchronize()
                _same(got, _sub(want[cap], ix), f"{what}, cap {cap}, timing on")
                cov_ms, cov_n = gpu_ctx.stage_time_ms(icp4r.STAGE_GICP_COV)
                _, upd_n = gpu_ctx.stage_time_ms(icp4r.STAGE_UPDATE)
                _, batch_n = gpu_ctx.stage_time_ms(icp4r.STAGE_BATCH)
                print(f"{what} cap {cap}: covariances {cov_ms:.4f} ms x {cov_n}, iteration launches {upd_n}")
                assert cov_n == 1 and cov_ms > 0.0 and batch_n == 1, (what, cap)
                assert upd_n == _iteration_launches(stop(got[0]), cap), (what, cap, upd_n, stop(got[0]))
    finally:
        gpu_ctx.set_kernel_timing(False)
        gpu_ctx.reset_timers()
    _same(_batch(gpu_ctx, pairs, _params(max_iterations=64), guesses), want[64], "timing off again")


# ------------------------------------------------------------------------ C14: invalid among healthy
MIXED_K = 20
MIXED_GATE = 1.0
HEALTHY = (1, 3, 5, 6, 9)
INVALID = {0: "empty target", 2: "NaN in the target", 7: "Inf in the source"}


def _moved(src, T):
    """The source in the target's frame (T = the scene's transform), so that the 1 m gate keeps every
    correspondence from the identity and from the small guesses below."""
    return np.ascontiguousarray((src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32))


def _mixed_pairs():
    """11 pairs, bad ones first, at gicp_block's row edge (7, 8) and last, and a small guess per pair
    (0.1-0.5 m at the scene's edge: far inside the gate): (pairs, guesses)."""
    sizes = {1: (600, 600), 3: (900, 900), 5: (1100, 1100), 6: (300, 800), 9: (1300, 1300)}
    pairs = [None] * 11
    for i, (n, m) in sizes.items():
        s, t, T = _pair(80 + i, n, m)
        pairs[i] = (_moved(s, T), t)
    s, t, T = _pair(90, 700)
    s = _moved(s, T)
    pairs[0] = (s[:400].copy(), t[:0].copy())                      # empty target
    bad = t.copy()
    bad[333, 1] = np.nan
    pairs[2] = (s.copy(), bad)                                     # a NaN in the target
    pairs[4] = (s[:500] + np.float32(100.0), t.copy())             # gated to zero correspondences
    bad = s[:650].copy()
    bad[649, 2] = np.inf
    pairs[7] = (bad, t.copy())                                     # an Inf in the source
    pairs[8] = (s[:12].copy(), t.copy())                           # 12 source points at k = 20
    pairs[10] = (s[:0].copy(), t[:500].copy())                     # empty source
    guesses = [_yaw_guess(0.001 * (1 + i % 3), np.array([0.05, -0.03, 0.01], np.float32) * (1 + i % 2)) for i in range(11)]
    return pairs, guesses


def test_oracle_mixed_batch_pairs(oracle_mod):
    """The oracle alone on the mixed batch's pairs: the gated pair has no correspondence and "converges"
    at once where it starts, the empty source and the empty target are refused (-2), the healthy pairs
    and the 12-point source keep every correspondence inside the gate and iterate."""
    pairs, guesses = _mixed_pairs()
    kw = dict(k=MIXED_K, max_correspondence_distance=MIXED_GATE)
    for g in (None, guesses[4]):
        o = oracle_mod.gicp_align(*pairs[4], guess=g, **kw)
        assert o["rc"] == 0 and o["n_valid"] == 0 and o["converged"] and o["iterations"] == 0
        np.testing.assert_array_equal(o["T"], np.eye(4) if g is None else g.astype(np.float64))
    assert oracle_mod.gicp_align(*pairs[10], **kw)["rc"] == -2 and oracle_mod.gicp_align(*pairs[0], **kw)["rc"] == -2
    for i in (1, 9, 8):
        for with_guess in (False, True):
            o = _want(oracle_mod, ("mixed", i, with_guess), *pairs[i], guess=guesses[i] if with_guess else None, **kw)
            assert o["rc"] == 0 and o["converged"] and not o["lm_failed"] and o["n_valid"] == len(pairs[i][0]), (i, with_guess)
            assert o["iterations"] >= 1 or not with_guess, (i, with_guess)


@pytest.mark.gpu
@pytest.mark.parametrize("with_guess", [False, True])
def test_gpu_invalid_pairs_among_healthy(gpu_ctx, oracle_mod, with_guess):
    """A device batch of 5 healthy and 6 bad pairs at k = 20 with a 1 m gate, once from the identity and
    once with a guess per pair, the aligned cloud asked for, 64 guard rows around the results and the
    aligned cloud: the healthy rows and clouds are those of the batch without the bad pairs and of
    single calls, bit for bit; every bad row equals the pair's own single call — an empty target
    ICP4R_E_EMPTY, a NaN / Inf ICP4R_E_NONFINITE (identity, not converged, nothing written to their
    aligned points); the gated pair converged after 0 iterations where it started with no
    correspondence; 12 source points at k = 20 as the oracle (1e-4: fewer points than k); the empty
    source (no oracle: it returns -2) by the rule of DESIGN.md §6d — like the gated pair, its fitness
    DBL_MAX.
    (Measured on the MI355X before gicp_knn_cov_kernel skipped invalid pairs: on a context that had run
    larger registrations it walked the earlier call's index left under each invalid pair and wrote
    covariances to that index's point numbers, past the pair's rows into the next pairs' — healthy pairs
    3 and 9 of this batch, then all five, came out with other poses than in the batch without the bad
    pairs; on a fresh context, whose workspace is zero, nothing showed.)"""
    import icp4r

    pairs, guesses = _mixed_pairs()
    g = guesses if with_guess else None
    start = lambda i: guesses[i] if with_guess else EYE  # noqa: E731
    kw = dict(k=MIXED_K, max_correspondence_distance=MIXED_GATE)
    want = lambda i: _want(oracle_mod, ("mixed", i, with_guess), *pairs[i], guess=g and g[i], **kw)  # noqa: E731
    p = _params(**kw)
    gpu_ctx.reset_plan_options()
    # a larger call first: it leaves its index in the workspace, under the invalid pairs too, which build
    # none of their own (see the docstring's last sentence)
    s2k, t2k, _ = _pair(61, 2000)
    _batch(gpu_ctx, [(s2k, t2k)] * 11, p, aligned=False)
    mixed = _batch(gpu_ctx, pairs, p, g)
    healthy = _batch(gpu_ctx, [pairs[i] for i in HEALTHY], p, g and [g[i] for i in HEALTHY])
    _same(_sub(mixed, HEALTHY), healthy, "healthy pairs, with and without the bad ones")
    rows, clouds = mixed
    singles = _singles(gpu_ctx, pairs, p, g)
    valid = [i for i in range(11) if i not in INVALID]
    _same(_sub(mixed, valid), _sub(singles, valid), "single calls")
    _same((rows[list(INVALID)], None), (singles[0][list(INVALID)], None), "single calls, invalid pairs")
    print(rows[["iterations", "converged", "status", "convergence_state", "n_correspondences", "fitness"]])
    for i in HEALTHY:
        assert rows[i]["status"] == 0 and rows[i]["converged"] == 1 and rows[i]["n_correspondences"] == len(pairs[i][0]), i
    for i in (1, 9):
        _assert_oracle(rows[i], want(i), f"pair {i}")
    _assert_oracle(rows[8], want(8), "12 source points", tol=1e-4)
    for i, what in INVALID.items():
        assert rows[i]["status"] == (icp4r.E_EMPTY if i == 0 else icp4r.E_NONFINITE), what
        assert rows[i]["converged"] == 0 and rows[i]["iterations"] == 0 and rows[i]["n_correspondences"] == 0, what
        assert rows[i]["fitness"] == DBL_MAX, what
        np.testing.assert_array_equal(rows[i]["T"].reshape(4, 4).T, EYE, err_msg=what)
        assert len(clouds[i]) == len(pairs[i][0]) and (clouds[i] == SENTINEL).all(), what
    for i in (4, 10):  # no correspondence: the first LM step is the identity, "converged"
        assert rows[i]["status"] == 0 and rows[i]["converged"] == 1 and rows[i]["iterations"] == 0, i
        assert rows[i]["n_correspondences"] == 0 and rows[i]["convergence_state"] == 2, i
        np.testing.assert_array_equal(rows[i]["T"].reshape(4, 4).T, start(i), err_msg=str(i))
    assert rows[4]["fitness"] > 1e3 and rows[10]["fitness"] == DBL_MAX and clouds[10].shape == (0, 4)
