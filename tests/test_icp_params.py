"""ICP parity with the oracle over the parameter and input space, on every execution plan.

The other ICP modules pin each plan (solo_kernel, the held / wide / 256-thread single-pair updates,
the multi-tile target with and without fold_keys, brute force, the batched LDS plan's
fold_update_kernel with lazy_x on and off, the unfused test, the record form, fold_update_res_kernel,
the sums tail, and the small batch) to the oracle with PCL's default parameters, Huber weights and a
distance threshold.  This module runs the rest of what a caller can set or feed in through ALL of
them (`_run` asserts through icp4r.plan() that the plan named was really taken):

1. convergence criteria: the similar-transforms counter, the relative and absolute MSE criteria, the
   explicit rotation threshold, mixed stops, with rejections, both parities of max_iterations;
2. per-pair guesses in a batch (exact identity rows at the batch's and the pair groups' edges), on
   the host and the device entry, and single pairs with a guess;
3. invalid pairs and pairs with too few correspondences beside healthy ones, a pair that runs out
   of correspondences after it has iterated, min_correspondences above a pair's size;
4. coordinates whose squared distances overflow (3e19) or are merely huge (2e17), through align,
   nearest and fitness;
5. 12-, 16-, 20- and 32-byte point strides and the output stride;
6. F64 numerics in a batch against the F64 oracle (the only comparison here with a tolerance: the
   bars of test_icp_f64_numerics_vs_oracle_f64).

"Equal to the oracle" is status, iterations, converged, convergence_state, n_correspondences equal,
T and fitness equal in bits, the aligned xyz equal in bits and the intensity copied through, for
EVERY pair of every batch.  The tests without the gpu marker check, with the oracle alone, that the
inputs still reach the states the GPU tests are about (a drift of icp4r.synth must not hollow them
out).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import pose_err

gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------- inputs
SHAPES = [(700, 650), (1024, 1024), (600, 900), (1500, 1200), (2048, 1500), (900, 2048), (513, 700), (1100, 640)]
NPAIRS = 260                      # >= 256 pairs: the batched LDS plan, in its two default pair groups
ALL = tuple(range(NPAIRS))
FIRST48 = tuple(range(48))        # the pairs the oracle-only conditions are stated on
SINGLE = tuple(range(16))         # the pairs run one by one on the single-pair plans
SMALL = (0, 3, 4, 8, 14)          # the 5-pair batch (sources above 1024: not solo_kernel)
EDGES = (0, NPAIRS // 2 - 1, NPAIRS // 2, NPAIRS - 1)  # first, last, both sides of the group boundary
FIXED = dict(mse_threshold_absolute=-1.0, transformation_epsilon=-1.0)

CONV_ITERATIONS, CONV_TRANSFORM, CONV_ABS_MSE, CONV_REL_MSE, CONV_NO_CORR = 1, 2, 3, 4, 5
E_EMPTY, E_TOO_FEW_CORR, E_NONFINITE = -2, -3, -4

_D = dict(max_iterations=12, transformation_epsilon=1e-7, euclidean_fitness_epsilon=2e-3,
          max_iterations_similar_transforms=1)
SETS = {
    "A": dict(max_iterations=30, transformation_epsilon=1e-6, max_iterations_similar_transforms=2),
    "B": dict(max_iterations=30, euclidean_fitness_epsilon=1e-3, mse_threshold_absolute=-1.0),
    "C": dict(max_iterations=30, mse_threshold_absolute=1e-4, max_iterations_similar_transforms=3),
    "D": dict(_D, mse_threshold_absolute=1e-5),
    "E": dict(max_iterations=30, transformation_epsilon=1e-3, transformation_rotation_epsilon=0.99999999),
    "F": dict(_D, mse_threshold_absolute=-1.0, max_correspondence_distance=1.0),
}
# the states each set reaches on FIRST48 and the range of its stop iterations there
SET_STATES = {
    "A": ({CONV_TRANSFORM}, (6, 15)), "B": ({CONV_REL_MSE}, (4, 9)), "C": ({CONV_ABS_MSE}, (7, 14)),
    "D": ({CONV_TRANSFORM, CONV_REL_MSE}, (4, 12)), "E": ({CONV_TRANSFORM}, (3, 30)),
    "F": ({CONV_ITERATIONS, CONV_TRANSFORM, CONV_REL_MSE}, (4, 12)),
}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _pair(k):
    """Pair k of the batch: shape SHAPES[k % 8], seeded 4000 + k."""
    from icp4r import synth

    p = synth.make_pair(4000 + k, *SHAPES[k % len(SHAPES)])
    return _frozen(p.src_xyzi(), p.tgt_xyzi())


@functools.lru_cache(maxsize=None)
def _mt_pair(i):
    """A 700 x 9000 pair: a target of two 8192-point tiles (the scan-to-map plan)."""
    from icp4r import synth

    p = synth.make_pair(4300 + i, 700, 9000)
    return _frozen(p.src_xyzi(), p.tgt_xyzi())


def _pairs(ix):
    return [_pair(k) for k in ix]


def _key(kw):
    return tuple(sorted(kw.items()))


_ORACLE = {}


def _oracle(oracle_mod, tag, pairs, kw, guesses=None):
    """The oracle's rows (aligned clouds included) of `pairs` under `kw`, computed once per (tag, kw):
    tag names the pair list (and its guesses)."""
    key = (tag, _key(kw))
    if key not in _ORACLE:
        kw = dict(kw)
        kw.setdefault("numerics", oracle_mod.NUM_F32)
        _ORACLE[key] = [oracle_mod.align(s, t, guess=None if guesses is None else guesses[k], aligned=True, **kw)
                        for k, (s, t) in enumerate(pairs)]
    return _ORACLE[key]


def _sub(rows, ix):
    return [rows[k] for k in ix]


# ---------------------------------------------------------------------------------------- the plans
# name -> (plan options, what icp4r.plan() must report).  Single-pair plans run the pairs one by one
# through icp4r_align, batch plans as one icp4r_align_batch_* call.
def _opt(ctx, name):
    return ctx.get_plan_option(name)[0]


SINGLE_PLANS = {
    "solo": ({}, lambda pl, c: pl["solo"]),
    "held": ({"solo": 0}, lambda pl, c: not pl["solo"] and not pl["lds"] and pl["wide_update"] and pl["held_update"]),
    "wide": ({"solo": 0, "held_update": 0},
             lambda pl, c: not pl["solo"] and not pl["lds"] and pl["wide_update"] and not pl["held_update"]),
    "fold-single": ({"solo": 0, "wide_update": 0},
                    lambda pl, c: not pl["solo"] and not pl["lds"] and not pl["wide_update"] and pl["pruned"]),
    "multi-tile": ({}, lambda pl, c: not pl["solo"] and not pl["lds"] and pl["pruned"] and pl["wide_update"]
                   and _opt(c, "fold_keys") == 1),
    "multi-tile-corr": ({"fold_keys": 0}, lambda pl, c: not pl["solo"] and not pl["lds"] and pl["pruned"]
                        and pl["wide_update"] and _opt(c, "fold_keys") == 0),
    "brute": ({}, lambda pl, c: not pl["pruned"] and not pl["solo"] and not pl["lds"]),
}
_LDS = lambda pl: pl["lds"] and pl["cache"]  # noqa: E731
BATCH_PLANS = {
    "batch-lazy": ({}, lambda pl, c: _LDS(pl) and pl["lazy_x"] and not pl["res_update"]),
    "batch-eager": ({"lazy_x": 0}, lambda pl, c: _LDS(pl) and not pl["lazy_x"] and not pl["res_update"]
                    and _opt(c, "fuse_test") == 1),
    "batch-unfused": ({"fuse_test": 0}, lambda pl, c: _LDS(pl) and not pl["lazy_x"] and not pl["res_update"]
                      and _opt(c, "fuse_test") == 0),
    "batch-records": ({"nn_cache": 0}, lambda pl, c: pl["lds"] and not pl["cache"] and not pl["res_update"]),
    "batch-res": ({"res_update": 1}, lambda pl, c: _LDS(pl) and pl["res_update"] and not pl["lazy_x"]),
    "batch-sums": ({"sums_tail": 1}, lambda pl, c: _LDS(pl) and not pl["res_update"] and not pl["lazy_x"]
                   and _opt(c, "sums_tail") == 1),
    "small-batch": ({}, lambda pl, c: not pl["lds"] and not pl["solo"] and pl["wide_update"]),
}
# the F64 batch: the LDS plan with the cached-neighbour test in its own kernel (nothing fused, no
# lazy_x, no on-chip update: those are PCL-numerics forms)
F64_PLANS = {
    "batch-f64": ({}, lambda pl, c: _LDS(pl) and not pl["lazy_x"]),
    "small-batch": ({}, lambda pl, c: not pl["lds"] and not pl["solo"] and not pl["wide_update"]),
}
LDS_PLANS = tuple(k for k in BATCH_PLANS if k != "small-batch")
ONE_TILE = ("solo", "held", "wide", "fold-single", "brute")


def _solo_ok(pair):
    return len(pair[0]) <= 1024 and 512 <= len(pair[1]) <= 8192


def _concat(pairs):
    sn = np.array([len(s) for s, _ in pairs], np.int32)
    tn = np.array([len(t) for _, t in pairs], np.int32)
    so = np.concatenate([[0], np.cumsum(sn)[:-1]]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tn)[:-1]]).astype(np.int64)
    src = np.concatenate([np.asarray(s, np.float32).reshape(-1, 4) for s, _ in pairs])
    tgt = np.concatenate([np.asarray(t, np.float32).reshape(-1, 4) for _, t in pairs])
    return src, so, sn, tgt, to, tn


def _guess_cm(guesses):
    """(npairs, 4, 4) row-major guesses -> (npairs, 16) column-major float32, as the C ABI takes them."""
    return np.ascontiguousarray(np.asarray(guesses, np.float32).transpose(0, 2, 1).reshape(len(guesses), 16))


def _run_batch_device(ctx, pairs, params, guesses):
    """icp4r_align_batch_device with Batch.aligned (and Batch.guess) set: rows and aligned clouds."""
    import torch

    import icp4r

    dev = torch.device("cuda", 0)
    src, so, sn, tgt, to, tn = _concat(pairs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    # (one spare point: an all-empty side still has a device buffer)
    t = {"src": up(np.concatenate([src, np.zeros((1, 4), np.float32)])),
         "tgt": up(np.concatenate([tgt, np.zeros((1, 4), np.float32)])),
         "so": up(so), "sn": up(sn), "to": up(to), "tn": up(tn)}
    t["aligned"] = torch.zeros_like(t["src"])
    g = None if guesses is None else up(_guess_cm(guesses))
    b = icp4r.Batch(src=t["src"].data_ptr(), tgt=t["tgt"].data_ptr(), src_off=t["so"].data_ptr(),
                    src_n=t["sn"].data_ptr(), tgt_off=t["to"].data_ptr(), tgt_n=t["tn"].data_ptr(),
                    guess=None if g is None else g.data_ptr(), aligned=t["aligned"].data_ptr(), npairs=len(pairs),
                    max_src_n=int(sn.max()), max_tgt_n=int(tn.max()))
    out = torch.zeros((len(pairs), 96), dtype=torch.uint8, device=dev)
    ctx.align_batch_device(b, params, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    rows = np.frombuffer(out.cpu().numpy().tobytes(), dtype=icp4r.RESULT_DTYPE)
    al = t["aligned"].cpu().numpy()
    return rows, [al[o: o + n].copy() for o, n in zip(so, sn)]


def _run(ctx, plan, name, pairs, kw, guesses=None, entry="device", plans=None):
    """`pairs` through the plan `name` with parameters kw: (result rows, aligned clouds or None).
    Asserts through icp4r.plan() that the plan was taken.  entry = "host": icp4r_align_batch_host (no
    aligned clouds)."""
    import icp4r

    ctx.reset_plan_options()
    table = plans or (SINGLE_PLANS if name in SINGLE_PLANS else BATCH_PLANS)
    options, taken = table[name]
    plan(**options)
    numerics = kw.get("numerics", icp4r.NUMERICS_PCL)
    try:
        if table is SINGLE_PLANS:
            rows = np.zeros(len(pairs), icp4r.RESULT_DTYPE)
            aligned = []
            for k, (s, t) in enumerate(pairs):
                mode = icp4r.NN_BRUTE if name == "brute" and len(t) >= 512 else icp4r.NN_AUTO
                if len(t):  # (an empty target is no plan's: init_kernel marks it and every kernel returns)
                    pl = icp4r.plan(1, len(s), len(t), mode, numerics, ctx=ctx)
                    assert taken(pl, ctx), (name, len(s), len(t), pl)
                    assert (len(t) > 8192) == name.startswith("multi-tile"), (name, len(t))
                r, al = ctx.align(s, t, icp4r.default_params(nn_mode=mode, **kw),
                                  guess=None if guesses is None else guesses[k], want_aligned=True)
                rows[k] = np.frombuffer(bytes(r), icp4r.RESULT_DTYPE)[0]
                aligned.append(al)
            return rows, aligned
        sn = [len(s) for s, _ in pairs]
        tn = [len(t) for _, t in pairs]
        assert (len(pairs) >= 256) == (name != "small-batch")
        pl = icp4r.plan(len(pairs), max(sn), max(tn), icp4r.NN_AUTO, numerics, ctx=ctx)
        assert taken(pl, ctx), (name, pl)
        params = icp4r.default_params(**kw)
        if entry == "host":
            return ctx.align_batch_host(*_concat(pairs), params=params, guess=guesses), None
        return _run_batch_device(ctx, pairs, params, guesses)
    finally:
        ctx.reset_plan_options()


def _bits(x):
    return np.float64(x).tobytes()


def _equal_oracle(rows, aligned, pairs, orows, label):
    """Every row (and aligned cloud) equal to the oracle's, T, fitness and xyz in bits."""
    assert len(rows) == len(pairs) == len(orows), label
    for k, ((s, _), o) in enumerate(zip(pairs, orows)):
        r, w = rows[k], (label, k)
        assert r["status"] == o["status"], w
        assert r["iterations"] == o["iterations"], w + (int(r["iterations"]), o["iterations"])
        assert bool(r["converged"]) == o["converged"], w
        assert r["convergence_state"] == o["convergence_state"], w
        assert r["n_correspondences"] == o["n_correspondences"], w + (int(r["n_correspondences"]), o["n_correspondences"])
        assert r["T"].tobytes() == np.ascontiguousarray(o["T"].T).tobytes(), w + (r["T"].reshape(4, 4).T, o["T"])
        assert _bits(r["fitness"]) == _bits(o["fitness"]), w + (float(r["fitness"]), o["fitness"])
        if aligned is not None:
            a = aligned[k]
            assert a.shape == o["aligned"].shape, w
            assert np.ascontiguousarray(a[:, :3]).tobytes() == np.ascontiguousarray(o["aligned"][:, :3]).tobytes(), w
            copied = o["status"] not in (E_EMPTY, E_NONFINITE) and np.asarray(s).shape[1] > 3
            want = np.asarray(s)[:, 3] if copied else np.zeros(len(a), np.float32)
            assert np.ascontiguousarray(a[:, 3]).tobytes() == np.ascontiguousarray(want).tobytes(), w


def _every_plan(ctx, oracle_mod, plan, tag, pairs, kw, batch_plans=LDS_PLANS, single=SINGLE, small=SMALL,
                single_plans=ONE_TILE):
    """The 260-pair list `pairs` on the batch plans, its `small` pairs as the 5-pair batch, its `single`
    pairs one by one on the single-pair plans (solo_kernel: those it takes): every row equal to the
    oracle and byte-equal across the plans.  Returns the oracle's rows."""
    orows = _oracle(oracle_mod, tag, pairs, kw)
    ref = None
    for name in batch_plans:
        rows, al = _run(ctx, plan, name, pairs, kw)
        _equal_oracle(rows, al, pairs, orows, name)
        if ref is None:
            ref = rows
        assert rows.tobytes() == ref.tobytes(), name
    if small:
        ix = list(small)
        rows, al = _run(ctx, plan, "small-batch", _sub(pairs, ix), kw)
        _equal_oracle(rows, al, _sub(pairs, ix), _sub(orows, ix), "small-batch")
        assert ref is None or rows.tobytes() == ref[ix].tobytes()
    for name in single_plans:
        ix = [k for k in single if name != "solo" or _solo_ok(pairs[k])]
        assert len(ix) >= 4, name
        rows, al = _run(ctx, plan, name, _sub(pairs, ix), kw)
        _equal_oracle(rows, al, _sub(pairs, ix), _sub(orows, ix), name)
        assert ref is None or rows.tobytes() == ref[ix].tobytes(), name
    return orows


def _multi_tile(ctx, oracle_mod, plan, tag, pairs, kw, guesses=None):
    orows = _oracle(oracle_mod, tag, pairs, kw, guesses)
    out = {}
    for name in ("multi-tile", "multi-tile-corr"):
        rows, al = _run(ctx, plan, name, pairs, kw, guesses)
        _equal_oracle(rows, al, pairs, orows, name)
        out[name] = rows.tobytes()
    assert out["multi-tile"] == out["multi-tile-corr"]
    return orows


# ------------------------------------------------------------------- 1. convergence criteria
def _states(rows):
    return {r["convergence_state"] for r in rows}


@pytest.mark.parametrize("name", sorted(SETS))
def test_oracle_reaches_the_criteria(oracle_mod, name):
    """The oracle alone, on the first 48 pairs: each parameter set stops in exactly the states it is
    there for, at 3 or more different iterations within the range noted; with the similar-transforms
    counter (A, C) pairs stop later than without it."""
    pairs = _pairs(FIRST48)
    rows = _oracle(oracle_mod, "first48", pairs, SETS[name])
    states, (lo, hi) = SET_STATES[name]
    assert all(r["status"] == 0 and r["converged"] for r in rows)
    assert _states(rows) == states, name
    its = {r["iterations"] for r in rows}
    assert len(its) >= 3 and lo <= min(its) and max(its) <= hi, (name, sorted(its))
    if name == "F":
        assert any(r["n_correspondences"] < len(s) for r, (s, _) in zip(rows, pairs))
    if name in ("A", "C"):
        plain = _oracle(oracle_mod, "first48", pairs, dict(SETS[name], max_iterations_similar_transforms=0))
        assert any(r["iterations"] > q["iterations"] for r, q in zip(rows, plain)), name


@pytest.mark.parametrize("name", ["A", "C"])
def test_oracle_stops_at_both_parities(oracle_mod, name):
    """A and C capped at 11 and at 12 iterations: in both, pairs stop early after an odd and after an
    even number of updates (lazy_x: in pending and in non-pending ones) and others run to the cap."""
    for cap in (11, 12):
        rows = _oracle(oracle_mod, "first48", _pairs(FIRST48), dict(SETS[name], max_iterations=cap))
        early = {r["iterations"] & 1 for r in rows if r["convergence_state"] != CONV_ITERATIONS}
        assert early == {0, 1}, (name, cap)
        assert any(r["convergence_state"] == CONV_ITERATIONS and r["iterations"] == cap for r in rows), (name, cap)


@gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_criteria_on_every_plan(gpu_ctx, oracle_mod, plan, name):
    """Each set on every plan.  Where a plan's special form does not apply (the on-chip update and
    the sums tail with rejections, the sums tail with an MSE criterion) the option must change
    nothing: the rows are byte-equal across the plans either way."""
    kw = SETS[name]
    orows = _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), kw, batch_plans=LDS_PLANS)
    assert SET_STATES[name][0] <= _states(orows)
    _multi_tile(gpu_ctx, oracle_mod, plan, "mt", [_mt_pair(0), _mt_pair(1)], kw)
    # NN_AUTO takes brute force by itself below 512 targets
    few = [(s, t[:400]) for s, t in _pairs((0, 1, 3))]
    rows, al = _run(gpu_ctx, plan, "brute", few, kw)
    _equal_oracle(rows, al, few, _oracle(oracle_mod, "few-targets", few, kw), "brute (auto)")


@gpu
@pytest.mark.parametrize("name,cap", [("A", 11), ("A", 12), ("C", 11), ("C", 12)])
def test_criteria_both_parities_of_max_iterations(gpu_ctx, oracle_mod, plan, name, cap):
    """lazy_x fixes its silent / storing tails from max_iterations alone: odd and even caps, with pairs
    whose stop the similar-transforms counter delays."""
    kw = dict(SETS[name], max_iterations=cap)
    _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), kw, batch_plans=("batch-lazy", "batch-eager"),
                small=None, single_plans=())


# ------------------------------------------------------------------------- 2. per-pair guesses
def _motion(t=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    G = np.eye(4)
    G[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    G[:3, 3] = t
    return G.astype(np.float32)


GUESSES = (_motion(), _motion(t=(0.3, -0.2, 0.05)), _motion(t=(7.0, -5.0, 1.0), yaw=0.4),
           _motion(yaw=-0.03, pitch=0.01))


def _guesses(n=NPAIRS):
    """Exact identity, a small motion, the far guess and a pure rotation in turn; identity at the
    batch's first and last row and on both sides of the pair-group boundary."""
    g = np.stack([GUESSES[(k + 1) % len(GUESSES)] for k in range(n)])
    for k in EDGES:
        if k < n:
            g[k] = GUESSES[0]
    return g


GUESS_SETS = {"defaults": {}, "A": SETS["A"]}


def test_oracle_guesses_matter(oracle_mod):
    """The oracle alone: the guesses change the registrations (the far guess ends elsewhere), and an
    exact identity guess equals no guess."""
    pairs, g = _pairs(FIRST48), _guesses(48)
    rows = _oracle(oracle_mod, "first48-guess", pairs, {}, g)
    plain = _oracle(oracle_mod, "first48", pairs, {})
    same = [(r["T"] == q["T"]).all() for r, q in zip(rows, plain)]
    ident = [(g[k] == np.eye(4)).all() for k in range(48)]
    assert all(s for s, i in zip(same, ident) if i) and sum(ident) >= 10
    assert sum(not s for s, i in zip(same, ident) if not i) >= 30


@gpu
@pytest.mark.parametrize("name", sorted(GUESS_SETS))
def test_batch_guesses(gpu_ctx, oracle_mod, plan, name):
    """A guess per pair through the device entry (Batch.guess, Batch.aligned) and the host entry: every
    row equal to the oracle with that guess, and to the pair's own icp4r_align call with it."""
    import icp4r

    kw, pairs, g = GUESS_SETS[name], _pairs(ALL), _guesses()
    orows = _oracle(oracle_mod, "all-guess", pairs, kw, g)
    ref = None
    for pname in ("batch-lazy", "batch-eager", "batch-res", "batch-records", "small-batch"):
        ix = list(SMALL) if pname == "small-batch" else list(ALL)
        sub, gs = _sub(pairs, ix), g[ix]
        rows, al = _run(gpu_ctx, plan, pname, sub, kw, gs)
        _equal_oracle(rows, al, sub, _sub(orows, ix), pname)
        host, _ = _run(gpu_ctx, plan, pname, sub, kw, gs, entry="host")
        assert host.tobytes() == rows.tobytes(), pname
        if ref is None:
            ref = rows
        assert rows.tobytes() == ref[ix].tobytes(), pname
    p = icp4r.default_params(**kw)
    for k, (s, t) in enumerate(pairs):
        r, al = gpu_ctx.align(s, t, p, guess=g[k], want_aligned=True)
        assert bytes(r) == ref[k].tobytes(), k
        assert al.tobytes() == orows[k]["aligned"].tobytes(), k


@gpu
@pytest.mark.parametrize("name", sorted(GUESS_SETS))
def test_single_pair_guesses(gpu_ctx, oracle_mod, plan, name):
    """Single pairs with a guess on solo_kernel, the held update and the multi-tile target."""
    kw, g = GUESS_SETS[name], _guesses(len(SINGLE))
    pairs = _pairs(SINGLE)
    orows = _oracle(oracle_mod, "single-guess", pairs, kw, g)
    for pname in ("solo", "held", "brute"):
        ix = [k for k in range(len(pairs)) if pname != "solo" or _solo_ok(pairs[k])]
        rows, al = _run(gpu_ctx, plan, pname, _sub(pairs, ix), kw, g[ix])
        _equal_oracle(rows, al, _sub(pairs, ix), _sub(orows, ix), pname)
    mt = [_mt_pair(0)] * len(GUESSES)
    _multi_tile(gpu_ctx, oracle_mod, plan, "mt-guess", mt, kw, np.stack(GUESSES))


# --------------------------------------------------- 3. failures among healthy pairs, and late ones
def _empty():
    return np.zeros((0, 4), np.float32)


def _replace(pair, kind):
    s, t = pair
    if kind == "empty_tgt":
        return s, _empty()
    if kind == "empty_src":
        return _empty(), t
    if kind == "nan_src":
        s = s.copy()
        s[len(s) // 3, 1] = np.nan
        return s, t
    if kind == "inf_tgt":
        t = t.copy()
        t[len(t) - 1, 0] = np.inf
        return s, t
    assert kind == "two_points"
    return s[:2].copy(), t


# pair index -> what replaces it (the batch's and the pair groups' edges among them)
# (an empty source as the very first pair and as a pair group's first: the kernels clamp a point index
# to n - 1, which must not reach in front of the workspace)
BAD = {0: "empty_src", 1: "empty_tgt", 2: "two_points", 57: "nan_src", 128: "empty_src", 129: "inf_tgt",
       130: "empty_src", 131: "empty_tgt", 200: "two_points", 258: "nan_src", 259: "inf_tgt"}
BAD_SMALL = {0: "empty_src", 2: "empty_tgt", 4: "two_points"}  # positions in the 5-pair batch
EXPECT = {"empty_tgt": (E_EMPTY, 0, 0), "nan_src": (E_NONFINITE, 0, 0), "inf_tgt": (E_NONFINITE, 0, 0),
          "empty_src": (E_TOO_FEW_CORR, CONV_NO_CORR, 0), "two_points": (E_TOO_FEW_CORR, CONV_NO_CORR, 2)}


def _with_bad(pairs, bad):
    return [_replace(p, bad[k]) if k in bad else p for k, p in enumerate(pairs)]


@pytest.mark.parametrize("guess", [False, True])
def test_oracle_rows_of_bad_pairs(oracle_mod, guess):
    """The oracle alone: invalid pairs report identity, DBL_MAX and zero counters whatever the guess;
    an empty or two-point source is PCL's "not enough correspondences" at iteration 0."""
    g = GUESSES[1] if guess else None
    for kind, (status, state, ncorr) in EXPECT.items():
        s, t = _replace(_pair(0), kind)
        o = oracle_mod.align(s, t, guess=g, numerics=oracle_mod.NUM_F32)
        assert (o["status"], o["convergence_state"], o["n_correspondences"]) == (status, state, ncorr), kind
        assert o["iterations"] == 0 and not o["converged"], kind
        if status != E_TOO_FEW_CORR:
            assert (o["T"] == np.eye(4)).all() and o["fitness"] == np.finfo(np.float64).max, kind


@gpu
@pytest.mark.parametrize("guess", [False, True])
def test_bad_pairs_among_healthy_ones(gpu_ctx, oracle_mod, plan, guess):
    """Invalid and too-small pairs inside a batch: their rows are the oracle's, and every other pair's
    row and aligned cloud are byte-equal to the same batch without them (a bad pair must not disturb
    its neighbours' work lists, the group's counters or the fused tails)."""
    healthy = _pairs(ALL)
    g = _guesses() if guess else None
    for pname in BATCH_PLANS:
        small = pname == "small-batch"
        ix = list(SMALL) if small else list(ALL)
        bad = BAD_SMALL if small else BAD
        good = _sub(healthy, ix)
        mixed = _with_bad(good, bad)
        gs = None if g is None else g[ix]
        rows0, al0 = _run(gpu_ctx, plan, pname, good, {}, gs)
        rows, al = _run(gpu_ctx, plan, pname, mixed, {}, gs)
        assert (rows0["status"] == 0).all(), pname
        for k in range(len(ix)):
            if k in bad:
                o = oracle_mod.align(*mixed[k], guess=None if gs is None else gs[k], aligned=True,
                                     numerics=oracle_mod.NUM_F32)
                assert (o["status"], o["convergence_state"], o["n_correspondences"]) == EXPECT[bad[k]]
                _equal_oracle(rows[k: k + 1], al[k: k + 1], mixed[k: k + 1], [o], (pname, bad[k], k))
                if o["status"] != E_TOO_FEW_CORR:
                    assert rows[k]["T"].tobytes() == np.eye(4, dtype=np.float32).tobytes(), (pname, k)
                    assert rows[k]["fitness"] == np.finfo(np.float64).max and rows[k]["iterations"] == 0
            else:
                assert rows[k].tobytes() == rows0[k].tobytes(), (pname, k)
                assert al[k].tobytes() == al0[k].tobytes(), (pname, k)


def _few_targets():
    s, t = _pair(0)
    return s, t[:400]


# plan -> the healthy pair each bad pair is made from (brute: NN_AUTO's choice below 512 targets)
BAD_SINGLE = {"solo": lambda: _pair(0), "held": lambda: _pair(0), "wide": lambda: _pair(0),
              "fold-single": lambda: _pair(0), "brute": _few_targets, "multi-tile": lambda: _mt_pair(0),
              "multi-tile-corr": lambda: _mt_pair(0)}


@gpu
@pytest.mark.parametrize("guess", [False, True])
def test_bad_single_pairs(gpu_ctx, oracle_mod, plan, guess):
    """The same bad pairs as single calls on every single-pair plan (the held update with the records,
    with the merged keys of a multi-tile target, and behind brute force), each after a healthy call
    with as many source points, whose aligned cloud the context's device buffer still holds: rows equal
    to the oracle, and the aligned output of a pair for which nothing was computed untouched.  An
    empty source is pair 0 of its launch: a point index clamped to n - 1 must not be followed."""
    for pname, make in BAD_SINGLE.items():
        good = make()
        pairs, kinds = [], []
        for kind in EXPECT:
            pairs += [good, _replace(good, kind)]
            kinds += [None, kind]
        gs = np.stack([GUESSES[1]] * len(pairs)) if guess else None
        rows, al = _run(gpu_ctx, plan, pname, pairs, {}, gs)
        orows = [oracle_mod.align(s, t, guess=None if gs is None else gs[k], numerics=oracle_mod.NUM_F32, aligned=True)
                 for k, (s, t) in enumerate(pairs)]
        _equal_oracle(rows, al, pairs, orows, pname)
        for o, kind in zip(orows, kinds):
            assert o["status"] == (0 if kind is None else EXPECT[kind][0]), (pname, kind)


@gpu
def test_facade_output_of_an_invalid_pair(gpu_ctx):
    """IterativeClosestPoint.align after a healthy registration: with a NaN in the source or an empty
    target nothing is computed, the transformation is the identity and the output is the input."""
    import icp4r

    s, t = _pair(0)
    icp = icp4r.IterativeClosestPoint(gpu_ctx)
    icp.setInputSource(s)
    icp.setInputTarget(t)
    moved = icp.align()
    assert icp.hasConverged() and (moved[:, :3] != s[:, :3]).any()
    for bad_s, bad_t in (_replace((s, t), "nan_src"), _replace((s, t), "empty_tgt")):
        icp.setInputSource(bad_s)
        icp.setInputTarget(bad_t)
        out = icp.align()
        assert not icp.hasConverged() and (icp.getFinalTransformation() == np.eye(4)).all()
        assert out.tobytes() == np.ascontiguousarray(bad_s, np.float32).tobytes()


def _late_failure(oracle_mod, pair, dist, iters=12):
    """From the oracle's trace: (j, min_correspondences) such that the pair fails at the first
    iteration j >= 1 whose |C| falls below every earlier one; None if |C| never does."""
    nc = oracle_mod.align(*pair, numerics=oracle_mod.NUM_F32, trace=True, max_correspondence_distance=dist,
                          max_iterations=iters)["trace"]["ncorr"]
    for j in range(1, len(nc)):
        if nc[j] < nc[:j].min():
            return j, int(nc[:j].min())
    return None


LATE = dict(pair=8, dist=2.0)       # the 700 x 650 pair seeded 4008: |C| 577 -> 575
LATE_MT = dict(pair=1, dist=1.0)    # the 700 x 9000 pair seeded 4301: |C| 279, 279, 278


def _late_kw(oracle_mod, iters=12):
    j, mc = _late_failure(oracle_mod, _pair(LATE["pair"]), LATE["dist"])
    return dict(max_correspondence_distance=LATE["dist"], min_correspondences=mc, max_iterations=iters)


def _failed_late(r):
    return r["status"] == E_TOO_FEW_CORR and r["iterations"] >= 1


def test_oracle_fails_after_iterating(oracle_mod):
    """The oracle alone: with the derived min_correspondences the batch holds a pair that fails after
    it has iterated (non-identity T, the failing count, a fitness), pairs that fail at iteration 0 and
    pairs that finish; the single-pair list and the 5-pair batch contain the late one; the multi-tile
    pair has a late failure of its own."""
    kw = _late_kw(oracle_mod)
    rows = _oracle(oracle_mod, "first48", _pairs(FIRST48), kw)
    late = [k for k, r in enumerate(rows) if _failed_late(r)]
    assert LATE["pair"] in late and LATE["pair"] in SINGLE and LATE["pair"] in SMALL
    assert any(r["status"] == E_TOO_FEW_CORR and r["iterations"] == 0 for r in rows)
    assert any(r["status"] == 0 for r in rows)
    r = rows[LATE["pair"]]
    assert r["convergence_state"] == CONV_NO_CORR and not r["converged"]
    assert not (r["T"] == np.eye(4)).all() and r["n_correspondences"] < kw["min_correspondences"]
    assert r["fitness"] < np.finfo(np.float64).max
    assert (r["aligned"][:, :3] != _pair(LATE["pair"])[0][:, :3]).any()
    for cap in (11, 12):  # (the failure iteration is the same under both caps)
        assert _failed_late(_oracle(oracle_mod, "first48", _pairs(FIRST48), _late_kw(oracle_mod, cap))[LATE["pair"]])
    assert _late_failure(oracle_mod, _mt_pair(LATE_MT["pair"]), LATE_MT["dist"]) is not None


@gpu
def test_failure_after_iterating(gpu_ctx, oracle_mod, plan):
    """|C| < min_correspondences at iteration >= 1: the row keeps the product of the transforms so far,
    the iterations done and the failing count, and the fitness pass and the aligned cloud use that T
    (a deferred transform included), on every plan, both parities of max_iterations on lazy_x."""
    kw = _late_kw(oracle_mod)
    orows = _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), kw, batch_plans=LDS_PLANS)
    assert sum(_failed_late(r) for r in orows) >= 1
    _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), _late_kw(oracle_mod, 11),
                batch_plans=("batch-lazy", "batch-eager"), small=None, single_plans=())
    j, mc = _late_failure(oracle_mod, _mt_pair(LATE_MT["pair"]), LATE_MT["dist"])
    mt = dict(max_correspondence_distance=LATE_MT["dist"], min_correspondences=mc, max_iterations=12)
    orows = _multi_tile(gpu_ctx, oracle_mod, plan, "mt", [_mt_pair(0), _mt_pair(1)], mt)
    assert _failed_late(orows[LATE_MT["pair"]]) and orows[LATE_MT["pair"]]["iterations"] == j


ABOVE_N = dict(min_correspondences=1000)


def test_oracle_min_correspondences_above_n(oracle_mod):
    rows = _oracle(oracle_mod, "first48", _pairs(FIRST48), ABOVE_N)
    for r, (s, _) in zip(rows, _pairs(FIRST48)):
        assert (r["status"] == E_TOO_FEW_CORR and r["iterations"] == 0) == (len(s) < 1000)
        assert r["status"] != E_TOO_FEW_CORR or r["n_correspondences"] == len(s)
    assert {r["status"] for r in rows} == {0, E_TOO_FEW_CORR}


@gpu
def test_min_correspondences_above_n(gpu_ctx, oracle_mod, plan):
    """min_correspondences above some pairs' size, no threshold: the failure at iteration 0 on every
    plan, the on-chip update (which a threshold would turn off) included."""
    _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), ABOVE_N, batch_plans=LDS_PLANS)
    _multi_tile(gpu_ctx, oracle_mod, plan, "mt", [_mt_pair(0), _mt_pair(1)], ABOVE_N)


# ------------------------------------------------------- 4. overflowing and huge coordinates
def _overflow(pair, variant):
    """12 source points at 3e19 (one at (-3e19, 2e19, 0)) and / or every 97th target at -3e19: their
    squared distances to anything finite are +inf in float."""
    s, t = pair[0].copy(), pair[1].copy()
    if variant in ("src", "both"):
        s[5:5 + 64 * 11:64, :3] = 3e19
        s[6, :3] = (-3e19, 2e19, 0.0)
    if variant in ("tgt", "both"):
        t[3::97, :3] = -3e19
    return s, t


VARIANTS = ("src", "tgt", "both")
OVERFLOW_AT = {0: "src", 3: "both", 4: "tgt", 5: "tgt", 8: "both", 14: "src", 77: "src", 129: "both", 130: "src",
               131: "tgt", 259: "both"}
OVERFLOW_SETS = {"defaults": {}, "fixed": dict(max_iterations=8, **FIXED), "huber": dict(huber_delta=0.5),
                 "threshold": dict(max_correspondence_distance=1.0)}


@functools.lru_cache(maxsize=None)
def _overflow_pair(variant):
    from icp4r import synth

    p = synth.make_pair(4100, 700, 650)
    return _overflow((p.src_xyzi(), p.tgt_xyzi()), variant)


@functools.lru_cache(maxsize=None)
def _overflow_batch():
    """The batch with the variants planted in a few pairs (every pair of the 5-pair batch, held-update
    shapes of the single-pair list), and the three variants of the 700 x 650 pair seeded 4100 in places
    of the single-pair list."""
    pairs = [_overflow(p, OVERFLOW_AT[k]) if k in OVERFLOW_AT else p for k, p in enumerate(_pairs(ALL))]
    for k, v in zip((1, 2, 6), VARIANTS):
        pairs[k] = _overflow_pair(v)
    return pairs


def test_oracle_registers_overflowing_clouds(oracle_mod):
    """The oracle alone: the clouds register (PCL rejects a correspondence whose d2 overflows even at
    the default threshold: 688 of 700 kept), with finite T, aligned cloud and fitness."""
    for v in VARIANTS:
        s, t = _overflow_pair(v)
        for kw in OVERFLOW_SETS.values():
            o = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, aligned=True, **kw)
            assert o["status"] == 0 and o["converged"], (v, kw)
            assert np.isfinite(o["T"]).all() and np.isfinite(o["aligned"]).all() and 1.0 < o["fitness"] < 10.0
            if "max_correspondence_distance" not in kw:
                assert o["n_correspondences"] == (700 if v == "tgt" else 688), (v, kw)
        _, d2 = oracle_mod.nearest(s, t)
        assert np.isinf(d2).sum() == (0 if v == "tgt" else 12)


@gpu
@pytest.mark.parametrize("name", sorted(OVERFLOW_SETS))
def test_overflowing_coordinates_on_every_plan(gpu_ctx, oracle_mod, plan, name):
    """Every plan, the on-chip update's "only an overflowing d2 is rejected" branch and the sums
    tail's sums_ok = -1 path among them."""
    kw = OVERFLOW_SETS[name]
    pairs = _overflow_batch()
    orows = _every_plan(gpu_ctx, oracle_mod, plan, "overflow", pairs, kw, batch_plans=LDS_PLANS)
    if "max_correspondence_distance" not in kw:
        assert sum(r["n_correspondences"] < len(s) for r, (s, _) in zip(orows, pairs)) >= 7
    mt = [_overflow(_mt_pair(0), v) for v in VARIANTS]
    _multi_tile(gpu_ctx, oracle_mod, plan, "mt-overflow", mt, kw)


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_overflowing_coordinates_nearest_and_fitness(gpu_ctx, oracle_mod, variant):
    """icp4r_nearest: d2 bits equal everywhere, the index wherever d2 is finite (the oracle reports -1
    for an overflowing d2: there any valid index); icp4r_fitness without and with a range."""
    for s, t in (_overflow_pair(variant), _overflow(_mt_pair(0), variant)):
        gi, gd = gpu_ctx.nearest(s, t)
        oi, od = oracle_mod.nearest(s, t, oracle_mod.NN_BRUTE)
        assert gd.tobytes() == od.tobytes()
        fin = np.isfinite(od)
        assert (gi[fin] == oi[fin]).all() and (oi[~fin] == -1).all()
        assert ((gi[~fin] >= 0) & (gi[~fin] < len(t))).all()
        assert (~fin).sum() == (0 if variant == "tgt" else 12)
        for T in (GUESSES[0], GUESSES[1]):
            for mr in (np.finfo(np.float64).max, 0.5):
                assert _bits(gpu_ctx.fitness(s, t, T, mr)) == _bits(oracle_mod.fitness(s, t, T, mr)), (mr,)


HUGE = dict(max_iterations=8, **FIXED)


def _huge(pair):
    s = pair[0].copy()
    s[11, :3] = (2e17, 0.0, 0.0)
    return s, pair[1]


def test_oracle_huge_coordinate(oracle_mod):
    """One source point at 2e17: flagged big on the device, but no d2 overflows (4e34 < FLT_MAX);
    the registration is numerically wild and still finite."""
    o = oracle_mod.align(*_huge(_overflow_pair("none")), numerics=oracle_mod.NUM_F32, **HUGE)
    assert o["status"] == 0 and o["n_correspondences"] == 700 and o["iterations"] == 8
    assert np.isfinite(o["T"]).all() and 1e30 < o["fitness"] < 1e33


@gpu
def test_huge_coordinate(gpu_ctx, oracle_mod, plan):
    """Fixed iterations on the held update and the sums tail (the pair never skips pass A's distance
    check): every fold is sequential in both implementations, so the bits still agree."""
    one = [_huge(_overflow_pair("none"))]
    rows, al = _run(gpu_ctx, plan, "held", one, HUGE)
    _equal_oracle(rows, al, one, _oracle(oracle_mod, "huge-one", one, HUGE), "held")
    pairs = [_huge(p) if k in (0, 64, 129, 130, 259) else p for k, p in enumerate(_pairs(ALL))]
    orows = _oracle(oracle_mod, "huge", pairs, HUGE)
    ref = None
    for name in ("batch-sums", "batch-lazy", "batch-res"):
        rows, al = _run(gpu_ctx, plan, name, pairs, HUGE)
        _equal_oracle(rows, al, pairs, orows, name)
        ref = rows if ref is None else ref
        assert rows.tobytes() == ref.tobytes(), name


# --------------------------------------------------------------------------------- 5. strides
def _strided(a, cols):
    """The cloud as an (N, cols) array: 3 drops the intensity, 5 and 8 add NaN columns (never read)."""
    out = np.full((len(a), cols), np.nan, np.float32)
    out[:, :min(cols, 4)] = a[:, :min(cols, 4)]
    return out


@gpu
def test_point_strides(gpu_ctx, oracle_mod):
    """12-, 16-, 20- and 32-byte points through align, nearest and fitness: byte-equal results across
    the strides and equal to the oracle; the aligned intensity is 0 for a 12-byte source."""
    import icp4r

    s4, t4 = _pair(3)
    T = GUESSES[1]
    ref = None
    for sc in (3, 4, 5, 8):
        for tc in (3, 4, 5, 8):
            if sc != 4 and tc != 4 and sc != tc:
                continue
            s, t = _strided(s4, sc), _strided(t4, tc)
            r, al = gpu_ctx.align(s, t, icp4r.default_params(), guess=T, want_aligned=True)
            o = oracle_mod.align(s, t, guess=T, numerics=oracle_mod.NUM_F32, aligned=True)
            row = np.frombuffer(bytes(r), icp4r.RESULT_DTYPE)
            _equal_oracle(row, [al], [(s, t)], [o], (sc, tc))
            assert (al[:, 3] == (0.0 if sc == 3 else s4[:, 3])).all(), (sc, tc)
            gi, gd = gpu_ctx.nearest(s, t)
            oi, od = oracle_mod.nearest(s, t, oracle_mod.NN_BRUTE)
            assert (gi == oi).all() and gd.tobytes() == od.tobytes(), (sc, tc)
            f = [gpu_ctx.fitness(s, t, T, mr) for mr in (np.finfo(np.float64).max, 0.5)]
            assert f == [oracle_mod.fitness(s, t, T, mr) for mr in (np.finfo(np.float64).max, 0.5)], (sc, tc)
            got = (row.tobytes(), al[:, :3].tobytes(), gi.tobytes(), gd.tobytes(), f)
            ref = got if ref is None else ref
            assert got == ref, (sc, tc)


@gpu
def test_output_strides(gpu_ctx, oracle_mod):
    """icp4r_align's out_stride_bytes: 32 writes x, y, z and the intensity and leaves a point's other
    four floats alone; 12 writes no intensity (nothing past a point's three floats)."""
    import icp4r

    s, t = _strided(_pair(3)[0], 5), _strided(_pair(3)[1], 8)
    o = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, aligned=True)
    n = len(s)
    L = icp4r.load()

    def call(out, stride):
        r, p = icp4r.Result(), icp4r.default_params()
        rc = L.icp4r_align(gpu_ctx.handle, s.ctypes.data, n, 20, t.ctypes.data, len(t), 32, None, C.byref(p),
                           C.byref(r), out.ctypes.data, stride)
        assert rc == 0 and r.matrix().tobytes() == o["T"].tobytes()

    wide = np.full((n, 8), np.nan, np.float32)
    call(wide, 32)
    assert wide[:, :4].tobytes() == o["aligned"].tobytes() and (wide[:, 3] == s[:, 3]).all()
    assert np.isnan(wide[:, 4:]).all()
    tight = np.full(3 * n + 8, np.nan, np.float32)
    call(tight, 12)
    assert tight[:3 * n].tobytes() == np.ascontiguousarray(o["aligned"][:, :3]).tobytes()
    assert np.isnan(tight[3 * n:]).all()


# --------------------------------------------------------------- 6. F64 numerics in a batch
@gpu
@pytest.mark.parametrize("huber", [False, True])
def test_f64_batch_vs_oracle_f64(gpu_ctx, oracle_mod, plan, huber):
    """NUMERICS_F64 in the batched LDS plan and the 5-pair batch against the F64 oracle, every pair,
    with the bars of test_icp_f64_numerics_vs_oracle_f64: pose within 2e-6 m / rad, fitness within
    1e-6 relative, equal iteration and correspondence counts."""
    import icp4r

    kw = dict(max_iterations=12, **FIXED, **({"huber_delta": 0.5} if huber else {}))
    pairs = _pairs(ALL)
    orows = _oracle(oracle_mod, "all", pairs, dict(kw, numerics=oracle_mod.NUM_F64))
    for name in F64_PLANS:
        ix = list(SMALL) if name == "small-batch" else list(ALL)
        rows, _ = _run(gpu_ctx, plan, name, _sub(pairs, ix), dict(kw, numerics=icp4r.NUMERICS_F64), plans=F64_PLANS)
        worst = [0.0, 0.0, 0.0]
        for r, o in zip(rows, _sub(orows, ix)):
            assert r["status"] == o["status"] == 0
            assert r["iterations"] == o["iterations"] == 12 and r["n_correspondences"] == o["n_correspondences"]
            dt, dr = pose_err(r["T"].reshape(4, 4).T, o["T"])
            worst = [max(a, b) for a, b in zip(worst, (dt, dr, abs(r["fitness"] - o["fitness"]) / o["fitness"]))]
        print(f"{name}: worst dt {worst[0]:.3e} m, dr {worst[1]:.3e} rad, fitness {worst[2]:.3e} relative")
        assert worst[0] <= 2e-6 and worst[1] <= 2e-6 and worst[2] <= 1e-6, (name, worst)
