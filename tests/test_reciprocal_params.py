"""Reciprocal correspondences (use_reciprocal_correspondences = 1) against the C oracle over the parameter
and input space of tests/test_icp_params.py, on every plan a reciprocal registration can take.

The oracle implements the flag (oracle_params.use_reciprocal_correspondences: PCL 1.8.1's
determineReciprocalCorrespondences stated directly; tests/test_reciprocal.py holds it bit-equal to the numpy
twin), so the matrix of test_icp_params.py runs again with the flag on, with that module's inputs and
its meaning of "equal to the oracle": status, iterations, converged, convergence_state and
n_correspondences equal, T and fitness equal in bits, the aligned xyz equal in bits and the intensity
copied through, for EVERY pair of every batch, and the rows byte-equal across the plans.  Only the
F64 sections have a tolerance: the bars of test_icp_params.test_f64_batch_vs_oracle_f64.

The plans (make_plan(..., reciprocal = true) and run_pairs: no solo_kernel, no cached-neighbour test,
no held update, no fold_keys):

  single pairs   wide (one tile, fold_update_wide_kernel, the transform deferred into the search),
                 wide-eager (tile_defer = 0), fold-single (wide_update = 0: the 256-thread update),
                 streamed (nn_tile = 0: the streamed pruned search), brute (NN_BRUTE: the records come
                 from corr_kernel after the stage's marks), two-tile (a 700 x 9000 pair) with
                 fuse_seed 1 and 0
  batches        lds-2groups (260 pairs: more pairs than CUs, fold_update_kernel without its fused
                 tail), lds-wide (the first 256 pairs: at most one pair per CU, the wide update),
                 lds-1group (groups = 1), lds-3groups (groups = 3 on 390 pairs: the 260 and their first
                 130 again — run_pairs lowers `groups` below 384 pairs), tiled (260 pairs, nn_lds = 0),
                 small (a 5-pair batch)

icp4r.plan() describes the flag-off plan: `_run` asserts from it only what the flag does not change
(pruned, lds, the tile count); test_stage_launch_counts asserts per plan name, from the per-kernel
events, that the reciprocal stage was launched groups x max(max_iterations, 1) times and the
cached-neighbour test never (it is the only test that turns kernel timing on).

Every GPU test has an oracle-only twin without the gpu marker, which asserts that the inputs still
reach the states the GPU test is about.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import pose_err
from test_icp_params import (ABOVE_N, ALL, BAD, BAD_SMALL, CONV_ABS_MSE, CONV_ITERATIONS, CONV_NO_CORR, CONV_REL_MSE,
                             CONV_TRANSFORM, E_TOO_FEW_CORR, EXPECT, FIRST48, FIXED, GUESSES, HUGE, OVERFLOW_AT,
                             OVERFLOW_SETS, SETS, SINGLE, VARIANTS, _bits, _concat, _equal_oracle, _failed_late, _guesses,
                             _huge, _mt_pair, _oracle, _overflow, _overflow_batch, _overflow_pair, _pair, _pairs,
                             _replace, _run_batch_device, _states, _strided, _sub, _with_bad)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icp-4dradar_amd", "icp4r", "_lib")

RECIP = dict(use_reciprocal_correspondences=1)


def _on(kw=None, **more):
    return dict(kw or {}, **RECIP, **more)


# pair 69 (900 x 2048, seeded 4069) is this module's late failure: with the flag on and no threshold
# its |C| falls below every earlier count at iteration 2 (test_oracle_fails_after_iterating)
LATE = 69
LATE_MT = dict(pair=1, dist=1.0)                 # the 700 x 9000 pair seeded 4301, at distance 1.0
R_SINGLE = SINGLE + (LATE,)                      # the pairs run one by one on the single-pair plans
R_SMALL = (0, 3, 4, 8, LATE)                     # the 5-pair batch

# ---------------------------------------------------------------------------------------- the plans
SINGLE_PLANS = {"wide": {}, "wide-eager": {"tile_defer": 0}, "fold-single": {"wide_update": 0},
                "streamed": {"nn_tile": 0}, "brute": {}, "two-tile": {}, "two-tile-noseed": {"fuse_seed": 0}}
ONE_TILE = ("wide", "wide-eager", "fold-single", "streamed", "brute")
TWO_TILE = ("two-tile", "two-tile-noseed")
# name -> (plan options, the pairs of the 260-pair list it runs, its pair groups)
BATCH_PLANS = {
    "lds-2groups": ({}, list(ALL), 2),
    "lds-wide": ({}, list(range(256)), 2),
    "lds-1group": ({"groups": 1}, list(ALL), 1),
    "lds-3groups": ({"groups": 3}, list(ALL) + list(range(130)), 3),
    "tiled": ({"nn_lds": 0}, list(ALL), 1),
    "small": ({}, list(R_SMALL), 1),
}
BIG = tuple(k for k in BATCH_PLANS if k != "small")


def _single_mode(name, t):
    import icp4r

    return icp4r.NN_BRUTE if name == "brute" and len(t) >= 512 else icp4r.NN_AUTO


def _run_single(ctx, plan, name, pairs, kw, guesses=None):
    """`pairs` one by one through icp4r_align on the single-pair plan `name`: (rows, aligned clouds)."""
    import icp4r

    ctx.reset_plan_options()
    plan(**SINGLE_PLANS[name])
    try:
        rows = np.zeros(len(pairs), icp4r.RESULT_DTYPE)
        aligned = []
        for k, (s, t) in enumerate(pairs):
            mode = _single_mode(name, t)
            if len(t):
                pl = icp4r.plan(1, len(s), len(t), mode, kw.get("numerics", icp4r.NUMERICS_PCL), ctx=ctx)
                assert pl["pruned"] == (name != "brute" and len(t) >= 512), (name, pl)
                assert not pl["lds"], (name, pl)
                assert (len(t) > 8192) == (name in TWO_TILE), (name, len(t))
            r, al = ctx.align(s, t, icp4r.default_params(nn_mode=mode, **kw),
                              guess=None if guesses is None else guesses[k], want_aligned=True)
            rows[k] = np.frombuffer(bytes(r), icp4r.RESULT_DTYPE)[0]
            aligned.append(al)
        return rows, aligned
    finally:
        ctx.reset_plan_options()


def _run_batch(ctx, plan, name, pairs, kw, guesses=None, entry="device", ix=None):
    """The pairs BATCH_PLANS[name] selects from the 260-pair list `pairs` (ix: other indices) as one
    batch: (rows, aligned clouds or None, the indices).  guesses: per pair of the 260-pair list."""
    import icp4r

    options, sel, _ = BATCH_PLANS[name]
    ix = list(sel if ix is None else ix)
    sub = _sub(pairs, ix)
    gs = None if guesses is None else np.ascontiguousarray(np.asarray(guesses)[ix])
    ctx.reset_plan_options()
    plan(**options)
    try:
        sn = [len(s) for s, _ in sub]
        tn = [len(t) for _, t in sub]
        assert (len(sub) >= 256) == (name != "small"), name
        pl = icp4r.plan(len(sub), max(sn), max(tn), icp4r.NN_AUTO, kw.get("numerics", icp4r.NUMERICS_PCL), ctx=ctx)
        assert pl["pruned"] and pl["lds"] == name.startswith("lds") and max(tn) <= 8192, (name, pl)
        params = icp4r.default_params(**kw)
        if entry == "host":
            return ctx.align_batch_host(*_concat(sub), params=params, guess=gs), None, ix
        rows, al = _run_batch_device(ctx, sub, params, gs)
        return rows, al, ix
    finally:
        ctx.reset_plan_options()


def _every_plan(ctx, oracle_mod, plan, tag, pairs, kw, batch_plans=BIG, small=True, single=R_SINGLE,
                single_plans=ONE_TILE):
    """The 260-pair list on the batch plans, its R_SMALL pairs as the 5-pair batch, its `single` pairs
    one by one on the single-pair plans: every row equal to the oracle (flag on) and byte-equal across
    the plans.  Returns the oracle's rows."""
    assert kw["use_reciprocal_correspondences"] == 1
    orows = _oracle(oracle_mod, tag, pairs, kw)
    ref = None
    for name in tuple(batch_plans) + (("small",) if small else ()):
        rows, al, ix = _run_batch(ctx, plan, name, pairs, kw)
        _equal_oracle(rows, al, _sub(pairs, ix), _sub(orows, ix), name)
        if ref is None:
            assert ix == list(ALL)
            ref = rows
        assert rows.tobytes() == ref[ix].tobytes(), name
    for name in single_plans:
        ix = list(single)
        rows, al = _run_single(ctx, plan, name, _sub(pairs, ix), kw)
        _equal_oracle(rows, al, _sub(pairs, ix), _sub(orows, ix), name)
        assert ref is None or rows.tobytes() == ref[ix].tobytes(), name
    return orows


def _two_tile(ctx, oracle_mod, plan, tag, pairs, kw, guesses=None):
    orows = _oracle(oracle_mod, tag, pairs, kw, guesses)
    out = []
    for name in TWO_TILE:
        rows, al = _run_single(ctx, plan, name, pairs, kw, guesses)
        _equal_oracle(rows, al, pairs, orows, name)
        out.append(rows.tobytes())
    assert out[0] == out[1]
    return orows


# ------------------------------------------------------------- 0. the plans really run: launch counts
@gpu
@pytest.mark.parametrize("name", sorted(SINGLE_PLANS) + sorted(BATCH_PLANS))
def test_stage_launch_counts(gpu_ctx, oracle_mod, plan, name):
    """Per plan name, from the per-kernel events: the reciprocal stage is launched once per pair group
    and iteration (groups x max(max_iterations, 1); every iteration is enqueued, converged or not) and
    the cached-neighbour test never.  This is what shows that 390 pairs ran as three groups and 260 as
    two; the rows of the timed runs equal the oracle's."""
    import icp4r

    for iters in (3, 0):
        kw = _on(FIXED, max_iterations=iters)
        gpu_ctx.set_kernel_timing(True)
        try:
            gpu_ctx.reset_timers()
            if name in SINGLE_PLANS:
                pairs = [_mt_pair(0)] if name in TWO_TILE else _pairs((0, 3))
                rows, al = _run_single(gpu_ctx, plan, name, pairs, kw)
                orows = _oracle(oracle_mod, "timed-" + ("mt" if name in TWO_TILE else "single"), pairs, kw)
                launches = len(pairs) * max(iters, 1)
            else:
                rows, al, ix = _run_batch(gpu_ctx, plan, name, _pairs(ALL), kw)
                pairs, orows = _sub(_pairs(ALL), ix), _sub(_oracle(oracle_mod, "all", _pairs(ALL), kw), ix)
                launches = BATCH_PLANS[name][2] * max(iters, 1)
            gpu_ctx.synchronize()
            assert gpu_ctx.stage_time_ms(icp4r.STAGE_RECIPROCAL)[1] == launches, (name, iters)
            assert gpu_ctx.stage_time_ms(icp4r.STAGE_NN_TEST)[1] == 0, (name, iters)
            assert gpu_ctx.stage_time_ms(icp4r.STAGE_UPDATE)[1] == launches, (name, iters)
        finally:
            gpu_ctx.set_kernel_timing(False)
            gpu_ctx.reset_timers()
        _equal_oracle(rows, al, pairs, orows, (name, iters))
        assert all(r["iterations"] == max(iters, 1) for r in orows)


# ------------------------------------------------------------------- 1. convergence criteria
# the states each set reaches with the flag on, on FIRST48, and the range of its stop iterations
R_STATES = {
    "A": ({CONV_TRANSFORM}, (5, 13)), "B": ({CONV_TRANSFORM, CONV_REL_MSE}, (3, 11)), "C": ({CONV_ABS_MSE}, (7, 14)),
    "D": ({CONV_ITERATIONS, CONV_TRANSFORM, CONV_ABS_MSE, CONV_REL_MSE}, (4, 12)),
    "E": ({CONV_ITERATIONS, CONV_TRANSFORM}, (2, 30)),
    "F": ({CONV_ITERATIONS, CONV_TRANSFORM, CONV_REL_MSE}, (4, 12)),
}
PARITY_SETS = ("A", "C")


@pytest.mark.parametrize("name", sorted(SETS))
def test_oracle_reaches_the_criteria(oracle_mod, name):
    """The oracle alone, flag on, on the first 48 pairs: each set stops in exactly the states noted, at
    8 or more different iterations within the range noted; 27 to 39 rows stop elsewhere than with the
    flag off; the flag rejects something for every pair (without a threshold it keeps 0.50 to 0.90 of
    the sources, to two decimals: 0.5000 to 0.9011)."""
    pairs = _pairs(FIRST48)
    rows = _oracle(oracle_mod, "first48", pairs, _on(SETS[name]))
    off = _oracle(oracle_mod, "first48", pairs, SETS[name])
    states, (lo, hi) = R_STATES[name]
    assert all(r["status"] == 0 and r["converged"] for r in rows)
    assert _states(rows) == states, name
    its = {r["iterations"] for r in rows}
    assert len(its) >= 8 and lo == min(its) and max(its) == hi, (name, sorted(its))
    moved = sum((r["iterations"], r["convergence_state"]) != (q["iterations"], q["convergence_state"])
                for r, q in zip(rows, off))
    assert 27 <= moved <= 39, (name, moved)
    assert all(r["n_correspondences"] < len(s) for r, (s, _) in zip(rows, pairs))
    if "max_correspondence_distance" not in SETS[name]:
        share = [r["n_correspondences"] / len(s) for r, (s, _) in zip(rows, pairs)]
        assert 0.50 <= round(min(share), 2) and round(max(share), 2) <= 0.90, (name, min(share), max(share))


@pytest.mark.parametrize("name", PARITY_SETS)
def test_oracle_stops_at_both_parities(oracle_mod, name):
    """A and C capped at 11 and at 12 iterations, flag on: pairs stop early after an odd and after an
    even number of iterations (the stage's two winner buffers alternate by iteration parity, and a pair
    that has stopped leaves the one it used uncleared) and others run to the cap."""
    for cap in (11, 12):
        rows = _oracle(oracle_mod, "first48", _pairs(FIRST48), _on(SETS[name], max_iterations=cap))
        early = {r["iterations"] & 1 for r in rows if r["convergence_state"] != CONV_ITERATIONS}
        assert early == {0, 1}, (name, cap)
        assert any(r["convergence_state"] == CONV_ITERATIONS and r["iterations"] == cap for r in rows), (name, cap)


@gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_criteria_on_every_plan(gpu_ctx, oracle_mod, plan, name):
    """Each set on every plan: a batch whose pairs stop at different iterations (the stage returns early
    for a pair that is no longer active, beside pairs that go on)."""
    kw = _on(SETS[name])
    orows = _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), kw)
    assert R_STATES[name][0] <= _states(orows)
    assert len({r["iterations"] for r in orows}) >= 8
    _two_tile(gpu_ctx, oracle_mod, plan, "mt", [_mt_pair(0), _mt_pair(1)], kw)


@gpu
@pytest.mark.parametrize("name,cap", [(n, c) for n in PARITY_SETS for c in (11, 12)])
def test_criteria_both_parities_of_max_iterations(gpu_ctx, oracle_mod, plan, name, cap):
    kw = _on(SETS[name], max_iterations=cap)
    _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), kw, batch_plans=("lds-2groups", "lds-3groups", "tiled"),
                single_plans=("wide", "brute"))
    _two_tile(gpu_ctx, oracle_mod, plan, "mt", [_mt_pair(0), _mt_pair(1)], kw)


# ------------------------------------------------------------------------- 2. per-pair guesses
GUESS_SETS = {"defaults": _on(), "A": _on(SETS["A"])}


def test_oracle_guesses_matter(oracle_mod):
    """The oracle alone, flag on: with the guesses all 48 rows finish with status 0, an exact identity
    guess equals no guess, and the other guesses change the registrations."""
    pairs, g = _pairs(FIRST48), _guesses(48)
    rows = _oracle(oracle_mod, "first48-guess", pairs, _on(), g)
    plain = _oracle(oracle_mod, "first48", pairs, _on())
    assert all(r["status"] == 0 for r in rows) and all(r["status"] == 0 for r in plain)
    assert all(r["status"] == 0 for r in _oracle(oracle_mod, "first48-guess", pairs, GUESS_SETS["A"], g))
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
    for pname in ("lds-2groups", "lds-wide", "lds-3groups", "tiled", "small"):
        rows, al, ix = _run_batch(gpu_ctx, plan, pname, pairs, kw, g)
        _equal_oracle(rows, al, _sub(pairs, ix), _sub(orows, ix), pname)
        host, _, _ = _run_batch(gpu_ctx, plan, pname, pairs, kw, g, entry="host")
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
    """Single pairs with a guess on the wide update, behind brute force and on the two-tile target."""
    kw, g = GUESS_SETS[name], _guesses(len(SINGLE))
    pairs = _pairs(SINGLE)
    orows = _oracle(oracle_mod, "single-guess", pairs, kw, g)
    for pname in ("wide", "brute"):
        rows, al = _run_single(gpu_ctx, plan, pname, pairs, kw, g)
        _equal_oracle(rows, al, pairs, orows, pname)
    _two_tile(gpu_ctx, oracle_mod, plan, "mt-guess", [_mt_pair(0)] * len(GUESSES), kw, np.stack(GUESSES))


# --------------------------------------------------- 3. failures among healthy pairs, and late ones
@pytest.mark.parametrize("guess", [False, True])
def test_oracle_rows_of_bad_pairs(oracle_mod, guess):
    """The oracle alone, flag on: an empty source is (-3, state 5, |C| 0, 0 iterations), an empty target
    -2, two points (-3, 5, 2, 0), a NaN or inf input -4, whatever the guess."""
    g = GUESSES[1] if guess else None
    for kind, (status, state, ncorr) in EXPECT.items():
        s, t = _replace(_pair(0), kind)
        o = oracle_mod.align(s, t, guess=g, numerics=oracle_mod.NUM_F32, **RECIP)
        assert (o["status"], o["convergence_state"], o["n_correspondences"]) == (status, state, ncorr), kind
        assert o["iterations"] == 0 and not o["converged"], kind
        if status != E_TOO_FEW_CORR:
            assert (o["T"] == np.eye(4)).all() and o["fitness"] == np.finfo(np.float64).max, kind
    assert BAD[0] == BAD[128] == BAD[130] == BAD_SMALL[0] == "empty_src"  # first in the batch and in a pair group


@gpu
@pytest.mark.parametrize("guess", [False, True])
def test_bad_pairs_among_healthy_ones(gpu_ctx, oracle_mod, plan, guess):
    """Invalid and too-small pairs inside a batch (an empty source first in the batch and first in the
    second and third pair group: the stage clamps a point index to n - 1): their rows are the oracle's,
    and every other pair's row and aligned cloud are byte-equal to the same batch without them, which
    equals the oracle."""
    healthy = _pairs(ALL)
    mixed260 = _with_bad(healthy, BAD)
    g = _guesses() if guess else None
    kw = _on()
    orows = _oracle(oracle_mod, "all-guess" if guess else "all", healthy, kw, g)
    for pname in ("lds-2groups", "lds-wide", "lds-3groups", "tiled", "small"):
        rows0, al0, ix = _run_batch(gpu_ctx, plan, pname, healthy, kw, g)
        if pname == "small":
            kinds = [BAD_SMALL.get(k) for k in range(len(ix))]
            mixed = _with_bad(_sub(healthy, ix), BAD_SMALL)
            rows, al, _ = _run_batch(gpu_ctx, plan, pname, mixed, kw, None if g is None else g[ix], ix=range(len(ix)))
        else:
            kinds = [BAD.get(i) for i in ix]
            mixed = _sub(mixed260, ix)
            rows, al, _ = _run_batch(gpu_ctx, plan, pname, mixed260, kw, g)
        assert (rows0["status"] == 0).all(), pname
        _equal_oracle(rows0, al0, _sub(healthy, ix), _sub(orows, ix), pname)
        assert kinds[0] == "empty_src"
        if pname == "lds-3groups":
            assert kinds[130] == kinds[260] == "empty_src"
        for k, kind in enumerate(kinds):
            if kind is not None:
                o = oracle_mod.align(*mixed[k], guess=None if g is None else g[ix[k]], aligned=True,
                                     numerics=oracle_mod.NUM_F32, **RECIP)
                assert (o["status"], o["convergence_state"], o["n_correspondences"]) == EXPECT[kind]
                _equal_oracle(rows[k: k + 1], al[k: k + 1], mixed[k: k + 1], [o], (pname, kind, k))
                if o["status"] != E_TOO_FEW_CORR:
                    assert rows[k]["T"].tobytes() == np.eye(4, dtype=np.float32).tobytes(), (pname, k)
                    assert rows[k]["fitness"] == np.finfo(np.float64).max and rows[k]["iterations"] == 0
            else:
                assert rows[k].tobytes() == rows0[k].tobytes(), (pname, k)
                assert al[k].tobytes() == al0[k].tobytes(), (pname, k)


@gpu
@pytest.mark.parametrize("guess", [False, True])
def test_bad_single_pairs(gpu_ctx, oracle_mod, plan, guess):
    """The same bad pairs one by one on every single-pair plan, each after a healthy call with as many
    source points (whose winner words, sorted copy and boxes the stage's workspace still holds)."""
    for pname in SINGLE_PLANS:
        good = _mt_pair(0) if pname in TWO_TILE else _pair(0)
        pairs, kinds = [], []
        for kind in EXPECT:
            pairs += [good, _replace(good, kind)]
            kinds += [None, kind]
        gs = np.stack([GUESSES[1]] * len(pairs)) if guess else None
        rows, al = _run_single(gpu_ctx, plan, pname, pairs, _on(), gs)
        orows = [oracle_mod.align(s, t, guess=None if gs is None else gs[k], numerics=oracle_mod.NUM_F32, aligned=True,
                                  **RECIP) for k, (s, t) in enumerate(pairs)]
        _equal_oracle(rows, al, pairs, orows, pname)
        for o, kind in zip(orows, kinds):
            assert o["status"] == (0 if kind is None else EXPECT[kind][0]), (pname, kind)


def test_oracle_min_correspondences_above_n(oracle_mod):
    """min_correspondences = 1000, the oracle alone: with the flag on 43 of the first 48 pairs fail at
    iteration 0 (24 with it off) and 5 finish; pairs of 1000 or more sources fail with the flag on and
    pass with it off — the count runs over the kept list, not the candidates."""
    pairs = _pairs(FIRST48)
    on = _oracle(oracle_mod, "first48", pairs, _on(ABOVE_N))
    off = _oracle(oracle_mod, "first48", pairs, ABOVE_N)
    failed0 = lambda rows: sum(r["status"] == E_TOO_FEW_CORR and r["iterations"] == 0 for r in rows)  # noqa: E731
    assert failed0(on) == 43 and failed0(off) == 24 and sum(r["status"] == 0 for r in on) == 5
    flipped = [k for k, (a, b) in enumerate(zip(on, off)) if a["status"] == E_TOO_FEW_CORR and b["status"] == 0]
    assert len(flipped) == 19 and all(len(pairs[k][0]) >= 1000 for k in flipped)
    assert all(on[k]["n_correspondences"] < 1000 <= off[k]["n_correspondences"] for k in flipped)
    assert set(flipped) & set(R_SINGLE) and set(flipped) & set(R_SMALL)


@gpu
def test_min_correspondences_above_n(gpu_ctx, oracle_mod, plan):
    _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), _on(ABOVE_N))
    _two_tile(gpu_ctx, oracle_mod, plan, "mt", [_mt_pair(0), _mt_pair(1)], _on(ABOVE_N))


def _late_failure(oracle_mod, pair, dist=None, iters=12):
    """From the oracle's trace, flag on: (j, min_correspondences) such that the pair fails at the first
    iteration j >= 1 whose |C| falls below every earlier one; None if |C| never does."""
    kw = {} if dist is None else {"max_correspondence_distance": dist}
    nc = oracle_mod.align(*pair, numerics=oracle_mod.NUM_F32, trace=True, max_iterations=iters, **kw,
                          **RECIP)["trace"]["ncorr"]
    for j in range(1, len(nc)):
        if nc[j] < nc[:j].min():
            return j, int(nc[:j].min())
    return None


def _late_kw(oracle_mod, iters=12):
    _, mc = _late_failure(oracle_mod, _pair(LATE))
    return _on(min_correspondences=mc, max_iterations=iters)


def test_oracle_fails_after_iterating(oracle_mod):
    """The oracle alone, flag on, no threshold: none of the first 48 pairs has a count that falls below
    all its earlier ones; of the 260, pairs 69, 92, 117, 191, 215 and 230 do.  With pair 69's derived
    min_correspondences (813, iteration 2) it fails after iterating and keeps the product of the
    transforms so far, the iterations done, the failing count and a fitness; the two-tile pair seeded
    4301 has a late failure of its own at distance 1.0 (iteration 1, 268)."""
    assert all(_late_failure(oracle_mod, _pair(k)) is None for k in FIRST48)
    found = {k: _late_failure(oracle_mod, _pair(k)) for k in (69, 92, 117, 191, 215, 230)}
    assert found == {69: (2, 813), 92: (1, 886), 117: (1, 658), 191: (2, 564), 215: (1, 434), 230: (1, 440)}
    assert LATE in R_SINGLE and LATE in R_SMALL
    assert _late_failure(oracle_mod, _mt_pair(LATE_MT["pair"]), LATE_MT["dist"]) == (1, 268)
    kw = _late_kw(oracle_mod)
    assert kw["min_correspondences"] == 813
    for cap in (11, 12):  # (the failure iteration is the same under both caps)
        r = oracle_mod.align(*_pair(LATE), numerics=oracle_mod.NUM_F32, aligned=True, **_late_kw(oracle_mod, cap))
        assert _failed_late(r) and r["iterations"] == 2
        assert r["convergence_state"] == CONV_NO_CORR and not r["converged"]
        assert not (r["T"] == np.eye(4)).all() and r["n_correspondences"] < kw["min_correspondences"]
        assert r["fitness"] < np.finfo(np.float64).max
        assert (r["aligned"][:, :3] != _pair(LATE)[0][:, :3]).any()
    rows = [oracle_mod.align(*_pair(k), numerics=oracle_mod.NUM_F32, **kw) for k in R_SMALL]
    assert any(r["status"] == E_TOO_FEW_CORR and r["iterations"] == 0 for r in rows)
    assert any(r["status"] == 0 for r in rows)


@gpu
@pytest.mark.parametrize("cap", [11, 12])
def test_failure_after_iterating(gpu_ctx, oracle_mod, plan, cap):
    """|C| < min_correspondences at iteration >= 1, counted over the kept list: the row keeps the product
    of the transforms so far, the iterations done and the failing count, and the fitness pass and the
    aligned cloud use that T (a deferred transform included), on every plan, both parities of the cap."""
    kw = _late_kw(oracle_mod, cap)
    orows = _every_plan(gpu_ctx, oracle_mod, plan, "all", _pairs(ALL), kw)
    assert _failed_late(orows[LATE]) and sum(_failed_late(r) for r in orows) >= 1
    j, mc = _late_failure(oracle_mod, _mt_pair(LATE_MT["pair"]), LATE_MT["dist"])
    mt = _on(max_correspondence_distance=LATE_MT["dist"], min_correspondences=mc, max_iterations=cap)
    orows = _two_tile(gpu_ctx, oracle_mod, plan, "mt", [_mt_pair(0), _mt_pair(1)], mt)
    assert _failed_late(orows[LATE_MT["pair"]]) and orows[LATE_MT["pair"]]["iterations"] == j


# ------------------------------------------------------- 4. overflowing and huge coordinates
R_OVERFLOW_SETS = {k: _on(OVERFLOW_SETS[k]) for k in ("defaults", "fixed", "threshold")}  # (Huber: F64 only)
R_HUBER = _on(OVERFLOW_SETS["huber"])
KEPT = {"src": 534, "tgt": 537, "both": 528}
R_HUGE = _on(HUGE)
HUGE_AT = (0, 64, 129, 130, 259)


def _huge_batch():
    return [_huge(p) if k in HUGE_AT else p for k, p in enumerate(_pairs(ALL))]


def _mt_overflow():
    return [_overflow(_mt_pair(0), v) for v in VARIANTS]


def test_oracle_registers_overflowing_clouds(oracle_mod):
    """The oracle alone, flag on: the 700 x 650 variants register with finite T and keep 534 (src), 537
    (tgt) and 528 (both) correspondences at the default threshold; the aligned cloud is finite for every
    planted input used below (no NaN distance arises, whose ordering FLANN and the key order would not
    share; +inf distances do); the 2e17 point gives status 0, 8 iterations, a finite T and a fitness
    near 5.7e31."""
    for v in VARIANTS:
        s, t = _overflow_pair(v)
        for name, kw in list(R_OVERFLOW_SETS.items()) + [("huber", dict(R_HUBER, numerics=oracle_mod.NUM_F64))]:
            kw = dict(kw)
            kw.setdefault("numerics", oracle_mod.NUM_F32)
            o = oracle_mod.align(s, t, aligned=True, **kw)
            assert o["status"] == 0 and o["converged"], (v, name)
            assert np.isfinite(o["T"]).all() and np.isfinite(o["aligned"]).all() and 1.0 < o["fitness"] < 10.0
            if "max_correspondence_distance" not in kw:
                assert o["n_correspondences"] == KEPT[v], (v, name)
        _, d2 = oracle_mod.nearest(s, t)
        assert np.isinf(d2).sum() == (0 if v == "tgt" else 12)
    batch = _overflow_batch()
    planted = [batch[k] for k in sorted(set(OVERFLOW_AT) | {1, 2, 6})] + _mt_overflow()
    for kw in R_OVERFLOW_SETS.values():
        for s, t in planted:
            o = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, aligned=True, **kw)
            assert o["status"] == 0 and np.isfinite(o["aligned"]).all() and np.isfinite(o["T"]).all()
            assert o["n_correspondences"] < len(s)
    o = oracle_mod.align(*_huge(_overflow_pair("none")), numerics=oracle_mod.NUM_F32, aligned=True, **R_HUGE)
    assert o["status"] == 0 and o["iterations"] == 8 and o["n_correspondences"] == 543
    assert np.isfinite(o["T"]).all() and np.isfinite(o["aligned"]).all() and 5.6e31 < o["fitness"] < 5.8e31


@gpu
@pytest.mark.parametrize("name", sorted(R_OVERFLOW_SETS))
def test_overflowing_coordinates_on_every_plan(gpu_ctx, oracle_mod, plan, name):
    """Every plan: the +inf the stage writes for a rejection beside the +inf of an overflowing d2, and
    source boxes whose bounds overflow."""
    kw = R_OVERFLOW_SETS[name]
    pairs = _overflow_batch()
    orows = _every_plan(gpu_ctx, oracle_mod, plan, "overflow", pairs, kw)
    assert all(np.isfinite(r["aligned"]).all() for r in orows)
    _two_tile(gpu_ctx, oracle_mod, plan, "mt-overflow", _mt_overflow(), kw)


def _f64_bars(rows, orows, label, iterations=None):
    """The bars of test_icp_params.test_f64_batch_vs_oracle_f64: equal iteration and correspondence
    counts, pose within 2e-6 m / rad, fitness within 1e-6 relative."""
    worst = [0.0, 0.0, 0.0]
    for k, (r, o) in enumerate(zip(rows, orows)):
        assert r["status"] == o["status"] == 0, (label, k)
        assert r["iterations"] == o["iterations"] and r["n_correspondences"] == o["n_correspondences"], (label, k)
        assert iterations is None or o["iterations"] == iterations
        dt, dr = pose_err(r["T"].reshape(4, 4).T, o["T"])
        worst = [max(a, b) for a, b in zip(worst, (dt, dr, abs(r["fitness"] - o["fitness"]) / o["fitness"]))]
    print(f"{label}: worst dt {worst[0]:.3e} m, dr {worst[1]:.3e} rad, fitness {worst[2]:.3e} relative")
    assert worst[0] <= 2e-6 and worst[1] <= 2e-6 and worst[2] <= 1e-6, (label, worst)


HUBER_SINGLE = (1, 2, 6, 0, 3)  # the three 700 x 650 variants and two planted pairs of the batch


def _huber_kw():
    return dict(R_HUBER, max_iterations=8, **FIXED)


def test_oracle_overflowing_huber_inputs(oracle_mod):
    """The oracle alone, F64 with Huber weights and with PCL numerics with them, flag on, on the planted
    pairs and the two-tile variants: status 0, the 8 iterations, finite T and aligned cloud, and the
    flag rejects something."""
    batch = _overflow_batch()
    planted = [batch[k] for k in sorted(set(OVERFLOW_AT) | {1, 2, 6})] + _mt_overflow()
    for num in (oracle_mod.NUM_F64, oracle_mod.NUM_F32):
        for s, t in planted:
            o = oracle_mod.align(s, t, numerics=num, aligned=True, **_huber_kw())
            assert o["status"] == 0 and o["iterations"] == 8 and o["n_correspondences"] < len(s)
            assert np.isfinite(o["T"]).all() and np.isfinite(o["aligned"]).all()


@gpu
def test_overflowing_coordinates_huber_f64(gpu_ctx, oracle_mod, plan):
    """Huber weights in F64 numerics on the overflowing batch, a fixed 8 iterations, on every plan: the
    five 260- to 390-pair batches, the 5-pair batch, the variants and two planted pairs one by one on
    every single-pair plan (F64 has no 1024-thread update: wide, wide-eager and fold-single differ in
    the deferred transform only) and the three two-tile variants, within the F64 bars."""
    import icp4r

    kw = _huber_kw()
    pairs = _overflow_batch()
    orows = _oracle(oracle_mod, "overflow", pairs, dict(kw, numerics=oracle_mod.NUM_F64))
    dkw = dict(kw, numerics=icp4r.NUMERICS_F64)
    for name in BATCH_PLANS:
        rows, _, ix = _run_batch(gpu_ctx, plan, name, pairs, dkw)
        _f64_bars(rows, _sub(orows, ix), "overflow huber " + name, 8)
    for name in ONE_TILE:
        rows, _ = _run_single(gpu_ctx, plan, name, _sub(pairs, HUBER_SINGLE), dkw)
        _f64_bars(rows, _sub(orows, HUBER_SINGLE), "overflow huber " + name, 8)
    mt = _mt_overflow()
    mrows = _oracle(oracle_mod, "mt-overflow", mt, dict(kw, numerics=oracle_mod.NUM_F64))
    for name in TWO_TILE:
        rows, _ = _run_single(gpu_ctx, plan, name, mt, dkw)
        _f64_bars(rows, mrows, "overflow huber " + name, 8)


@gpu
def test_overflowing_coordinates_huber_pcl(gpu_ctx, oracle_mod, plan):
    """Huber weights in PCL numerics, flag on (the flag-off matrix pins them in bits on every plan): a
    record's weight is formed before the stage marks a rejection, and the update must drop the record
    all the same.  Every plan, equal to the oracle in bits."""
    kw = _huber_kw()
    _every_plan(gpu_ctx, oracle_mod, plan, "overflow", _overflow_batch(), kw)
    _two_tile(gpu_ctx, oracle_mod, plan, "mt-overflow", _mt_overflow(), kw)


@gpu
def test_huge_coordinate(gpu_ctx, oracle_mod, plan):
    """One source point at 2e17 (d2 4e34 < FLT_MAX: huge, not overflowing), fixed iterations: its key
    must lose or win its target's vote as any other."""
    one = [_huge(_overflow_pair("none"))]
    orow = _oracle(oracle_mod, "huge-one", one, R_HUGE)
    for name in ONE_TILE:
        rows, al = _run_single(gpu_ctx, plan, name, one, R_HUGE)
        _equal_oracle(rows, al, one, orow, name)
    _every_plan(gpu_ctx, oracle_mod, plan, "huge", _huge_batch(), R_HUGE, single=HUGE_AT[:2] + (3, 8),
                single_plans=("wide", "brute"))


# --------------------------------------------------------------------------------- 5. strides
STRIDES = [(sc, tc) for sc in (3, 4, 5, 8) for tc in (3, 4, 5, 8) if sc == 4 or tc == 4 or sc == tc]


def test_oracle_strided_inputs(oracle_mod):
    """The oracle alone, flag on: the strided forms of pair 3 register with the guess (status 0, the flag
    rejects something) and give one and the same row whatever the strides; so does the 20- / 32-byte
    pair of the output-stride test without a guess."""
    s4, t4 = _pair(3)
    ref = None
    for sc, tc in STRIDES:
        o = oracle_mod.align(_strided(s4, sc), _strided(t4, tc), guess=GUESSES[1], numerics=oracle_mod.NUM_F32,
                             aligned=True, **RECIP)
        assert o["status"] == 0 and o["iterations"] >= 2 and o["n_correspondences"] < len(s4), (sc, tc)
        got = (o["T"].tobytes(), o["fitness"], o["iterations"], o["n_correspondences"], o["aligned"][:, :3].tobytes())
        ref = got if ref is None else ref
        assert got == ref, (sc, tc)
    o = oracle_mod.align(_strided(s4, 5), _strided(t4, 8), numerics=oracle_mod.NUM_F32, **RECIP)
    assert o["status"] == 0 and o["n_correspondences"] < len(s4) and not (o["T"] == np.eye(4)).all()


@gpu
def test_point_strides(gpu_ctx, oracle_mod):
    """12-, 16-, 20- and 32-byte points through a reciprocal align with a guess: byte-equal results across
    the strides and equal to the oracle; the aligned intensity is 0 for a 12-byte source."""
    import icp4r

    s4, t4 = _pair(3)
    T = GUESSES[1]
    ref = None
    for sc, tc in STRIDES:
        s, t = _strided(s4, sc), _strided(t4, tc)
        r, al = gpu_ctx.align(s, t, icp4r.default_params(**RECIP), guess=T, want_aligned=True)
        o = oracle_mod.align(s, t, guess=T, numerics=oracle_mod.NUM_F32, aligned=True, **RECIP)
        assert o["status"] == 0 and o["n_correspondences"] < len(s)
        row = np.frombuffer(bytes(r), icp4r.RESULT_DTYPE)
        _equal_oracle(row, [al], [(s, t)], [o], (sc, tc))
        assert (al[:, 3] == (0.0 if sc == 3 else s4[:, 3])).all(), (sc, tc)
        got = (row.tobytes(), al[:, :3].tobytes())
        ref = got if ref is None else ref
        assert got == ref, (sc, tc)


@gpu
def test_output_strides(gpu_ctx, oracle_mod):
    """icp4r_align's out_stride_bytes with the flag on: 32 writes x, y, z and the intensity and leaves a
    point's other four floats alone; 12 writes nothing past a point's three floats."""
    import icp4r

    s, t = _strided(_pair(3)[0], 5), _strided(_pair(3)[1], 8)
    o = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, aligned=True, **RECIP)
    n = len(s)
    L = icp4r.load()

    def call(out, stride):
        r, p = icp4r.Result(), icp4r.default_params(**RECIP)
        rc = L.icp4r_align(gpu_ctx.handle, s.ctypes.data, n, 20, t.ctypes.data, len(t), 32, None, C.byref(p),
                           C.byref(r), out.ctypes.data, stride)
        assert rc == 0 and r.matrix().tobytes() == o["T"].tobytes()
        assert r.n_correspondences == o["n_correspondences"] < n

    wide = np.full((n, 8), np.nan, np.float32)
    call(wide, 32)
    assert wide[:, :4].tobytes() == o["aligned"].tobytes() and (wide[:, 3] == s[:, 3]).all()
    assert np.isnan(wide[:, 4:]).all()
    tight = np.full(3 * n + 8, np.nan, np.float32)
    call(tight, 12)
    assert tight[:3 * n].tobytes() == np.ascontiguousarray(o["aligned"][:, :3]).tobytes()
    assert np.isnan(tight[3 * n:]).all()


# --------------------------------------------------------------- 6. F64 numerics in a batch
def _f64_kw(huber):
    return _on(FIXED, max_iterations=12, **({"huber_delta": 0.5} if huber else {}))


@pytest.mark.parametrize("huber", [False, True])
def test_oracle_f64_batch_inputs(oracle_mod, huber):
    """The F64 oracle alone, flag on, on the first 48 pairs: status 0, the 12 iterations, the flag
    rejects something for every pair, and the Huber weights change the poses."""
    pairs = _pairs(FIRST48)
    rows = _oracle(oracle_mod, "first48", pairs, dict(_f64_kw(huber), numerics=oracle_mod.NUM_F64))
    assert all(o["status"] == 0 and o["iterations"] == 12 for o in rows)
    assert all(o["n_correspondences"] < len(s) for o, (s, _) in zip(rows, pairs))
    if huber:
        plain = _oracle(oracle_mod, "first48", pairs, dict(_f64_kw(False), numerics=oracle_mod.NUM_F64))
        assert sum(not (a["T"] == b["T"]).all() for a, b in zip(rows, plain)) >= 40


@gpu
@pytest.mark.parametrize("huber", [False, True])
def test_f64_batch_vs_oracle_f64(gpu_ctx, oracle_mod, plan, huber):
    """NUMERICS_F64 with the flag on, the 260-pair batch and the 5-pair batch against the F64 oracle,
    every pair, within the bars of test_icp_params.test_f64_batch_vs_oracle_f64."""
    import icp4r

    kw = _f64_kw(huber)
    pairs = _pairs(ALL)
    orows = _oracle(oracle_mod, "all", pairs, dict(kw, numerics=oracle_mod.NUM_F64))
    assert all(o["n_correspondences"] < len(s) for o, (s, _) in zip(orows, pairs))
    for name in ("lds-2groups", "lds-3groups", "small"):
        rows, _, ix = _run_batch(gpu_ctx, plan, name, pairs, dict(kw, numerics=icp4r.NUMERICS_F64))
        _f64_bars(rows, _sub(orows, ix), name, 12)


# ------------------------------------------------------------------- 7. the other entries, flag on
@gpu
def test_align_batch_multi_and_sharded(gpu_ctx, oracle_mod):
    """icp4r_align_batch_multi over 3 contexts on one device and icp4r_align_batch_sharded on a one-rank
    communicator, flag on: byte-equal to the single batch, which equals the oracle."""
    import torch

    import icp4r

    ix = list(range(16)) + [LATE]
    pairs = _pairs(ix)
    kw = _on(SETS["D"])
    params = icp4r.default_params(**kw)
    ref = gpu_ctx.align_batch_host(*_concat(pairs), params=params)
    _equal_oracle(ref, None, pairs, _sub(_oracle(oracle_mod, "all", _pairs(ALL), kw), ix), "single batch")
    ctxs = [icp4r.Context(0) for _ in range(3)]
    try:
        got = icp4r.align_batch_multi(ctxs, *_concat(pairs), params=params)
    finally:
        for c in ctxs:
            c.close()
    assert got.tobytes() == ref.tobytes()
    dev = torch.device("cuda", 0)
    src, so, sn, tgt, to, tn = _concat(pairs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t = [up(a) for a in (src, so, sn, tgt, to, tn)]
    P = len(pairs)
    batch = icp4r.Batch(src=t[0].data_ptr(), tgt=t[3].data_ptr(), src_off=t[1].data_ptr(), src_n=t[2].data_ptr(),
                        tgt_off=t[4].data_ptr(), tgt_n=t[5].data_ptr(), guess=None, aligned=None, npairs=P,
                        max_src_n=int(sn.max()), max_tgt_n=int(tn.max()))
    stream = torch.cuda.current_stream(dev).cuda_stream
    comm = icp4r.Comm(gpu_ctx, 1, 0, icp4r.Comm.unique_id())
    try:
        rows = torch.zeros((P, 96), dtype=torch.uint8, device=dev)
        gathered = torch.full((P, 96), 255, dtype=torch.uint8, device=dev)
        comm.align_batch_sharded(batch, P, params, rows.data_ptr(), gathered.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        assert rows.cpu().numpy().tobytes() == ref.tobytes() and gathered.cpu().numpy().tobytes() == ref.tobytes()
    finally:
        comm.close()


def _static_frames():
    from icp4r import synth

    return synth.make_sequence(30 + 1024, frames=6, n=1024, dynamic=0.3)[0]


def test_oracle_static_sequence_inputs(oracle_mod):
    """The oracle alone on the ungated scans of the sequence below: frame 0 (a scan against itself)
    keeps every point and equals the flag-off row; frames 1 to 5 keep 566 to 586 of 1024."""
    from icp4r import synth

    xyzi = [synth.records_to_xyzi(f) for f in _static_frames()]
    for k in range(6):
        on = oracle_mod.align(xyzi[k], xyzi[k - 1 if k else 0], numerics=oracle_mod.NUM_F32, **RECIP)
        off = oracle_mod.align(xyzi[k], xyzi[k - 1 if k else 0], numerics=oracle_mod.NUM_F32)
        assert on["status"] == 0
        if k == 0:
            assert on["n_correspondences"] == 1024 and all(np.array_equal(on[f], off[f]) for f in on)
        else:
            assert 566 <= on["n_correspondences"] <= 586 and not np.array_equal(on["T"], off["T"]), k


@gpu
def test_register_static_sequence(gpu_ctx, oracle_mod):
    """ego.register_static_sequence(..., icp_params = reciprocal), GATE_STATIC, both pairings: the source
    and target of every pair lie in the one packed buffer.  Every frame equals the oracle (flag on) on
    the twin-compacted clouds and align_batch_host on host copies; frame 0 equals flag off, the others
    do not; with an empty scan the node's pairing registers the carried-over clouds."""
    import gate_twin
    import icp4r
    from icp4r import ego
    from test_gate_gpu import _host_batch, _node_pairs, _twin_clouds

    frames = _static_frames()
    p = ego.default_params(seed=31)
    ip = icp4r.default_params(**RECIP)
    node = ego.register_static_sequence(frames, pairing=ego.PAIR_NODE, ego_params=p, icp_params=ip, ctx=gpu_ctx,
                                        want_masks=True)
    strict = ego.register_static_sequence(frames, pairing=ego.PAIR_STRICT, ego_params=p, icp_params=ip, ctx=gpu_ctx)
    off = ego.register_static_sequence(frames, pairing=ego.PAIR_NODE, ego_params=p, ctx=gpu_ctx)
    _, icp, reg, masks = node
    assert reg.tolist() == [1] * 6
    clouds = _twin_clouds(frames, masks, gate_twin.GATE_STATIC)
    pairs = _node_pairs(clouds)
    host = _host_batch(gpu_ctx, pairs, ip)
    for k, src, tgt in pairs:
        o = oracle_mod.align(src, tgt, numerics=oracle_mod.NUM_F32, **RECIP)
        _equal_oracle(icp[k: k + 1], None, [(src, tgt)], [o], k)
        assert icp[k].tobytes() == host[k].tobytes() == strict[1][k].tobytes(), k
        if k == 0:
            assert o["n_correspondences"] == len(src) and icp[k].tobytes() == off[1][k].tobytes()
        else:
            assert o["n_correspondences"] < len(src) and icp[k]["T"].tobytes() != off[1][k]["T"].tobytes(), k
    # an empty scan 3: frame 3 is skipped, frame 4 registers scan 4 against scans 2 and 3 carried over
    frames[3] = frames[3][:0]
    _, icp, reg, masks = ego.register_static_sequence(frames, pairing=ego.PAIR_NODE, ego_params=p, icp_params=ip,
                                                      ctx=gpu_ctx, want_masks=True)
    pairs = _node_pairs(_twin_clouds(frames, masks, gate_twin.GATE_STATIC))
    assert reg.tolist() == [1, 1, 1, 0, 1, 1] and [k for k, _, _ in pairs] == [0, 1, 2, 4, 5]
    host = _host_batch(gpu_ctx, pairs, ip)
    for q, (k, src, tgt) in enumerate(pairs):
        o = oracle_mod.align(src, tgt, numerics=oracle_mod.NUM_F32, **RECIP)
        _equal_oracle(icp[k: k + 1], None, [(src, tgt)], [o], k)
        assert icp[k].tobytes() == host[q].tobytes(), k


def _replay_frames():
    """Six ragged scans without movers and without Doppler noise: the node's delta > 0.2 test keeps every
    point, so --static-points registers the same clouds as the other modes."""
    from icp4r import synth

    frames, _ = synth.make_sequence(16, frames=6, n=1024, dynamic=0.0, doppler_noise=0.0)
    frames[3] = frames[3][:700]
    return frames


def test_oracle_replay_gate_keeps_everything(oracle_mod):
    for k, f in enumerate(_replay_frames()):
        ft = oracle_mod.ego_features(f)
        A, b, _, _, _ = oracle_mod.ego_ransac(ft, seed=77 + (k << 32))
        assert oracle_mod.ego_split_lsq(ft, A, b)[2] == len(f), k


@gpu
def test_replay_reciprocal(tmp_path, oracle_mod):
    """icp4radar_replay --reciprocal: the per-frame loop (the C++ facade's setter), --batch, --devices
    0,0,0 and --static-points --batch write identical ICP text, which is the node's loop restated over
    the oracle with the flag on, and not the text without --reciprocal."""
    from icp4r import synth
    from test_replay import _check_against_oracle, _run_replay

    synth.write_sequence(str(tmp_path), _replay_frames())
    seed = 77
    modes = {"frame": [], "batch": ["--batch"], "multi": ["--batch", "--devices", "0,0,0"],
             "static": ["--static-points", "--batch"]}
    outs = {m: _run_replay(tmp_path, seed, False, tmp_path / f"out_{m}.csv", ["--reciprocal"] + extra)
            for m, extra in modes.items()}
    icp_cols = lambda o: [ln.split(",")[:18] for ln in o["csv"].splitlines()]  # noqa: E731
    for m in modes:
        assert outs[m]["icp.txt"] == outs["frame"]["icp.txt"] and outs[m]["pcl_info.txt"] == outs["frame"]["pcl_info.txt"], m
        assert icp_cols(outs[m]) == icp_cols(outs["frame"]), m
    assert outs["batch"] == outs["frame"] and outs["multi"] == outs["frame"]
    _check_against_oracle(outs["batch"], tmp_path, oracle_mod, seed, reciprocal=True)
    plain = _run_replay(tmp_path, seed, True, tmp_path / "plain.csv")
    assert plain["icp.txt"] != outs["batch"]["icp.txt"]


FACADE_CPP = r"""
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include <icp4r/pcl_compat.hpp>
using Cloud = pcl::PointCloud<pcl::PointXYZI>;
static Cloud::Ptr load(const char* path) {
    Cloud::Ptr c(new Cloud);
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return c;
    float p[4];
    while (std::fread(p, sizeof(float), 4, f) == 4) c->push_back(pcl::PointXYZI(p[0], p[1], p[2], p[3]));
    std::fclose(f);
    return c;
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    Cloud::Ptr src = load(argv[1]), tgt = load(argv[2]);
    pcl::IterativeClosestPoint<pcl::PointXYZI, pcl::PointXYZI> icp;
    icp.setInputSource(src);
    icp.setInputTarget(tgt);
    icp.setUseReciprocalCorrespondences(true);
    Cloud out;
    icp.align(out);
    const Eigen::Matrix4f T = icp.getFinalTransformation();
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            const float v = T(r, c);
            unsigned u;
            std::memcpy(&u, &v, 4);
            std::printf("%08x ", u);
        }
    const double fit = icp.getFitnessScore();
    unsigned long long b;
    std::memcpy(&b, &fit, 8);
    std::printf("\n%016llx\n%d %d %zu\n", b, icp.hasConverged() ? 1 : 0, icp.getNrIterations(), out.size());
    return 0;
}
"""


@gpu
def test_cpp_facade_registration(tmp_path, oracle_mod):
    """A program over pcl_compat.hpp with setUseReciprocalCorrespondences(true) aligns a 700 x 650 pair:
    T and the fitness, printed as hex bits, are the oracle's with the flag on (and not with it off)."""
    s, t = _pair(0)
    assert (len(s), len(t)) == (700, 650)
    o = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, **RECIP)
    off = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32)
    assert o["status"] == 0 and o["T"].tobytes() != off["T"].tobytes()
    np.ascontiguousarray(s, np.float32).tofile(tmp_path / "src.bin")
    np.ascontiguousarray(t, np.float32).tofile(tmp_path / "tgt.bin")
    cpp, exe = tmp_path / "recip_align.cpp", tmp_path / "recip_align"
    cpp.write_text(FACADE_CPP)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/include", "-o", str(exe), str(cpp),
                        f"-L{LIB}", "-licp4r", f"-Wl,-rpath,{LIB}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe), str(tmp_path / "src.bin"), str(tmp_path / "tgt.bin")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    want_T = " ".join("%08x" % u for u in np.ascontiguousarray(o["T"].T).view(np.uint32).reshape(-1))
    assert lines[0].strip() == want_T
    assert lines[1] == "%016x" % np.float64(o["fitness"]).view(np.uint64)
    assert lines[2] == f"{int(o['converged'])} {o['iterations']} {len(s)}"
