"""Voxelized GICP over its parameter space (include/icp4r/icp4r_vgicp.h): rejected Levenberg-Marquardt trials,
the lookup's integer side, large and lopsided batches, caps, epsilons, tiny targets, workspace reuse and the
map entry's arguments.  tests/test_vgicp_gpu.py holds the default paths; this file the rest.

The bars are the existing ones of tests/test_vgicp_gpu.py, no wider: poses within 1e-5 (m, rad) of the numpy
twin tests/vgicp_twin.py, iterations, converged and n_correspondences identical, the fitness within 1e-6
relative, device against device bit for bit.  The twin is fed the device's own covariances
(icp4r_gicp_covariances), as test_gpu_align_matches_twin does, so only the order of the Gauss-Newton sums
differs.  The tests without the gpu mark run the twin alone (oracle covariances, or none where only cells
count) and pin what the GPU tests rely on: that the chosen inputs really reject trials, really sit on the
faces and the key range's edge.

Rejected trials need a nearly singular H: sources of 2 or 3 points, where the first step at lambda = 1e-9
max|diag H| overshoots.  LM_ROWS lists them with the trial pattern measured on the twin (oracle covariances,
k = 5, PLANE) and the deviation between the twin's two summation orders (source points ascending and
reversed): the room a device that sums in a third order has inside the 1e-5 bar.

Measured on an MI355X: the 50 GPU cases take about 6 s in all (the slowest, a sweep of 12 calls, 0.7 s); the
largest deviation from the twin is 9.3e-7 m and 2.1e-8 rad.
"""
import ctypes as C

import numpy as np
import pytest

import vgicp_twin as tw
from helpers import pose_err
from test_gicp import _scene
from test_gicp_paths import _far_guess
from test_vgicp_gpu import _near_guess, _run_batch

K = 5
POSE_BAR = 1e-5       # m, rad: device against the twin
FITNESS_BAR = 1e-6    # relative
ORDER_BAR = 1e-7      # m, rad: the twin against itself with the source reversed (100 times inside POSE_BAR)


def _vgicp():
    from icp4r import vgicp

    return vgicp


def _dev_covs(ctx, cloud, k=K, reg=3):
    from icp4r import gicp

    return gicp.covariances(cloud, k, reg, ctx=ctx)


def _twin(src, tgt, CA, CB, p, G):
    """The twin with every parameter of p."""
    g = p.gicp
    return tw.align(src, tgt, CA, CB, resolution=p.voxel_resolution, mode=p.neighbor_search, guess=G,
                    max_iterations=g.max_iterations, rotation_epsilon=g.rotation_epsilon,
                    transformation_epsilon=g.transformation_epsilon, lm_max_iterations=g.lm_max_iterations,
                    lm_init_lambda_factor=g.lm_init_lambda_factor)


def _hold(group, what, T, iterations, converged, ncorr, fitness, o, src, tgt):
    """One device result against the twin's run o at the bars of this file."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    dt, dr = pose_err(T, o["T"])
    print(f"[{group}] {what}: dt {dt:.3e} dr {dr:.3e} iterations {iterations}/"
          f"{o['iterations']} converged {int(converged)}/{int(o['converged'])} correspondences {ncorr}/{o['n_valid']} "
          f"trials {o['trials']}")
    assert dt < POSE_BAR and dr < POSE_BAR, (what, dt, dr)
    assert iterations == o["iterations"] and bool(converged) == o["converged"], what
    assert ncorr == o["n_valid"], what
    if fitness is not None:
        fit = tw.fitness(src, tgt, T)
        assert abs(fitness - fit) <= FITNESS_BAR * max(fit, 1e-12), (what, fitness, fit)


def _hold_result(group, what, r, o, src, tgt):
    assert r.status == 0, what
    _hold(group, what, r.matrix(), r.iterations, r.converged, r.n_correspondences, r.fitness, o, src, tgt)


def _tuple(r, aligned):
    return (r.matrix().tobytes(), r.iterations, r.converged, r.fitness, r.n_correspondences, r.status,
            None if aligned is None else aligned.tobytes())


# =============================================================================== A. rejected LM trials
def _axis_guess(ang):
    """A rotation by ang rad about (0.2, 0.3, 1), then the translation (0.5, -0.3, 0.1)."""
    ax = np.array([0.2, 0.3, 1.0])
    ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    G = np.eye(4, dtype=np.float32)
    G[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    G[:3, 3] = [0.5, -0.3, 0.1]
    return G


LM_VALUES = (1, 2, 3, 5, 10)
# name -> seed, source points, ang, mode, resolution, (rotation_epsilon, transformation_epsilon) or None;
#         trials: the twin's trials per iteration with lm_max_iterations = 10;
#         runs: lm_max_iterations -> (iterations, converged, lm_failed);
#         order: the measured deviation (m, rad) between the twin's two summation orders, the largest over
#         LM_VALUES.
# The target is the first 1024 points of _scene(seed, 1024), the source the scene's first n source points.
# The last two rows converge on a rejected trial (stop == 2 of step_lm): the epsilons are raised until the
# rejected step itself counts as converged; in "stop2_at_iteration_1" iteration 0 first takes 5 trials.
LM_ROWS = {
    "s0_n3_direct7_res5": dict(
        seed=0, n=3, ang=0.0, mode=tw.DIRECT7, res=5.0, eps=None, trials=[6, 1, 1, 1, 1, 1, 1, 1, 1],
        runs={1: (0, False, True), 2: (0, False, True), 3: (0, False, True), 5: (0, False, True), 10: (8, True, False)},
        order=(1.6e-11, 2.4e-12)),
    "s1_n3_direct7_res5": dict(
        seed=1, n=3, ang=0.0, mode=tw.DIRECT7, res=5.0, eps=None, trials=[1, 5, 1, 1, 1, 1, 1, 1],
        runs={1: (1, False, True), 2: (1, False, True), 3: (1, False, True), 5: (7, True, False), 10: (7, True, False)},
        order=(2.1e-10, 6.2e-12)),
    "s1_n3_ang0p3_direct27_res2p5": dict(
        seed=1, n=3, ang=0.3, mode=tw.DIRECT27, res=2.5, eps=None, trials=[1, 6, 1, 1, 1, 1, 1],
        runs={1: (1, False, True), 2: (1, False, True), 3: (1, False, True), 5: (1, False, True), 10: (6, True, False)},
        order=(2.0e-10, 6.1e-12)),
    "s2_n2_direct27_res2p5": dict(
        seed=2, n=2, ang=0.0, mode=tw.DIRECT27, res=2.5, eps=None, trials=[5, 2, 2, 1, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1],
        runs={1: (0, False, True), 2: (0, False, True), 3: (0, False, True), 5: (14, True, False), 10: (14, True, False)},
        order=(6.3e-11, 5.4e-12)),
    "s3_n3_direct7_res5": dict(
        seed=3, n=3, ang=0.0, mode=tw.DIRECT7, res=5.0, eps=None, trials=[1, 1, 1, 1, 1, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
        runs={1: (5, False, True), 2: (5, False, True), 3: (5, False, True), 5: (15, True, False), 10: (15, True, False)},
        order=(3.0e-12, 7.6e-14)),
    "stop2_at_iteration_0": dict(
        seed=0, n=3, ang=0.0, mode=tw.DIRECT7, res=5.0, eps=(2.0, 10.0), trials=[1],
        runs={1: (0, True, False), 2: (0, True, False), 3: (0, True, False), 5: (0, True, False), 10: (0, True, False)},
        order=(0.0, 0.0)),
    "stop2_at_iteration_1": dict(
        seed=2, n=2, ang=0.0, mode=tw.DIRECT27, res=2.5, eps=(2.0, 10.0), trials=[5, 1],
        runs={1: (0, False, True), 2: (0, False, True), 3: (0, False, True), 5: (1, True, False), 10: (1, True, False)},
        order=(1.4e-12, 1.4e-13)),
}
STOP2_ROWS = ("stop2_at_iteration_0", "stop2_at_iteration_1")


def _lm_clouds(row):
    src, tgt, _ = _scene(row["seed"], 1024)
    return np.ascontiguousarray(src[:row["n"]]), np.ascontiguousarray(tgt[:1024]), _axis_guess(row["ang"])


def _lm_params(row, lm):
    kw = dict(k_correspondences=K, neighbor_search=row["mode"], voxel_resolution=row["res"], lm_max_iterations=lm)
    if row["eps"]:
        kw.update(rotation_epsilon=row["eps"][0], transformation_epsilon=row["eps"][1])
    return kw


def _lm_twin(row, src, tgt, CA, CB, G, lm):
    kw = {}
    if row["eps"]:
        kw = dict(rotation_epsilon=row["eps"][0], transformation_epsilon=row["eps"][1])
    return tw.align(src, tgt, CA, CB, resolution=row["res"], mode=row["mode"], guess=G, lm_max_iterations=lm, **kw)


@pytest.mark.parametrize("name", sorted(LM_ROWS))
def test_twin_rejected_trials(oracle_mod, name):
    """The rows reject trials on the twin as recorded, under every lm_max_iterations, and the twin's two
    summation orders agree: the same trial counts and iterations, poses within 1e-7."""
    row = LM_ROWS[name]
    src, tgt, G = _lm_clouds(row)
    CA = oracle_mod.gicp_covariances(src, K, oracle_mod.GICP_REG_PLANE)
    CB = oracle_mod.gicp_covariances(tgt, K, oracle_mod.GICP_REG_PLANE)
    worst = [0.0, 0.0]
    for lm in LM_VALUES:
        r = _lm_twin(row, src, tgt, CA, CB, G, lm)
        rev = _lm_twin(row, src[::-1], tgt, CA[::-1], CB, G, lm)
        dt, dr = pose_err(r["T"], rev["T"])
        worst = [max(worst[0], dt), max(worst[1], dr)]
        print(f"{name} lm {lm}: iterations {r['iterations']} converged {r['converged']} failed {r['lm_failed']} "
              f"trials {r['trials']} stops {r['stops']} reversed dt {dt:.2e} dr {dr:.2e}")
        assert (r["iterations"], r["converged"], r["lm_failed"]) == row["runs"][lm], lm
        assert rev["trials"] == r["trials"] and rev["stops"] == r["stops"] and rev["iterations"] == r["iterations"]
        assert (rev["converged"], rev["lm_failed"], rev["n_valid"]) == (r["converged"], r["lm_failed"], r["n_valid"])
        assert dt < ORDER_BAR and dr < ORDER_BAR, (lm, dt, dr)
        if lm == 10:
            assert r["trials"] == row["trials"]
        # a failed run stops at x0 of the failed iteration with every trial spent
        if r["lm_failed"]:
            assert r["trials"][-1] == lm and r["stops"][-1] == 0
        if name in STOP2_ROWS and not r["lm_failed"]:
            assert r["stops"][-1] == 2 and r["converged"]
    print(f"{name}: the two orders differ by {worst[0]:.2e} m {worst[1]:.2e} rad (recorded {row['order']})")


def test_twin_rejected_trials_cover_the_paths():
    """What the rows are for: at least three with an iteration of >= 3 trials (trials past two speculated
    ones), at least two that fail at an iteration > 0 under a small lm_max_iterations, an iteration of
    exactly 2 trials (the second speculative trial decides), and both stop == 2 cases."""
    plain = [r for n, r in LM_ROWS.items() if n not in STOP2_ROWS]
    assert len(plain) == 5
    assert sum(max(r["trials"]) >= 3 for r in plain) >= 3
    assert sum(r["runs"][1][2] and r["runs"][1][0] > 0 for r in plain) >= 2
    assert any(2 in r["trials"] for r in plain)
    r = LM_ROWS["s2_n2_direct27_res2p5"]
    assert sum(t >= 2 for t in r["trials"]) == 4 and sum(t >= 3 for t in r["trials"]) == 2 and max(r["trials"]) == 5
    for n in ("s0_n3_direct7_res5", "s1_n3_direct7_res5", "s1_n3_ang0p3_direct27_res2p5", "s3_n3_direct7_res5"):
        t = LM_ROWS[n]["trials"]
        assert sum(x >= 2 for x in t) == 1 and sum(x >= 3 for x in t) == 1 and max(t) in (5, 6)
    assert LM_ROWS["stop2_at_iteration_1"]["trials"] == [5, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM_ROWS))
def test_gpu_rejected_trials_match_twin(gpu_ctx, name):
    """The same rows and lm_max_iterations values on the device against the twin fed the device's covariances.
    First the twin: with these covariances the run still has its iterations of >= 3 trials."""
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    row = LM_ROWS[name]
    src, tgt, G = _lm_clouds(row)
    CA, CB = _dev_covs(gpu_ctx, src), _dev_covs(gpu_ctx, tgt)
    for lm in LM_VALUES:
        o = _lm_twin(row, src, tgt, CA, CB, G, lm)
        if lm == 10:
            assert o["trials"] == row["trials"], o["trials"]
            if name not in STOP2_ROWS:
                assert max(o["trials"]) >= 3
        assert (o["iterations"], o["converged"], o["lm_failed"]) == row["runs"][lm], lm
        r, _ = vgicp.align(src, tgt, vgicp.default_params(**_lm_params(row, lm)), guess=G, ctx=gpu_ctx)
        _hold_result("A", f"{name} lm {lm}", r, o, src, tgt)
        if o["lm_failed"]:  # the pose is x0 before the failed step (the twin's T)
            assert not r.converged
        if name in STOP2_ROWS and not o["lm_failed"]:
            assert o["stops"][-1] == 2 and r.converged


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LM_ROWS))
def test_gpu_rejected_trials_any_spec_and_grid(gpu_ctx, plan, name):
    """gicp_spec 0, 1 and 2 crossed with gicp_grid 1 and the default on inputs that reject trials, where the
    setting decides which code computes a trial's error (the trial kernel's speculative lanes or the one by
    one path through vgicp_point_err): results and aligned clouds bit-identical.  lm_max_iterations 1 with
    gicp_spec 2 evaluates one trial only (nt = 1).  A source of 2 or 3 points is one slice, so every gicp_grid
    launches one workgroup per pair: here only gicp_spec changes the launch (the grid matters with a wide
    pair, test_gpu_batch_one_wide_pair).  The crossing costs nothing and holds should that ever change."""
    vgicp = _vgicp()
    row = LM_ROWS[name]
    src, tgt, G = _lm_clouds(row)
    for lm in (1, 2, 10):
        p = vgicp.default_params(**_lm_params(row, lm))
        runs = []
        for spec in (2, 1, 0):
            for grid in (None, 1):
                gpu_ctx.reset_plan_options()
                plan(gicp_spec=spec, **({} if grid is None else {"gicp_grid": grid}))
                runs.append(_tuple(*vgicp.align(src, tgt, p, guess=G, want_aligned=True, ctx=gpu_ctx)))
        assert runs[0][5] == 0 and runs[0][1] == row["runs"][lm][0] and bool(runs[0][2]) == row["runs"][lm][1]
        for other in runs[1:]:
            assert other == runs[0], (name, lm)


# =============================================================================== B. the correspondence census
def _census(src, tgt, G, resolution, mode):
    """The number of (point, voxel) pairs of the linearisation at G: the twin's correspondences() at
    transform(G) (covariances play no part in it: identities)."""
    G = np.eye(4) if G is None else np.asarray(G, np.float32).astype(np.float64)
    vm = tw.voxel_map(tgt, np.broadcast_to(np.eye(3), (len(tgt), 3, 3)), resolution)
    a = np.asarray(src, np.float32)[:, :3].astype(np.float64)
    pi, vi = tw.correspondences(vm, tw.transform(G[:3, :3], G[:3, 3], a), resolution, mode)
    return len(pi), pi, vm.coords[vi] if len(vi) else np.zeros((0, 3), np.int32)


SWEEP_RES = (0.3, 0.5, 1.0, 2.5)
_sweep = {}


def _sweep_scene():
    if not _sweep:
        src, tgt, _ = _scene(0, 2048)
        _sweep["src"], _sweep["tgt"] = np.ascontiguousarray(src[:1500]), tgt
        _sweep["guess"] = {"none": None, "near": _near_guess(), "far": _far_guess()}
    return _sweep


def test_twin_census_sweep_separates_modes_and_guesses():
    """The sweep's counts grow with the mode everywhere, and DIRECT7's last offset (0, 0, -1) finds pairs in
    most of the sweep: a shortened offset list cannot leave every count equal."""
    s = _sweep_scene()
    a = s["src"].astype(np.float64)
    through_last = 0
    for res in SWEEP_RES:
        for g, G in s["guess"].items():
            n1, _, _ = _census(s["src"], s["tgt"], G, res, tw.DIRECT1)
            n7, pi, found = _census(s["src"], s["tgt"], G, res, tw.DIRECT7)
            n27, _, _ = _census(s["src"], s["tgt"], G, res, tw.DIRECT27)
            assert 0 < n1 < n7 < n27, (res, g)
            Gd = np.eye(4) if G is None else G.astype(np.float64)
            own = tw.cells(tw.transform(Gd[:3, :3], Gd[:3, 3], a), res)[pi]
            last = int(np.all(found - own == (0, 0, -1), axis=1).sum())
            print(f"res {res} guess {g}: {n1} / {n7} / {n27} pairs, {last} through DIRECT7's last offset")
            through_last += last > 0
    assert through_last >= 6


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [tw.DIRECT1, tw.DIRECT7, tw.DIRECT27])
def test_gpu_census_sweep(gpu_ctx, mode):
    """max_iterations = 1: n_correspondences is the count of the linearisation at the guess, equal to the
    twin's census; the one-step pose within the bar of the twin's."""
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    s = _sweep_scene()
    if "CA" not in s:
        s["CA"], s["CB"] = _dev_covs(gpu_ctx, s["src"]), _dev_covs(gpu_ctx, s["tgt"])
    for res in SWEEP_RES:
        for g, G in s["guess"].items():
            p = vgicp.default_params(k_correspondences=K, neighbor_search=mode, voxel_resolution=res, max_iterations=1)
            r, _ = vgicp.align(s["src"], s["tgt"], p, guess=G, ctx=gpu_ctx)
            want, _, _ = _census(s["src"], s["tgt"], G, res, mode)
            assert r.status == 0 and r.n_correspondences == want and want > 0, (res, g, r.n_correspondences, want)
            o = _twin(s["src"], s["tgt"], s["CA"], s["CB"], p, G)
            assert o["n_valid"] == want
            _hold_result("B1", f"mode {mode} res {res} guess {g}", r, o, s["src"], s["tgt"])


# ---- faces: DIRECT1, resolution 0.5, identity rotation and a translation that is a float, so Ta is exact
FACE_RES = 0.5


def _face_targets():
    """8 points in cell (0, 0, 0) and 8 in (-1, 0, 0) of resolution 0.5: both, the first alone, the second
    alone (which voxel a point found shows in the three counts)."""
    rng = np.random.default_rng(21)
    c0 = rng.uniform(0.05, 0.45, (8, 3)).astype(np.float32)
    cm = c0.copy()
    cm[:, 0] = -c0[:, 0]
    return {"both": np.concatenate([c0, cm]), "cell_0": c0, "cell_m1": cm}


def _face_guess(t):
    G = np.eye(4, dtype=np.float32)
    G[:3, 3] = t
    return G


# name -> (source point, translation, Ta.x, its cell, the counts against both / cell 0 / cell -1).  y and z
# land on 0.25, inside cell 0.  Ta.x = x + t.x exactly (a sum of two floats of like magnitude, in double).
#   on_face_0          Ta.x =  0.0: floor( 0.0 / 0.5) =  0          -> cell  0: found in both and in cell_0
#   minus_zero         Ta.x = -0.0: floor(-0.0 / 0.5) = -0.0        -> cell  0 (-0.0 converts to 0)
#                      (-0.0 survives Ta = ((1 * -0.0 + 0 * -0.25) + 0 * -0.25) + -0.0: every term is -0.0)
#   below_face_0       Ta.x = -2^-20: floor(-2^-19) = -1            -> cell -1: found in both and in cell_m1
#                      (truncation would give cell 0)
#   below_face_1       Ta.x = 0.5 - 2^-24: floor(1 - 2^-23) = 0     -> cell  0
#   on_face_1          Ta.x = 0.5: floor(1.0) = 1                   -> cell  1: found nowhere
#   on_face_m1         Ta.x = -0.5: floor(-1.0) = -1                -> cell -1
#   below_face_m1      Ta.x = -0.5 - 2^-20: floor(-1 - 2^-19) = -2  -> cell -2: found nowhere
#                      (truncation would give cell -1)
FACE_CASES = {
    "on_face_0": ((0.25, 0.5, 0.5), (-0.25, -0.25, -0.25), 0.0, 0, (1, 1, 0)),
    "minus_zero": ((-0.0, -0.25, -0.25), (-0.0, 0.5, 0.5), -0.0, 0, (1, 1, 0)),
    "below_face_0": ((0.25 - 2.0 ** -20, 0.5, 0.5), (-0.25, -0.25, -0.25), -(2.0 ** -20), -1, (1, 0, 1)),
    "below_face_1": ((0.75 - 2.0 ** -24, 0.5, 0.5), (-0.25, -0.25, -0.25), 0.5 - 2.0 ** -24, 0, (1, 1, 0)),
    "on_face_1": ((0.75, 0.5, 0.5), (-0.25, -0.25, -0.25), 0.5, 1, (0, 0, 0)),
    "on_face_m1": ((-0.25, 0.5, 0.5), (-0.25, -0.25, -0.25), -0.5, -1, (1, 0, 1)),
    "below_face_m1": ((-0.25 - 2.0 ** -20, 0.5, 0.5), (-0.25, -0.25, -0.25), -0.5 - 2.0 ** -20, -2, (0, 0, 0)),
}


@pytest.mark.parametrize("name", sorted(FACE_CASES))
def test_twin_census_faces(name):
    """The crafted points are exact: the source and Ta are representable, Ta.x is the stated value (sign of
    zero included) in the stated cell, and the twin's census gives the hand-derived counts."""
    pt, t, tax, cell, counts = FACE_CASES[name]
    src = np.array([pt], np.float32)
    assert np.array_equal(src.astype(np.float64), np.array([pt]))  # the point is a float
    G = _face_guess(t)
    ta = tw.transform(G[:3, :3].astype(np.float64), G[:3, 3].astype(np.float64), src.astype(np.float64))
    assert ta[0, 0] == tax and np.signbit(ta[0, 0]) == np.signbit(tax) and ta[0, 1] == 0.25 and ta[0, 2] == 0.25
    assert int(tw.cells(ta, FACE_RES)[0, 0]) == cell and tuple(tw.cells(ta, FACE_RES)[0, 1:]) == (0, 0)
    targets = _face_targets()
    assert len(tw.voxel_map(targets["both"], np.broadcast_to(np.eye(3), (16, 3, 3)), FACE_RES).coords) == 2
    for which, want in zip(("both", "cell_0", "cell_m1"), counts):
        assert _census(src, targets[which], G, FACE_RES, tw.DIRECT1)[0] == want, which


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FACE_CASES))
def test_gpu_census_faces(gpu_ctx, name):
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    pt, t, _, _, counts = FACE_CASES[name]
    src = np.array([pt], np.float32)
    G = _face_guess(t)
    p = vgicp.default_params(k_correspondences=K, voxel_resolution=FACE_RES, max_iterations=1)
    targets = _face_targets()
    for which, want in zip(("both", "cell_0", "cell_m1"), counts):
        r, _ = vgicp.align(src, targets[which], p, guess=G, ctx=gpu_ctx)
        assert r.status == 0 and np.isfinite(r.matrix()).all(), which
        assert r.n_correspondences == _census(src, targets[which], G, FACE_RES, tw.DIRECT1)[0] == want, (which, r.n_correspondences)


# ---- the key range's edge and the carry between the key's fields: resolution 1.0, counts only (floats
# are 1/16 apart at 2^20: too coarse a scene for a pose bar)
EDGE = 2 ** 20


def _cell_points(cell, n, seed):
    """n float points inside the unit cell `cell`, on the 1/16 grid floats have at 2^20."""
    rng = np.random.default_rng(seed)
    pts = (np.array(cell, np.float64) + rng.integers(1, 15, (n, 3)) / 16.0).astype(np.float32)
    assert np.array_equal(np.floor(pts.astype(np.float64)), np.broadcast_to(np.array(cell, np.float64), (n, 3)))
    return pts


def _edge_scene(name):
    """-> source, target, {mode: the hand-derived count}."""
    if name == "x_edge":
        # voxels A = (2^20 - 1, 0, 0), B = (2^20 - 2, 0, 0), C = (2^20 - 1, 1, 0), D = (2^20 - 2, 1, 0); 4 source
        # points in A.  DIRECT7 finds A, B (-x) and C (+y): 3 each; DIRECT27 also D: 4 each.  The +x
        # neighbours (cell 2^20) lie outside the key range and do not exist.
        cellsv = [(EDGE - 1, 0, 0), (EDGE - 2, 0, 0), (EDGE - 1, 1, 0), (EDGE - 2, 1, 0)]
        tgt = np.concatenate([_cell_points(c, 8, 30 + i) for i, c in enumerate(cellsv)])
        return _cell_points(cellsv[0], 4, 40), tgt, {tw.DIRECT1: 4, tw.DIRECT7: 12, tw.DIRECT27: 16}
    if name == "y_carry":
        # voxels (0, 2^20 - 1, 0) and (1, -2^20, 0); 4 source points in the first.  Its +y neighbour (0, 2^20,
        # 0) is outside the range; an unguarded key of it carries into x and equals the second voxel's.
        # Every mode finds the own cell only: 1 each.
        cellsv = [(0, EDGE - 1, 0), (1, -EDGE, 0)]
    elif name == "z_carry":
        # the same one field down: (0, 0, 2^20 - 1) and (0, 1, -2^20); +z of the first carries into y.
        cellsv = [(0, 0, EDGE - 1), (0, 1, -EDGE)]
    else:
        raise KeyError(name)
    tgt = np.concatenate([_cell_points(c, 8, 50 + i) for i, c in enumerate(cellsv)])
    return _cell_points(cellsv[0], 4, 60), tgt, {tw.DIRECT1: 4, tw.DIRECT7: 4, tw.DIRECT27: 4}


EDGE_SCENES = ("x_edge", "y_carry", "z_carry")


@pytest.mark.parametrize("name", EDGE_SCENES)
def test_twin_census_key_edge(name):
    """The twin's index is a dict of integer triples: no key, no carry.  It gives the hand-derived counts,
    and the aliased neighbour really is what an unguarded, unmasked key would find."""
    src, tgt, want = _edge_scene(name)
    for mode, n in want.items():
        assert _census(src, tgt, None, 1.0, mode)[0] == n, mode
    if name != "x_edge":
        bias, bits = 1 << 20, 21
        key = lambda c: ((c[0] + bias) << (2 * bits)) + ((c[1] + bias) << bits) + (c[2] + bias)  # fields not masked
        vm = tw.voxel_map(tgt, np.broadcast_to(np.eye(3), (len(tgt), 3, 3)), 1.0)
        own, other = tuple(int(v) for v in vm.coords[0]), tuple(int(v) for v in vm.coords[1])
        step = (0, 1, 0) if name == "y_carry" else (0, 0, 1)
        assert key(tuple(o + d for o, d in zip(own, step))) == key(other)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_SCENES)
def test_gpu_census_key_edge(gpu_ctx, name):
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    src, tgt, want = _edge_scene(name)
    for mode, n in want.items():
        p = vgicp.default_params(k_correspondences=K, neighbor_search=mode, max_iterations=1)
        r, _ = vgicp.align(src, tgt, p, ctx=gpu_ctx)
        assert r.status == 0 and np.isfinite(r.matrix()).all(), mode
        assert r.n_correspondences == _census(src, tgt, None, 1.0, mode)[0] == n, (mode, r.n_correspondences)


def _out_of_range_guess():
    G = _near_guess()
    G[0, 3] = np.float32(3e6)
    return G


def test_twin_census_out_of_range():
    src, tgt, _ = _scene(1, 400)
    for mode in (tw.DIRECT1, tw.DIRECT7, tw.DIRECT27):
        assert _census(src, tgt, _out_of_range_guess(), 1.0, mode)[0] == 0
    I = np.broadcast_to(np.eye(3), (400, 3, 3))
    o = tw.align(src, tgt, I, I, mode=tw.DIRECT27, guess=_out_of_range_guess())
    assert o["n_valid"] == 0 and o["converged"] and o["iterations"] == 0


@pytest.mark.gpu
def test_gpu_census_out_of_range(gpu_ctx):
    """A translation of 3e6 takes every Ta outside the key range: no cell is looked up, 0 correspondences,
    converged at iteration 0 at the guess, bit for bit."""
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    src, tgt, _ = _scene(1, 400)
    G = _out_of_range_guess()
    for mode in (tw.DIRECT1, tw.DIRECT7, tw.DIRECT27):
        r, _ = vgicp.align(src, tgt, vgicp.default_params(k_correspondences=K, neighbor_search=mode), guess=G, ctx=gpu_ctx)
        assert r.status == 0 and r.n_correspondences == 0 and r.converged and r.iterations == 0, mode
        np.testing.assert_array_equal(r.matrix(), G)


# =============================================================================== C. batches
NPAIRS = 300
BAD = {0: "empty_target", 255: "nan_in_source", 256: "target_at_2^21", 299: "inf_in_target"}
TWIN_PAIRS = (1, 60, 127, 128, 200, 254, 257, 298)
_batch = {}


def _batch_pairs():
    """300 ragged pairs: prefixes of ten scenes, 40 to 200 source and 64 to 260 target points, the guesses
    none, near and far in turn; four bad pairs."""
    if not _batch:
        scenes = [_scene(s, 260) for s in range(10)]
        pairs, guesses = [], []
        for i in range(NPAIRS):
            src, tgt, _ = scenes[i % 10]
            src = src[:40 + (i * 37) % 161].copy()
            tgt = tgt[:64 + (i * 53) % 197].copy()
            if i == 0:
                tgt = tgt[:0]
            elif i == 255:
                src[17, 2] = np.nan
            elif i == 256:
                tgt[3, 0] = np.float32(2.0 ** 21)
            elif i == 299:
                tgt[5, 1] = np.inf
            pairs.append((src, tgt))
            guesses.append((np.eye(4, dtype=np.float32), _near_guess(), _far_guess())[i % 3])
        _batch["pairs"], _batch["guesses"] = pairs, guesses
    return _batch["pairs"], _batch["guesses"]


def _batch_params(vgicp):
    return vgicp.default_params(k_correspondences=K, neighbor_search=vgicp.DIRECT7)


def _batch_singles(ctx):
    """Every healthy pair's single vgicp.align, once."""
    if "singles" not in _batch:
        vgicp = _vgicp()
        pairs, guesses = _batch_pairs()
        p = _batch_params(vgicp)
        _batch["singles"] = {i: vgicp.align(pairs[i][0], pairs[i][1], p, guess=guesses[i], want_aligned=True, ctx=ctx)
                             for i in range(NPAIRS) if i not in BAD}
    return _batch["singles"]


def _assert_row_is_single(row, al, single, what):
    r, a1 = single
    np.testing.assert_array_equal(row["T"], np.array(r.T, np.float32), err_msg=what)
    assert row["status"] == r.status == 0, what
    assert row["iterations"] == r.iterations and row["converged"] == r.converged, what
    assert row["fitness"] == r.fitness and row["n_correspondences"] == r.n_correspondences, what
    np.testing.assert_array_equal(al[:, :3], a1[:, :3], err_msg=what)


def test_batch_pairs_shape():
    pairs, guesses = _batch_pairs()
    sn = [len(p[0]) for p in pairs]
    tn = [len(p[1]) for i, p in enumerate(pairs) if i != 0]
    assert min(sn) == 40 and max(sn) == 200 and min(tn) >= 64 and max(tn) == 260 and len(set(zip(sn, tn))) > 100
    for n, bits in ((2, 1), (256, 8), (257, 9), (300, 9)):  # the radix passes over the pair word
        b = 1
        while (1 << b) < n:
            b += 1
        assert b == bits


@pytest.mark.gpu
@pytest.mark.parametrize("npairs", [2, 256, 257, 300])
def test_gpu_batch_prefixes_of_300_pairs(gpu_ctx, npairs):
    """The map sort's third key, the pair, takes 1, 8, 9 and 9 bits: one radix pass, one full pass, two.
    Every healthy row and aligned cloud is bit-identical to its single call; bad rows carry their status
    and leave `aligned` untouched; the guards are intact (_run_batch asserts them)."""
    import icp4r

    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    pairs, guesses = _batch_pairs()
    singles = _batch_singles(gpu_ctx)
    rows, al = _run_batch(gpu_ctx, vgicp, pairs[:npairs], guesses[:npairs], _batch_params(vgicp))
    status = {"empty_target": icp4r.E_EMPTY, "nan_in_source": icp4r.E_NONFINITE, "target_at_2^21": icp4r.E_INVALID,
              "inf_in_target": icp4r.E_NONFINITE}
    for i in range(npairs):
        if i in BAD:
            assert rows[i]["status"] == status[BAD[i]], (i, BAD[i], rows[i]["status"])
            assert not rows[i]["converged"] and (al[i] == -7.5).all(), (i, BAD[i])
        else:
            _assert_row_is_single(rows[i], al[i], singles[i], f"pair {i} of {npairs}")
    if npairs == NPAIRS:
        assert len(set(rows["iterations"].tolist())) >= 4
        for i in TWIN_PAIRS:
            src, tgt = pairs[i]
            o = _twin(src, tgt, _dev_covs(gpu_ctx, src), _dev_covs(gpu_ctx, tgt), _batch_params(vgicp), guesses[i])
            _hold("C", f"pair {i}", rows[i]["T"].reshape(4, 4).T, rows[i]["iterations"], rows[i]["converged"],
                  rows[i]["n_correspondences"], rows[i]["fitness"], o, src, tgt)


WIDE_N, WIDE_M, WIDE_PAIRS = 17000, 9000, 6
WIDE_GRIDS = (1, 7, 42, 120, None)   # gicp_grid; None: the default
DEFAULT_GRID = 2048                  # kGicpGrid of csrc/icp4r_internal.hpp


def _slices(n):
    """gicp_slices(n) of csrc/icp4r_gicp_dev.hpp: slices of 256 points, of more once there would be over 64."""
    pts = 256 * max(1, -(-n // (256 * 64)))
    return max(1, -(-n // pts))


def _workgroups_per_pair(grid, npairs, max_n):
    """W of gicp_iter_grid: grid / npairs, at least 1, at most the slices of the largest source."""
    return min(max((DEFAULT_GRID if grid is None else grid) // npairs, 1), _slices(max_n))


def test_wide_pair_grids_give_distinct_workgroup_counts():
    """The grids of test_gpu_batch_one_wide_pair on its 6 pairs: W = 1 (twice: 7 / 6 = 1), 7 and 20, both
    strictly between 1 and the wide pair's 34 slices, and 34.  With W = 7 the wide pair's workgroups stride
    over 5 or 4 slices each; with W = 20 some take two slices and some one."""
    assert _slices(WIDE_N) == 34 and _slices(200) == 1 and _slices(16384) == 64 and _slices(16385) == 33
    W = [_workgroups_per_pair(g, WIDE_PAIRS, WIDE_N) for g in WIDE_GRIDS]
    assert W == [1, 1, 7, 20, 34]
    assert sum(1 < w < _slices(WIDE_N) for w in W) == 2


@pytest.mark.gpu
def test_gpu_batch_one_wide_pair(gpu_ctx, plan):
    """A 17000-point source (34 slices of 512) with a 9000-point target at index 2 among five small pairs of
    one slice each: t_stride makes the small pairs' sort segments almost all padding keys.  gicp_grid 1, 7,
    42, 120 and the default give W = 1, 1, 7, 20 and 34 workgroups per pair (the test above): at 7 and 20 the
    wide pair's workgroups stride over several slices (q += W) while the small pairs' spare workgroups
    return at j >= ns.  Every run is bit-identical to the singles."""
    vgicp = _vgicp()
    src, tgt, _ = _scene(9, WIDE_N)
    small, guesses = _batch_pairs()
    pairs = [small[1], small[2], (src, np.ascontiguousarray(tgt[:WIDE_M])), small[3], small[4], small[5]]
    gs = [guesses[1], guesses[2], np.eye(4, dtype=np.float32), guesses[3], guesses[4], guesses[5]]
    assert len(pairs) == WIDE_PAIRS and max(len(a) for a, _ in pairs) == WIDE_N
    p = _batch_params(vgicp)
    gpu_ctx.reset_plan_options()
    singles = [vgicp.align(a, b, p, guess=g, want_aligned=True, ctx=gpu_ctx) for (a, b), g in zip(pairs, gs)]
    assert singles[2][0].n_correspondences > 0 and singles[2][0].iterations > 0
    for grid in WIDE_GRIDS:
        gpu_ctx.reset_plan_options()
        if grid is not None:
            plan(gicp_grid=grid)
        rows, al = _run_batch(gpu_ctx, vgicp, pairs, gs, p)
        for i in range(WIDE_PAIRS):
            _assert_row_is_single(rows[i], al[i], singles[i], f"grid {grid} pair {i}")


@pytest.mark.gpu
def test_gpu_status_order_nonfinite_before_range(gpu_ctx):
    """A NaN in the target, an inf in the target, and a target with both a NaN and a coordinate outside the
    key range: ICP4R_E_NONFINITE, single and batched.  The stage that decides is the registration's begin
    (the validation every GICP pair gets before its covariances); the map's key kernel skips a pair that is
    already invalid, so its range flag is never raised and ICP4R_E_INVALID never replaces the status."""
    import icp4r

    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    src, tgt, _ = _scene(2, 300)
    nan_t, inf_t, both = tgt.copy(), tgt.copy(), tgt.copy()
    nan_t[7, 1] = np.nan
    inf_t[9, 2] = -np.inf
    both[3, 0] = np.float32(2.0 ** 21)
    both[200, 2] = np.nan
    far = tgt.copy()
    far[3, 0] = np.float32(2.0 ** 21)
    p = _batch_params(vgicp)
    targets = [nan_t, tgt, inf_t, both, far]
    want = [icp4r.E_NONFINITE, 0, icp4r.E_NONFINITE, icp4r.E_NONFINITE, icp4r.E_INVALID]
    for t, w in zip(targets, want):
        r, _ = vgicp.align(src, t, p, ctx=gpu_ctx)
        assert r.status == w and (w == 0 or not r.converged), (r.status, w)
    rows, al = _run_batch(gpu_ctx, vgicp, [(src, t) for t in targets], [np.eye(4, dtype=np.float32)] * 5, p)
    assert rows["status"].tolist() == want
    for i, w in enumerate(want):
        assert (w == 0) != bool((al[i] == -7.5).all()), i
    _assert_row_is_single(rows[1], al[1], vgicp.align(src, tgt, p, want_aligned=True, ctx=gpu_ctx), "the healthy pair")


# =============================================================================== D. options, tiny clouds, reuse
_far = {}


def _far_scene(ctx):
    if not _far:
        src, tgt, _ = _scene(0, 2048)
        _far["src"], _far["tgt"] = np.ascontiguousarray(src[:1500]), tgt
        _far["CA"], _far["CB"] = _dev_covs(ctx, _far["src"]), _dev_covs(ctx, tgt)
    return _far["src"], _far["tgt"], _far["CA"], _far["CB"]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [2, 3, 4, 5, 6, 7])
def test_gpu_iteration_caps_match_twin(gpu_ctx, cap):
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    src, tgt, CA, CB = _far_scene(gpu_ctx)
    p = vgicp.default_params(k_correspondences=K, neighbor_search=vgicp.DIRECT7, max_iterations=cap)
    o = _twin(src, tgt, CA, CB, p, _far_guess())
    assert o["iterations"] == cap - 1 and not o["converged"] and not o["lm_failed"]  # the cap cuts the run short
    r, _ = vgicp.align(src, tgt, p, guess=_far_guess(), ctx=gpu_ctx)
    _hold_result("D", f"cap {cap}", r, o, src, tgt)


# (rotation_epsilon, transformation_epsilon, max_iterations) -> the twin's (iterations, converged): DIRECT1,
# seed 0, the far guess
EPSILONS = {(0.1, 0.1, 64): (4, True), (1e-6, 1e-7, 64): (42, True), (2e-3, 1e-9, 20): (19, False)}


def test_twin_epsilons_decide(oracle_mod):
    src, tgt, _ = _scene(0, 2048)
    src = np.ascontiguousarray(src[:1500])
    CA = oracle_mod.gicp_covariances(src, K, oracle_mod.GICP_REG_PLANE)
    CB = oracle_mod.gicp_covariances(tgt, K, oracle_mod.GICP_REG_PLANE)
    for (re_, te, cap), want in EPSILONS.items():
        o = tw.align(src, tgt, CA, CB, guess=_far_guess(), rotation_epsilon=re_, transformation_epsilon=te, max_iterations=cap)
        assert (o["iterations"], o["converged"]) == want and not o["lm_failed"], (re_, te)


@pytest.mark.gpu
@pytest.mark.parametrize("eps", sorted(EPSILONS))
def test_gpu_epsilons_match_twin(gpu_ctx, eps):
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    src, tgt, CA, CB = _far_scene(gpu_ctx)
    p = vgicp.default_params(k_correspondences=K, rotation_epsilon=eps[0], transformation_epsilon=eps[1], max_iterations=eps[2])
    o = _twin(src, tgt, CA, CB, p, _far_guess())
    assert (o["iterations"], o["converged"]) == EPSILONS[eps]
    r, _ = vgicp.align(src, tgt, p, guess=_far_guess(), ctx=gpu_ctx)
    _hold_result("D", f"epsilons {eps}", r, o, src, tgt)


# target points -> the twin's (iterations, n_valid) on _scene(0, 300), DIRECT27, k = 5: it converges every time.
# Up to 4 points every voxel is found once; the 5-point target has two voxels in reach of two source points
# (7 pairs) and takes a third iteration.
TINY = {1: (2, 1), 3: (2, 3), 4: (1, 4), 5: (3, 7)}


def _tiny_clouds(m):
    src, tgt, _ = _scene(0, 300)
    return src, np.ascontiguousarray(tgt[:m])


def _tiny_holds(o, m):
    assert o["converged"] and not o["lm_failed"] and len(o["map"].coords) == m
    assert (o["iterations"], o["n_valid"]) == TINY[m], (o["iterations"], o["n_valid"])


@pytest.mark.parametrize("m", sorted(TINY))
def test_twin_tiny_targets(oracle_mod, m):
    src, tgt = _tiny_clouds(m)
    CA = oracle_mod.gicp_covariances(src, K, oracle_mod.GICP_REG_PLANE)
    CB = oracle_mod.gicp_covariances(tgt, K, oracle_mod.GICP_REG_PLANE)
    _tiny_holds(tw.align(src, tgt, CA, CB, resolution=1.0, mode=tw.DIRECT27), m)


@pytest.mark.gpu
@pytest.mark.parametrize("m", sorted(TINY))
def test_gpu_tiny_targets_match_twin(gpu_ctx, m):
    """Targets of fewer than k points, and of k: the covariances' n < k rule on the target side, voxels of
    one point."""
    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    src, tgt = _tiny_clouds(m)
    p = vgicp.default_params(k_correspondences=K, neighbor_search=vgicp.DIRECT27)
    o = _twin(src, tgt, _dev_covs(gpu_ctx, src), _dev_covs(gpu_ctx, tgt), p, None)
    _tiny_holds(o, m)
    r, _ = vgicp.align(src, tgt, p, ctx=gpu_ctx)
    _hold_result("D", f"target of {m}", r, o, src, tgt)


@pytest.mark.gpu
def test_gpu_workspace_reuse_across_sizes_and_modes(gpu_ctx):
    """A large DIRECT27 align, a small DIRECT1 align, voxel_map, a GICP align and the first again on the
    session's context (whose work areas earlier tests sized) equal, bit for bit, the same calls on a fresh
    context that meets them in the opposite order.  The opposite order is deliberate: with one fresh context
    for all four calls, only the first call made on it meets untouched work areas, and the same order on
    both contexts would give both the same history; reversed, every call's history differs between the two
    (the small align, voxel_map and the GICP align come before anything larger on the fresh one)."""
    import icp4r
    from icp4r import gicp

    vgicp = _vgicp()
    gpu_ctx.reset_plan_options()
    big_s, big_t, _ = _scene(4, 6000)
    small_s, small_t, _ = _scene(5, 90)
    pts = np.ascontiguousarray(big_t[:700])

    def calls(ctx):
        return [
            lambda: _tuple(*vgicp.align(big_s, big_t, vgicp.default_params(k_correspondences=K, neighbor_search=vgicp.DIRECT27,
                                                                         voxel_resolution=0.5),
                                        guess=_near_guess(), want_aligned=True, ctx=ctx)),
            lambda: _tuple(*vgicp.align(small_s, small_t, vgicp.default_params(k_correspondences=K), want_aligned=True, ctx=ctx)),
            lambda: tuple(a.tobytes() for a in vgicp.voxel_map(pts, 0.7, k=K, ctx=ctx)),
            lambda: _tuple(*gicp.align(small_s, big_t, gicp.default_params(k_correspondences=K), want_aligned=True, ctx=ctx)),
        ]

    mine = calls(gpu_ctx)
    got = [mine[i]() for i in (0, 1, 2, 3, 0)]
    fresh = icp4r.Context(0)
    try:
        theirs = calls(fresh)
        want = {i: theirs[i]() for i in (3, 2, 1, 0)}
    finally:
        fresh.close()
    for j, i in enumerate((0, 1, 2, 3, 0)):
        assert got[j] == want[i], f"call {j}"
    assert got[0][5] == 0 and got[1][5] == 0 and got[3][5] == 0


# ---- icp4r_vgicp_voxel_map's arguments through the raw entry
def _raw_map(ctx, buf, n, stride, cov9, res, cap, outs, k=K):
    """outs: which of coords, num, mean, cov get a buffer (the others NULL) -> rc, n_voxels, the buffers."""
    import icp4r

    vgicp = _vgicp()
    room = max(cap, 1)
    bufs = {"coords": np.full((room, 3), 777, np.int32), "num": np.full(room, 777, np.int32),
            "mean": np.full((room, 3), 777.0), "cov": np.full((room, 3, 3), 777.0)}
    ptr = lambda name: icp4r._ptr(bufs[name]) if name in outs else None
    nv = C.c_int32(-1)
    rc = vgicp._lib().icp4r_vgicp_voxel_map(ctx.handle, icp4r._ptr(buf), n, stride, icp4r._ptr(cov9) if cov9 is not None else None,
                                            k, 3, float(res), cap, ptr("coords"), ptr("num"), ptr("mean"), ptr("cov"),
                                            C.byref(nv))
    return rc, nv.value, bufs


@pytest.mark.gpu
def test_gpu_voxel_map_raw_arguments(gpu_ctx):
    import icp4r

    gpu_ctx.reset_plan_options()
    src, _, _ = _scene(3, 400)
    n = len(src)
    Cv = _dev_covs(gpu_ctx, src)
    c9 = np.ascontiguousarray(Cv.reshape(n, 9))
    vm = tw.voxel_map(src, Cv, 1.0)
    V = len(vm.coords)
    names = ("coords", "num", "mean", "cov")
    want = {"coords": vm.coords, "num": vm.num, "mean": vm.mean, "cov": vm.cov}
    # records of 20 and 32 bytes: the floats after z are not read
    for floats in (5, 8):
        rec = np.full((n, floats), 9.5, np.float32)
        rec[:, :3] = src
        rc, nv, bufs = _raw_map(gpu_ctx, rec, n, 4 * floats, c9, 1.0, n, names)
        assert rc == 0 and nv == V
        for name in names:
            np.testing.assert_array_equal(bufs[name][:V], want[name], err_msg=f"{name} stride {4 * floats}")
            assert (bufs[name][V:] == 777).all()
        # the k-NN covariances (cov_in = NULL) read the same records
        rc, nv, bufs = _raw_map(gpu_ctx, rec, n, 4 * floats, None, 1.0, n, names)
        assert rc == 0 and nv == V
        np.testing.assert_array_equal(bufs["cov"][:V], vm.cov)
    # every output NULL in turn, then all: the others are written, *n_voxels is set
    for leave in names + (None,):
        outs = tuple(x for x in names if x != leave) if leave else ()
        rc, nv, bufs = _raw_map(gpu_ctx, src, n, 12, c9, 1.0, n, outs)
        assert rc == 0 and nv == V, leave
        for name in names:
            if name in outs:
                np.testing.assert_array_equal(bufs[name][:V], want[name], err_msg=f"{name} without {leave}")
            else:
                assert (bufs[name] == 777).all()
    # no point, one point, no room
    rc, nv, bufs = _raw_map(gpu_ctx, src, 0, 12, c9, 1.0, 4, names)
    assert rc == 0 and nv == 0 and all((bufs[x] == 777).all() for x in names)
    rc, nv, bufs = _raw_map(gpu_ctx, src, 0, 12, c9, 1.0, 0, names)
    assert rc == 0 and nv == 0
    rc, nv, bufs = _raw_map(gpu_ctx, src, 1, 12, c9, 1.0, 1, names)
    one = tw.voxel_map(src[:1], Cv[:1], 1.0)
    assert rc == 0 and nv == 1
    np.testing.assert_array_equal(bufs["coords"][:1], one.coords)
    np.testing.assert_array_equal(bufs["mean"][:1], src[:1].astype(np.float64))
    np.testing.assert_array_equal(bufs["cov"][:1], one.cov)
    assert bufs["num"][0] == 1
    rc, nv, bufs = _raw_map(gpu_ctx, src, n, 12, c9, 1.0, 0, names)
    assert rc == icp4r.E_INVALID and nv == V and all((bufs[x] == 777).all() for x in names)


@pytest.mark.gpu
def test_gpu_voxel_map_5000_points_in_one_voxel(gpu_ctx):
    """One lane adds a run of 5000 points sequentially: mean and cov bit-equal to the twin's sequential sum
    (a pairwise or a blocked sum of the covariances would differ in the last bits)."""
    from test_vgicp import random_spd

    vgicp = _vgicp()
    rng = np.random.default_rng(77)
    pts = rng.uniform(0.001, 0.999, (5000, 3)).astype(np.float32)
    Cv = random_spd(rng, 5000)
    vm = tw.voxel_map(pts, Cv, 1.0)
    assert len(vm.coords) == 1 and vm.num[0] == 5000
    # (the mean's sum of floats is exact in double in any order; the covariances' sum is not)
    halves = Cv.reshape(2, 2500, 3, 3).sum(1).sum(0) / 5000.0
    assert not np.array_equal(halves, vm.cov[0])  # another order is visible in the bits
    coords, num, mean, cov = vgicp.voxel_map(pts, 1.0, cov=Cv, ctx=gpu_ctx)
    np.testing.assert_array_equal(coords, vm.coords)
    np.testing.assert_array_equal(num, vm.num)
    np.testing.assert_array_equal(mean, vm.mean)
    np.testing.assert_array_equal(cov, vm.cov)
