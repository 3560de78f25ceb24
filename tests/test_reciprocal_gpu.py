"""Reciprocal correspondences on the device (icp4r_params.use_reciprocal_correspondences) against the numpy
twin tests/reciprocal_twin.py.  "Equal" below: status, iterations, converged, convergence_state and
n_correspondences equal; T and fitness equal in bits; the aligned xyz equal in bits where asked for."""
import functools

import numpy as np
import pytest

import reciprocal_twin as rt
from helpers import pose_err

pytestmark = pytest.mark.gpu

SHAPES = [(4000, 700, 650), (4001, 1024, 1024), (4002, 600, 900), (4003, 2048, 1500), (4004, 900, 2048),
          (4300, 700, 9000)]  # solo-sized, one-tile, n < m, n > m, and the two-tile target
PARAMS = [{}, {"max_iterations": 7}, {"max_correspondence_distance": 1.0}]


@functools.lru_cache(maxsize=None)
def _pair(seed, n, m):
    from icp4r import synth

    p = synth.make_pair(seed, n, m)
    return p.src_xyzi(), p.tgt_xyzi()


@functools.lru_cache(maxsize=None)
def _twin(seed, n, m, kw=()):
    s, t = _pair(seed, n, m)
    return rt.icp(s, t, **dict(kw))


def _params(**kw):
    import icp4r

    return icp4r.default_params(use_reciprocal_correspondences=1, **kw)


def _row(r):
    """An icp4r.Result or a RESULT_DTYPE row as a dict with a row-major T."""
    if isinstance(r, np.void):
        d = {k: r[k].item() for k in ("fitness", "iterations", "converged", "status", "convergence_state",
                                      "n_correspondences")}
        d["T"] = r["T"].reshape(4, 4).T.copy()
        return d
    return {"T": r.matrix(), "fitness": r.fitness, "iterations": r.iterations, "converged": r.converged,
            "status": r.status, "convergence_state": r.convergence_state, "n_correspondences": r.n_correspondences}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_equal_twin(r, o, aligned=None, what=""):
    d = _row(r)
    got = (d["status"], d["iterations"], bool(d["converged"]), d["convergence_state"], d["n_correspondences"])
    want = (o["status"], o["iterations"], bool(o["converged"]), o["state"], o["n_correspondences"])
    assert got == want, (what, got, want, o["ncorr"])
    assert (_bits(d["T"]) == _bits(o["T"])).all(), (what, np.abs(d["T"] - o["T"]).max())
    assert np.float64(d["fitness"]).view(np.uint64) == np.float64(o["fitness"]).view(np.uint64), (what, d["fitness"], o["fitness"])
    if aligned is not None:
        assert (_bits(aligned[:, :3]) == _bits(o["aligned"])).all(), what


def assert_same_rows(a, b, what=""):
    a, b = _row(a), _row(b)
    for k in ("status", "iterations", "converged", "convergence_state", "n_correspondences"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert (_bits(a["T"]) == _bits(b["T"])).all(), what
    assert np.float64(a["fitness"]).view(np.uint64) == np.float64(b["fitness"]).view(np.uint64), what


def _batch(ctx, pairs, params):
    srcs = [s for s, _ in pairs]
    tgts = [t for _, t in pairs]
    sn = np.array([len(a) for a in srcs], np.int32)
    tn = np.array([len(a) for a in tgts], np.int32)
    so = (np.cumsum(sn) - sn).astype(np.int64)
    to = (np.cumsum(tn) - tn).astype(np.int64)
    return ctx.align_batch_host(np.concatenate(srcs), so, sn, np.concatenate(tgts), to, tn, params)


# ---- 1. single pairs

@pytest.mark.parametrize("kw", PARAMS, ids=["defaults", "iters7", "maxdist1"])
@pytest.mark.parametrize("seed,n,m", SHAPES)
def test_single_pair_equals_twin(gpu_ctx, seed, n, m, kw):
    s, t = _pair(seed, n, m)
    o = _twin(seed, n, m, tuple(sorted(kw.items())))
    assert sum(o["rejected"]) > 0  # the flag matters on this input
    r, out = gpu_ctx.align(s, t, _params(**kw), want_aligned=True)
    assert_equal_twin(r, o, out, (seed, n, m, kw))
    assert (out[:, 3] == s[:, 3]).all()


def test_a_pair_stops_on_the_identity_criterion():
    """Seed 4002 ends on convergence state 2 (an exactly-identity increment) before the iteration limit:
    the single-pair case above covers the early stop with a rejecting list."""
    o = _twin(4002, 600, 900)
    assert o["state"] == 2 and o["iterations"] < 10


# ---- 2. the batched plan

BATCH_UNIQUE = 32


@functools.lru_cache(maxsize=None)
def _batch_pairs():
    from icp4r import synth

    rng = np.random.default_rng(7)
    out = []
    for u in range(BATCH_UNIQUE):
        n, m = int(rng.integers(300, 701)), int(rng.integers(300, 701))
        p = synth.make_pair(4400 + u, n, m)
        out.append((p.src_xyzi(), p.tgt_xyzi()))
    return out


@functools.lru_cache(maxsize=None)
def _batch_twins():
    return [rt.icp(s, t, max_iterations=6) for s, t in _batch_pairs()]


@pytest.mark.parametrize("npairs", [256, 320])  # two pair groups of 128 / 160; at most and more than one pair per CU
def test_batched_plan_equals_twin(gpu_ctx, plan, npairs):
    import icp4r

    uniq, tw = _batch_pairs(), _batch_twins()
    pairs = [uniq[i % BATCH_UNIQUE] for i in range(npairs)]
    pl = icp4r.plan(npairs, 700, 700, ctx=gpu_ctx)
    assert pl["lds"] and gpu_ctx.get_plan_option("groups")[0] == 2
    res = _batch(gpu_ctx, pairs, _params(max_iterations=6))
    assert sum(sum(o["rejected"]) > 0 for o in tw) == BATCH_UNIQUE
    for i in range(npairs):
        assert_equal_twin(res[i], tw[i % BATCH_UNIQUE], None, i)


# ---- 3. plan options cannot change a reciprocal result

OPTIONS = [{"solo": 0}, {"solo": 1}, {"fuse_test": 0}, {"lazy_x": 0}, {"res_update": 1}, {"held_update": 0},
           {"wide_update": 0}, {"fold_keys": 0}, {"nn_tile": 0}, {"groups": 1}, {"groups": 3}, {"nn_lds": 0},
           {"nn_lds": 1}, {"nn_cache": 0}, {"tile_own": 0}, {"tile_defer": 0}, {"fuse_seed": 0}, {"sums_tail": 1}]


@pytest.mark.parametrize("seed,n,m", [(4000, 700, 650), (4003, 2048, 1500), (4300, 700, 9000)])
def test_plan_options_keep_single_pair_bits(gpu_ctx, plan, seed, n, m):
    import icp4r

    s, t = _pair(seed, n, m)
    ref, ref_out = gpu_ctx.align(s, t, _params(), want_aligned=True)
    assert_equal_twin(ref, _twin(seed, n, m), ref_out)
    for o in OPTIONS:
        gpu_ctx.reset_plan_options()
        plan(**o)
        r, out = gpu_ctx.align(s, t, _params(), want_aligned=True)
        assert_same_rows(r, ref, o)
        assert (_bits(out) == _bits(ref_out)).all(), o
    gpu_ctx.reset_plan_options()
    if m <= 2048:  # brute force: every target against every query
        for mode in (icp4r.NN_BRUTE, icp4r.NN_BRUTE_PACKED, icp4r.NN_PRUNED):
            r, out = gpu_ctx.align(s, t, _params(nn_mode=mode), want_aligned=True)
            assert_same_rows(r, ref, mode)
            assert (_bits(out) == _bits(ref_out)).all(), mode


def test_plan_options_keep_batch_bits(gpu_ctx, plan):
    """groups = 3 runs on 384 pairs (the 256 and their first 128 again): run_pairs lowers `groups` while a
    group would hold fewer than 128 pairs, so on 256 pairs the option never formed three groups.  That
    three groups really run is asserted from the stage's launch count in
    test_reciprocal_params.test_stage_launch_counts[lds-3groups]."""
    import icp4r

    uniq = _batch_pairs()
    pairs = [uniq[i % BATCH_UNIQUE] for i in range(256)]
    ref = _batch(gpu_ctx, pairs, _params(max_iterations=6))
    for o in OPTIONS + [{"nn_mode": icp4r.NN_BRUTE}]:
        gpu_ctx.reset_plan_options()
        kw = {}
        if "nn_mode" in o:
            kw = o
        else:
            plan(**o)
        run = pairs + pairs[:128] if o == {"groups": 3} else pairs
        res = _batch(gpu_ctx, run, _params(max_iterations=6, **kw))
        for i in range(len(run)):
            assert_same_rows(res[i], ref[i % len(pairs)], (o, i))


# ---- 4. tie to the C oracle: a pair on which the reciprocal rule rejects nothing

@functools.lru_cache(maxsize=None)
def _lattice_pair():
    """A jittered 1-m lattice of 12 x 12 x 10 = 1440 targets; the source: 1,000 of them under a 0.1-m,
    0.5-degree motion with 2-cm noise — every source's nearest target is its own lattice point, and
    that target's nearest source is the source again."""
    rng = np.random.default_rng(4500)
    g = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), np.arange(10.0), indexing="ij"), -1).reshape(-1, 3)
    tgt = np.zeros((len(g), 4), np.float32)
    tgt[:, :3] = g + rng.uniform(-0.05, 0.05, g.shape)
    tgt[:, 3] = rng.uniform(0, 30, len(g))
    pick = rng.permutation(len(g))[:1000]
    a = np.deg2rad(0.5)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c = g.mean(0)
    src = np.zeros((1000, 4), np.float32)
    src[:, :3] = (tgt[pick, :3].astype(np.float64) - c) @ R.T + c + np.array([0.06, -0.06, 0.05]) \
        + rng.normal(0, 0.02, (1000, 3))
    src[:, 3] = rng.uniform(0, 30, 1000)
    return src, tgt


def test_nothing_rejected_equals_flag_off_and_the_oracle(gpu_ctx, oracle_mod):
    import icp4r

    s, t = _lattice_pair()
    o = rt.icp(s, t)
    assert o["iterations"] >= 2 and sum(o["rejected"]) == 0 and o["ncorr"] == [1000] * len(o["ncorr"])
    on, on_out = gpu_ctx.align(s, t, _params(), want_aligned=True)
    off, off_out = gpu_ctx.align(s, t, icp4r.default_params(), want_aligned=True)
    assert_same_rows(on, off)
    assert (_bits(on_out) == _bits(off_out)).all()
    assert_equal_twin(on, o, on_out)
    c = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, aligned=True)
    assert (on.matrix() == c["T"]).all() and on.fitness == c["fitness"] and on.iterations == c["iterations"]
    assert on.convergence_state == c["convergence_state"] and (on_out == c["aligned"]).all()
    pairs = [(s, t)] * 3 + [_pair(4000, 700, 650)]
    b_on = _batch(gpu_ctx, pairs, _params())
    b_off = _batch(gpu_ctx, pairs, icp4r.default_params())
    for i in range(3):
        assert_same_rows(b_on[i], b_off[i], i)
        assert_same_rows(b_on[i], on, i)
    assert_equal_twin(b_on[3], _twin(4000, 700, 650))  # ... beside a pair on which it does reject


# ---- 5. edge cases

def _dup_pair():
    s, t = _pair(4100, 400, 300)
    return np.concatenate([s, s[:50]]), np.concatenate([t, t[:40]])


def test_too_few_reciprocal_correspondences(gpu_ctx):
    """Five sources against one target: the target keeps one source, |C| = 1 < 3."""
    import icp4r

    s, t = _pair(4100, 400, 300)
    s, t = s[:5], t[:1]
    o = rt.icp(s, t)
    assert (o["status"], o["state"], o["iterations"], o["ncorr"]) == (-3, 5, 0, [1])
    r, _ = gpu_ctx.align(s, t, _params())
    assert (r.status, r.convergence_state, r.iterations, r.converged) == (icp4r.E_TOO_FEW_CORR, 5, 0, 0)
    assert_equal_twin(r, o)


def test_duplicated_points(gpu_ctx):
    s, t = _dup_pair()
    o = rt.icp(s, t, check_forms=True)
    assert o["rejected"][0] >= 50  # at least the higher-indexed copy of every duplicated source
    r, out = gpu_ctx.align(s, t, _params(), want_aligned=True)
    assert_equal_twin(r, o, out)


@pytest.mark.parametrize("n", [1, 2])
def test_fewer_than_three_sources(gpu_ctx, n):
    s, t = _pair(4100, 400, 300)
    o = rt.icp(s[:n], t)
    assert o["status"] == -3
    r, _ = gpu_ctx.align(s[:n], t, _params())
    assert_equal_twin(r, o)


def test_edge_cases_beside_a_healthy_pair_in_one_batch(gpu_ctx):
    s, t = _pair(4100, 400, 300)
    pairs = [(s[:5], t[:1]), _dup_pair(), (s[:2], t), _pair(4000, 700, 650), (s[:1], t[:1])]
    res = _batch(gpu_ctx, pairs, _params())
    for i, (ps, pt) in enumerate(pairs):
        o = _twin(4000, 700, 650) if i == 3 else rt.icp(ps, pt)
        assert_equal_twin(res[i], o, None, i)
    assert res[3]["status"] == 0 and res[0]["status"] == -3 and res[2]["status"] == -3


# ---- 6. F64 numerics (the tolerances of test_gpu_parity.test_icp_f64_numerics_vs_oracle_f64)

@pytest.mark.parametrize("huber", [np.inf, 0.5])
@pytest.mark.parametrize("seed,n,m", [(4001, 1024, 1024), (4003, 2048, 1500)])
def test_f64_numerics_vs_twin_f64(gpu_ctx, seed, n, m, huber):
    import icp4r

    s, t = _pair(seed, n, m)
    o = rt.icp(s, t, numerics="f64", huber_delta=huber)
    assert sum(o["rejected"]) > 0
    r, _ = gpu_ctx.align(s, t, _params(numerics=icp4r.NUMERICS_F64, huber_delta=huber))
    dt, dr = pose_err(r.matrix(), o["T"])
    print(f"f64 huber={huber}: iterations {r.iterations}/{o['iterations']} ncorr {r.n_correspondences}/"
          f"{o['n_correspondences']} dt {dt:.3e} dr {dr:.3e} fitness {r.fitness!r}/{o['fitness']!r}")
    assert r.status == 0 and r.iterations == o["iterations"]
    assert dt <= 2e-6 and dr <= 2e-6, (dt, dr)
    assert abs(r.fitness - o["fitness"]) <= 1e-6 * o["fitness"]


# ---- 7. the facade and the map registration entry

def test_python_facade(gpu_ctx):
    import icp4r

    s, t = _pair(4002, 600, 900)
    icp = icp4r.IterativeClosestPoint(gpu_ctx)
    icp.setInputSource(s)
    icp.setInputTarget(t)
    icp.setUseReciprocalCorrespondences(True)
    out = icp.align()
    o = _twin(4002, 600, 900)
    assert icp.hasConverged() == o["converged"]
    assert (_bits(icp.getFinalTransformation()) == _bits(o["T"])).all()
    assert icp.getFitnessScore() == o["fitness"]
    assert (_bits(np.asarray(out)[:, :3]) == _bits(o["aligned"])).all()


def test_scan_to_map_registration(gpu_ctx):
    """The map entry: the sector search's device-resident submap as the target of a device batch."""
    import torch

    import icp4r
    from icp4r import synth
    from icp4r.mapstore import KD_TREE

    mp = synth.make_map_pair(3, n_src=1000, scans=7)
    map_pts, scan = mp.tgt_xyzi(), mp.src_xyzi()
    tree = KD_TREE(ctx=gpu_ctx)
    try:
        tree.Build(map_pts)
        center, heading = [0.0, 0.0, 0.0], 0.0
        host_sub = tree.Sector_Search(center, 80.0, heading)
        assert len(host_sub) > 8192  # more than one target tile
        dev = torch.device("cuda", 0)
        d_sub = torch.zeros((tree.size(), 4), dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        tree.sector_search_device(center, 80.0, heading, d_sub.data_ptr(), d_cnt.data_ptr())
        src = torch.from_numpy(scan).to(dev)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        sn = torch.tensor([len(scan)], dtype=torch.int32, device=dev)
        res = torch.zeros((1, 96), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        batch = icp4r.Batch(src=src.data_ptr(), tgt=d_sub.data_ptr(), src_off=zero.data_ptr(), src_n=sn.data_ptr(),
                            tgt_off=zero.data_ptr(), tgt_n=d_cnt.data_ptr(), npairs=1, max_src_n=len(scan),
                            max_tgt_n=tree.size())
        gpu_ctx.align_batch_device(batch, _params(max_iterations=8), res.data_ptr(), None)
        gpu_ctx.synchronize()
        r = np.frombuffer(res.cpu().numpy().tobytes(), dtype=icp4r.RESULT_DTYPE)[0]
    finally:
        tree.close()
    o = rt.icp(scan, host_sub, max_iterations=8)
    assert sum(o["rejected"]) > 0
    assert_equal_twin(r, o)
