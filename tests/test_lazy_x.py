"""Plan option lazy_x: every second fused tail of fold_update_kernel is silent — it tests the moved
source cloud without storing it or its bounds, the next update forms T_pend * X itself, the search in
between flags the points it re-writes, and the following tail stores both steps at once — needs a
real MI355X.

lazy_x = 0 stores in every tail.  Both settings must give byte-equal result rows and aligned clouds
and the same cached-neighbour counters (the L and U values are the same bits, only formed later), over a
ragged batch on the batched plan: both parities of max_iterations (the tails alternate backwards from
the last one, so the first tail is silent or storing), PCL's early stops live (pairs converge in
pending and in non-pending updates), Huber weights, a distance threshold, and fuse_test = 0 (where the
option must do nothing).  Sampled pairs equal the oracle bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the smallest batch that takes the batched plan (256 pairs): a few full-size and odd-size pairs (last
# partial tail groups, more than one fold chunk, fewer points than one wave), the rest 600..2048 points
SPECIAL = [(8192, 8192), (8191, 8000), (4097, 5000), (300, 4000), (37, 4000)]
NPAIRS = 260
SAMPLED = (0, 1, 2, 3, 4, 5, 131, 259)
FIXED = dict(mse_threshold_absolute=-1.0, transformation_epsilon=-1.0)


def _shapes():
    rng = np.random.default_rng(77)
    rest = [(int(rng.integers(600, 2049)), int(rng.integers(600, 2049))) for _ in range(NPAIRS - 2 * len(SPECIAL))]
    return SPECIAL + rest + SPECIAL  # (specials in both pair groups)


@pytest.fixture(scope="module")
def batch():
    """The ragged batch, on the device once: host pairs, the Batch structure with an aligned-cloud
    buffer, and run(ctx, params) -> (result rows, aligned cloud, nn_stats)."""
    import torch

    import icp4r
    from icp4r import synth

    shapes = _shapes()
    pairs = []
    for k, (n, m) in enumerate(shapes):
        p = synth.make_pair(5200 + k, n, m)
        pairs.append((p.src_xyzi(), p.tgt_xyzi()))
    dev = torch.device("cuda", 0)
    sn = np.array([len(p[0]) for p in pairs], np.int32)
    tn = np.array([len(p[1]) for p in pairs], np.int32)
    so = np.concatenate([[0], np.cumsum(sn)[:-1]]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tn)[:-1]]).astype(np.int64)
    t = {
        "src": torch.from_numpy(np.concatenate([p[0] for p in pairs]).astype(np.float32)).to(dev),
        "tgt": torch.from_numpy(np.concatenate([p[1] for p in pairs]).astype(np.float32)).to(dev),
        "so": torch.from_numpy(so).to(dev), "sn": torch.from_numpy(sn).to(dev),
        "to": torch.from_numpy(to).to(dev), "tn": torch.from_numpy(tn).to(dev),
    }
    t["aligned"] = torch.zeros_like(t["src"])
    b = icp4r.Batch(src=t["src"].data_ptr(), tgt=t["tgt"].data_ptr(), src_off=t["so"].data_ptr(),
                    src_n=t["sn"].data_ptr(), tgt_off=t["to"].data_ptr(), tgt_n=t["tn"].data_ptr(), guess=None,
                    aligned=t["aligned"].data_ptr(), npairs=len(pairs), max_src_n=int(sn.max()), max_tgt_n=int(tn.max()))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(ctx, params):
        out = torch.zeros((len(pairs), 96), dtype=torch.uint8, device=dev)
        t["aligned"].zero_()
        ctx.reset_timers()
        ctx.align_batch_device(b, params, out.data_ptr(), stream)
        torch.cuda.synchronize(dev)
        rows = np.frombuffer(out.cpu().numpy().tobytes(), dtype=icp4r.RESULT_DTYPE)
        return rows, t["aligned"].cpu().numpy().copy(), ctx.nn_stats()

    return {"pairs": pairs, "so": so, "sn": sn, "run": run, "max_n": int(sn.max()), "max_m": int(tn.max())}


def _both(gpu_ctx, plan, batch, params, **options):
    """The batch with lazy_x = 0 and 1 (and `options`), checked equal: rows, aligned clouds, counters."""
    import icp4r

    plan(counters=1, **options)
    pl = icp4r.plan(NPAIRS, batch["max_n"], batch["max_m"], ctx=gpu_ctx)
    assert pl["lds"] and pl["cache"]
    out = {}
    for on in (0, 1):
        plan(lazy_x=on)
        out[on] = batch["run"](gpu_ctx, params)
    assert out[1][0].tobytes() == out[0][0].tobytes()
    assert out[1][1].tobytes() == out[0][1].tobytes()
    for key in ("cache_tested", "cache_hits", "tested_in_update", "hits_in_update"):
        assert out[1][2][key] == out[0][2][key], (key, out[0][2][key], out[1][2][key])
    return out[1]


def _oracle(oracle_mod, batch, rows, aligned, ks, **kw):
    for k in ks:
        s, t = batch["pairs"][k]
        o = oracle_mod.align(s, t, numerics=oracle_mod.NUM_F32, aligned=True, **kw)
        assert rows[k]["status"] == o["status"], k
        assert (rows[k]["T"].reshape(4, 4).T == o["T"]).all(), k
        assert rows[k]["fitness"] == o["fitness"], k
        assert rows[k]["iterations"] == o["iterations"], k
        assert rows[k]["n_correspondences"] == o["n_correspondences"], k
        a = aligned[batch["so"][k]: batch["so"][k] + batch["sn"][k]]
        assert a[:, :3].tobytes() == np.ascontiguousarray(o["aligned"][:, :3]).tobytes(), k


def test_plan_reports_lazy_x(gpu_ctx, plan):
    """icp4r.plan(): on by default where the fused tail runs in fold_update_kernel, off with the option,
    without the fused test, with the sums tail or the on-chip update, in F64 numerics and off the
    batched plan."""
    import icp4r

    shape = (NPAIRS, 8192, 8192)
    assert icp4r.plan(*shape, ctx=gpu_ctx)["lazy_x"]
    assert gpu_ctx.get_plan_option("lazy_x") == (1, False)
    assert not icp4r.plan(*shape, numerics=icp4r.NUMERICS_F64, ctx=gpu_ctx)["lazy_x"]
    assert not icp4r.plan(1, 8192, 8192, ctx=gpu_ctx)["lazy_x"]
    for off in (dict(lazy_x=0), dict(fuse_test=0), dict(sums_tail=1), dict(res_update=1), dict(nn_cache=0)):
        gpu_ctx.reset_plan_options()
        plan(**off)
        assert not icp4r.plan(*shape, ctx=gpu_ctx)["lazy_x"], off


@pytest.mark.parametrize("iters", [1, 2, 7, 8])
def test_lazy_x_fixed_iterations(gpu_ctx, oracle_mod, batch, plan, iters):
    """Fixed iteration counts of both parities: no tail at all (1), one storing tail (2), and runs whose
    first tail is silent (7) or storing (8); the fitness pass always follows a storing tail."""
    import icp4r

    p = icp4r.default_params(max_iterations=iters, **FIXED)
    rows, aligned, st = _both(gpu_ctx, plan, batch, p)
    assert (rows["status"] == 0).all() and (rows["iterations"] == iters).all()
    assert (st["tested_in_update"] > 0) == (iters > 1)
    if iters in (7, 8):
        _oracle(oracle_mod, batch, rows, aligned, SAMPLED, max_iterations=iters, **FIXED)


def test_lazy_x_early_stops(gpu_ctx, oracle_mod, batch, plan):
    """PCL's defaults: pairs converge at different iterations, in pending updates (whose stop makes the
    store the silent tail left out) and in non-pending ones."""
    import icp4r

    p = icp4r.default_params(max_iterations=20)
    rows, aligned, _ = _both(gpu_ctx, plan, batch, p)
    assert (rows["status"] == 0).all()
    its = set(rows["iterations"].tolist())
    assert len(its) > 1
    assert {i & 1 for i in its} == {0, 1}, its  # stops after an even and after an odd number of updates
    _oracle(oracle_mod, batch, rows, aligned, SAMPLED, max_iterations=20)


@pytest.mark.parametrize("kw", [{"huber_delta": 0.5}, {"max_correspondence_distance": 0.45}])
def test_lazy_x_weighted_and_thresholded(gpu_ctx, oracle_mod, batch, plan, kw):
    """Huber weights (passes A and B weight the re-formed points) and a distance threshold (rejected
    correspondences: the sigma panels' ranked starts are counted over the re-formed points; the 37-point
    pairs run out of correspondences under it and stop with PCL's error, as in the oracle)."""
    import icp4r

    rows, aligned, _ = _both(gpu_ctx, plan, batch, icp4r.default_params(max_iterations=9, **kw))
    assert ((rows["status"] != 0).sum() > 0) == ("max_correspondence_distance" in kw)
    _oracle(oracle_mod, batch, rows, aligned, SAMPLED[2:], max_iterations=9, **kw)


def test_lazy_x_without_fused_test(gpu_ctx, batch, plan):
    """fuse_test = 0 (the test in its own kernel): lazy_x = 1 does nothing — equal to lazy_x = 0 there and to
    the default plan."""
    import icp4r

    p = icp4r.default_params(max_iterations=8, **FIXED)
    unfused = _both(gpu_ctx, plan, batch, p, fuse_test=0)
    gpu_ctx.reset_plan_options()
    rows, aligned, _ = batch["run"](gpu_ctx, p)
    assert rows.tobytes() == unfused[0].tobytes() and aligned.tobytes() == unfused[1].tobytes()
