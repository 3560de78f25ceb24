"""The 3D Doppler ego-velocity estimator on the GPU (include/icp4r/icp4r_reve.h) against its twin
(tests/reve_twin.py).

Bars.  The hypothesis stage is + - * / sqrt in a stated order on both sides, so the inlier mask, n_valid,
n_inliers, iterations, accepted, best, zero_velocity and success are compared exactly, and so are the
packed clouds and their descriptors.  v and sigma come out of the refit, whose sums the device forms in
a fixed-order tree and the twin in index order: they take the bar tests/test_ego_edges.py uses for its
least squares, max(1e-9, 16 c n_inliers 2^-53) max|.| with c = cond(HtH) of the refit (numpy, on the
twin's sums).  Where the twin's value is not finite (three inliers: 0 / 0) the pattern of non-finite
components is compared.  ICP over the packed clouds is bit-exact against the oracle on the twin's
clouds (tests/test_gate_gpu.py's bar).
"""
import numpy as np
import pytest

import gate_twin
import reve_twin
from icp4r import synth
from test_reve import KNOWN, _scan

E_INVALID, E_EMPTY = -1, -2
GUARD = 64
EXACT = ("n", "n_valid", "n_inliers", "iterations", "accepted", "best", "zero_velocity", "success")


def _twin_params(p):
    return reve_twin.params(**p.as_dict())


def _guarded(torch, n, dtype, fill, dev, cols=None):
    shape = (n + 2 * GUARD,) if cols is None else (n + 2 * GUARD, cols)
    whole = torch.full(shape, fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _intact(whole, n, fill):
    a = whole.cpu().numpy()
    return bool((a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all())


def _run(ctx, rec, off, cnt, max_n, params=None, pack=False, use_stream=True):
    """The batch entries on device tensors with guard elements around every output.  -> dict(res, mask
    [, clouds, pair_off, pair_n]); asserts the guards."""
    import torch

    from icp4r import reve

    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 5)
    off, cnt = np.asarray(off, np.int64), np.asarray(cnt, np.int32)
    ns, total = len(cnt), len(rec)
    dev = torch.device("cuda", 0)
    rec_d = torch.from_numpy(rec).to(dev) if total else torch.zeros((1, 5), dtype=torch.float32, device=dev)
    off_d, cnt_d = torch.from_numpy(off).to(dev), torch.from_numpy(cnt).to(dev)
    res_w, res_d = _guarded(torch, ns * 88, torch.uint8, 0xA5, dev)
    mask_w, mask_d = _guarded(torch, max(total, 1), torch.uint8, 9, dev)
    out = {}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev) if use_stream else None
    st = stream.cuda_stream if stream is not None else None
    if pack:
        room = max(total, 1)
        clouds_w, clouds_d = _guarded(torch, room, torch.float32, -7.0, dev, cols=4)
        poff_w, poff_d = _guarded(torch, ns + 1, torch.int64, -7, dev)
        pn_w, pn_d = _guarded(torch, ns + 1, torch.int32, -7, dev)
        torch.cuda.synchronize()
        reve.inlier_clouds_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n, res_d.data_ptr(),
                                        clouds_d.data_ptr(), poff_d.data_ptr(), pn_d.data_ptr(), params=params,
                                        mask_ptr=mask_d.data_ptr(), ctx=ctx, stream=st)
    else:
        reve.estimate_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, max_n, res_d.data_ptr(),
                                   params=params, mask_ptr=mask_d.data_ptr(), ctx=ctx, stream=st)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    torch.cuda.synchronize()
    out["res"] = np.frombuffer(res_d.cpu().numpy().tobytes(), dtype=reve.REVE_RESULT_DTYPE)
    out["mask"] = mask_d.cpu().numpy()[:total]
    assert _intact(res_w, ns * 88, 0xA5) and _intact(mask_w, max(total, 1), 9)
    if pack:
        out["clouds"], out["pair_off"], out["pair_n"] = clouds_d.cpu().numpy(), poff_d.cpu().numpy(), pn_d.cpu().numpy()
        assert _intact(clouds_w, room, -7.0) and _intact(poff_w, ns + 1, -7) and _intact(pn_w, ns + 1, -7)
    return out


def _close(got, want, c, n_inl, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.isfinite(want).all():
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (what, got, want)
        return
    bar = max(1e-9, 16.0 * c * n_inl * 2.0 ** -53) * np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"{what}: |device - twin| = {err:.3e}, bar {bar:.3e} (cond {c:.3g}, {n_inl} inliers)")
    assert err <= bar, (what, got, want, c, bar)


def _check_scan(row, mask, t, tag=""):
    """One result row and its mask bytes against the twin's result of the same scan."""
    for k in EXACT:
        assert int(row[k]) == int(t[k]), (tag, k, int(row[k]), int(t[k]))
    assert int(row["status"]) == (0 if t["n"] else E_EMPTY), tag
    assert np.array_equal(mask, t["mask"]), (tag, int((mask != t["mask"]).sum()))
    c = 1.0
    if t["refit_M"] is not None:
        m = t["refit_M"]
        c = np.linalg.cond(np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]]))
    if not c <= 1e12:
        assert np.array_equal(np.isfinite(row["v"]), np.isfinite(t["v"])), tag
        return
    _close(row["v"], t["v"], c, t["n_inliers"], f"{tag} v")
    _close(row["sigma"], t["sigma"], c, t["n_inliers"], f"{tag} sigma")


def _crafted(n, seed=3):
    """n points of a moving scan with invalid points strewn in (ranks differ from indices) and a few
    standstill-like Dopplers; n < 8: every point valid."""
    rec = synth.make_sequence(seed, frames=1, n=max(n, 8), el_deg=30.0)[0][0][:n].copy()
    if n >= 8:
        rec[1::7, 3] = 0.0        # intensity 0: invalid
        rec[5::31, 0] = np.nan
        rec[6::53, 4] = np.inf
        rec[3::11, 4] = 0.01
    return rec


# ----------------------------------------------------------------------------------- 1. sizes
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_parity_with_twin_on_crafted_sizes(gpu_ctx, n):
    from icp4r import reve

    rec = _crafted(n)
    p = reve.default_params(seed=1000 + n)
    t = reve_twin.estimate(rec, _twin_params(p))
    got = _run(gpu_ctx, rec, [0], [n], n, p)
    _check_scan(got["res"][0], got["mask"], t, f"n={n}")
    if n >= 63:
        assert t["best"] >= 0 and 0 < t["n_valid"] < n and t["n_inliers"] > n // 2
    if n in (3, 4):
        assert t["n_valid"] == n and t["iterations"] == 37
    if n:  # the one-scan host entry: the same row and mask
        r, mask = reve.estimate(rec, p, ctx=gpu_ctx, want_mask=True)
        assert bytes(r) == got["res"][0].tobytes() and np.array_equal(mask, got["mask"])


@pytest.mark.gpu
def test_scan_past_the_lds_copy(gpu_ctx):
    """8192 + 300 points: the points past the LDS copy are re-read from the workspace, and drawn from;
    a second, short scan shares the batch (its workspace rows are unused)."""
    from icp4r import reve

    n = 8192 + 300
    rec = synth.make_sequence(8, frames=1, n=n, el_deg=30.0)[0][0].copy()
    rec[1::7, 3] = 0.0
    p = reve.default_params(seed=77)
    tp = _twin_params(p)
    small = _crafted(100)
    both = np.concatenate([rec, small])
    got = _run(gpu_ctx, both, [0, n], [n, 100], n, p, pack=True)
    ts = reve_twin.estimate_batch(both, [0, n], [n, 100], n, tp)
    _check_scan(got["res"][0], got["mask"][:n], ts[0], "8492")
    _check_scan(got["res"][1], got["mask"][n:], ts[1], "100 beside 8492")
    assert ts[0]["mask"][8192:].sum() > 100  # inliers past the LDS copy
    tri = [reve_twin.draw(p.seed, k, ts[0]["n_valid"]) for k in range(37)]
    assert max(max(d) for d in tri) > 8192 * 6 // 7  # hypotheses drew from there too
    mask = np.concatenate([ts[0]["mask"], ts[1]["mask"]])
    clouds, po, pn = gate_twin.compact(both[:, :4], [0, n], [n, 100], mask, n)
    assert np.array_equal(got["pair_n"], pn) and np.array_equal(got["pair_off"], po)
    assert got["clouds"][:len(clouds)].tobytes() == clouds.tobytes()


# ----------------------------------------------------------------------------------- 2. filters and edges
GOOD = np.array([[10, 1, 1, 5, -9.6], [12, -2, 0.5, 5, -9.7], [9, 3, -1, 5, -9.1], [15, 0, 2, 5, -9.8],
                 [20, 5, -3, 7, -9.3], [8, -1, 2, 3, -9.2]], np.float32)
BAD = np.array([[0.25, 0, 0, 5, 1], [0.1, 0, 0, 5, 1], [100, 0, 0, 5, 1], [150, 0, 0, 5, 1], [10, 1, 1, 0, 1],
                [5, 10, 0, 5, 1], [-5, 1, 0, 5, 1], [5, 0, 10, 5, 1], [5, 0, -10, 5, 1], [np.nan, 1, 1, 5, 1],
                [10, np.inf, 1, 5, 1], [10, 1, -np.inf, 5, 1], [10, 1, 1, 5, np.nan], [10, 1, 1, 5, -np.inf],
                [10, 1, 1, np.nan, 1]], np.float32)


@pytest.mark.gpu
def test_each_filter_alone_and_two_or_three_valid_targets(gpu_ctx):
    """Range at and beyond both limits, intensity 0, azimuth and elevation beyond, non-finite coordinates,
    Doppler and intensity: one scan per bad point among six good ones, then exactly 2 and exactly 3 valid
    targets among all the bad ones, and the z limits on and off."""
    from icp4r import reve

    p = reve.default_params(seed=5)
    tp = _twin_params(p)
    scans = [np.concatenate([GOOD[:3], b[None], GOOD[3:]]) for b in BAD]
    scans.append(np.concatenate([BAD[:7], GOOD[:1], BAD[7:], GOOD[1:2]]))           # 2 valid
    scans.append(np.concatenate([GOOD[:1], BAD[:7], GOOD[1:2], BAD[7:], GOOD[2:3]]))  # 3 valid
    cnt = [len(s) for s in scans]
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rec = np.concatenate(scans)
    got = _run(gpu_ctx, rec, off, cnt, max(cnt), p)
    ts = reve_twin.estimate_batch(rec, off, cnt, max(cnt), tp)
    for s, t in enumerate(ts):
        _check_scan(got["res"][s], got["mask"][off[s]:off[s] + cnt[s]], t, f"scan {s}")
    assert [int(r["n_valid"]) for r in got["res"]] == [6] * len(BAD) + [2, 3]
    assert all(got["mask"][off[s] + 3] == 0 for s in range(len(BAD)))
    two, three = got["res"][-2], got["res"][-1]
    assert (two["iterations"], two["n_inliers"], two["best"], two["success"]) == (0, 0, -1, 0)
    assert three["iterations"] == 37
    # the z limits act only with use_z_filter = 1
    zrec = np.concatenate([GOOD, [[5, 0, 3.0, 5, -9.0], [5, 0, 2.9, 5, -9.0]]]).astype(np.float32)
    for use_z, nv in ((0, 8), (1, 6)):  # z = -3 (the fifth good point) and z = 3 go
        pz = reve.default_params(seed=5, use_z_filter=use_z)
        g = _run(gpu_ctx, zrec, [0], [8], 8, pz)
        _check_scan(g["res"][0], g["mask"], reve_twin.estimate(zrec, _twin_params(pz)), f"use_z={use_z}")
        assert g["res"][0]["n_valid"] == nv


@pytest.mark.gpu
def test_standstill_threshold_one_float_below_and_at(gpu_ctx):
    """8 valid targets, n = (size_t)(8 * 0.75) = 6: a[6] one float below the threshold is a standstill
    (7 inliers), a[6] at the threshold is not (median < threshold is false) and RANSAC runs."""
    from icp4r import reve

    thr = np.float32(0.05)
    p = reve.default_params(seed=11, thresh_zero_velocity=float(thr))
    tp = _twin_params(p)
    base = synth.make_sequence(4, frames=1, n=8, el_deg=30.0)[0][0].copy()
    base[:, 4] = [0.01, -0.02, 3.0, 0.0, -0.03, 0.04, 0.0, 0.02]
    below, at = base.copy(), base.copy()
    below[6, 4] = -np.nextafter(thr, np.float32(0))
    at[6, 4] = -thr
    rec = np.concatenate([below, at])
    got = _run(gpu_ctx, rec, [0, 8], [8, 8], 8, p)
    ts = reve_twin.estimate_batch(rec, [0, 8], [8, 8], 8, tp)
    for s in range(2):
        _check_scan(got["res"][s], got["mask"][8 * s:8 * s + 8], ts[s], f"scan {s}")
    r0, r1 = got["res"]
    assert (r0["zero_velocity"], r0["n_inliers"], r0["success"], r0["iterations"]) == (1, 7, 1, 0)
    assert (r0["sigma"] == 0.025).all() and (r0["v"] == 0).all()
    assert (r1["zero_velocity"], r1["iterations"]) == (0, 37)


@pytest.mark.gpu
def test_first_of_tied_hypotheses_wins(gpu_ctx):
    """Noise-free Doppler, 40 % dynamic points: every accepted hypothesis drawn from three static points
    counts exactly the static points, so the maximum is attained many times; the first must win."""
    from icp4r import reve

    rec = synth.make_sequence(21, frames=1, n=513, doppler_noise=0.0, dynamic=0.4, el_deg=30.0)[0][0]
    p = reve.default_params(seed=4)
    t = reve_twin.estimate(rec, _twin_params(p))
    top = max(t["counts"])
    tied = [k for k, c in enumerate(t["counts"]) if c == top]
    assert len(tied) >= 3 and t["best"] == tied[0] and tied[0] > 0  # not hypothesis 0, and later ties exist
    got = _run(gpu_ctx, rec, [0], [513], 513, p)
    _check_scan(got["res"][0], got["mask"], t, "tie")
    assert got["res"][0]["best"] == tied[0] and got["res"][0]["n_inliers"] == top


@pytest.mark.gpu
def test_all_planar_scan_rejects_every_hypothesis(gpu_ctx):
    from icp4r import reve

    rec = _scan("planar")
    got = _run(gpu_ctx, rec, [0], [2048], 2048, reve.default_params())
    r = got["res"][0]
    _check_scan(r, got["mask"], reve_twin.estimate(rec), "planar")
    assert (r["n_valid"], r["iterations"], r["accepted"], r["best"], r["n_inliers"], r["success"]) == (2048, 37, 0, -1, 0, 0)
    assert not got["mask"].any()


# ----------------------------------------------------------------------------------- 3. batches
@pytest.mark.gpu
@pytest.mark.parametrize("pack", [False, True])
def test_batch_shuffled_oversized_guarded_on_a_callers_stream(gpu_ctx, pack):
    """Scans in shuffled memory order, standstill and moving ones together, an empty one, a negative
    count, one scan above max_n lying over 0xFF bytes (not read: its mask bytes keep their fill and it
    packs nothing), guard elements around every output, a caller's stream."""
    from icp4r import reve

    rng = np.random.default_rng(12)
    max_n = 700
    scans = [_crafted(700, 5), _scan("still")[:300], _crafted(65, 6), np.zeros((0, 5), np.float32), _crafted(64, 7),
             np.zeros((max_n + 5, 5), np.float32), _scan("still")[300:364], _crafted(2, 8), _crafted(333, 9)]
    big = 5
    scans[big] = np.frombuffer(b"\xff" * (20 * (max_n + 5)), np.float32).reshape(-1, 5)
    cnt = np.array([len(s) for s in scans], np.int32)
    order = rng.permutation(len(scans))
    off = np.zeros(len(scans), np.int64)
    pos = 0
    for s in order:
        off[s] = pos
        pos += cnt[s]
    rec = np.zeros((pos, 5), np.float32)
    for s, sc in enumerate(scans):
        rec[off[s]:off[s] + cnt[s]] = sc
    # a tenth scan with a negative count, pointing at the first scan's records
    off = np.concatenate([off, [0]])
    cnt = np.concatenate([cnt, [-3]]).astype(np.int32)
    ns = len(cnt)
    p = reve.default_params(seed=321)
    ts = reve_twin.estimate_batch(rec, off, cnt, max_n, _twin_params(p))
    assert ts[big] is None and ts[-1] is None
    got = _run(gpu_ctx, rec, off, cnt, max_n, p, pack=pack)
    exp_mask = np.full(len(rec), 9, np.uint8)
    for s, t in enumerate(ts):
        row = got["res"][s]
        if t is None:
            assert row["status"] == E_INVALID and row["n_inliers"] == 0 and row["best"] == -1 and row["n"] == 0
            continue
        _check_scan(row, got["mask"][off[s]:off[s] + cnt[s]], t, f"scan {s}")
        exp_mask[off[s]:off[s] + cnt[s]] = t["mask"]
    assert np.array_equal(got["mask"], exp_mask)  # the oversized scan's bytes keep their fill
    assert (got["mask"][off[big]:off[big] + cnt[big]] == 9).all()
    zero = [int(r["zero_velocity"]) for r in got["res"]]
    assert zero[1] == 1 and zero[6] == 1 and zero[0] == 0 and zero[8] == 0
    assert got["res"][3]["status"] == E_EMPTY
    if pack:
        clouds, po, pn = gate_twin.compact(rec[:, :4], off, cnt, np.where(exp_mask == 9, 0, exp_mask), max_n)
        assert np.array_equal(got["pair_n"], pn) and np.array_equal(got["pair_off"], po)
        assert pn[1 + big] == 0 and pn[-1] == 0
        assert got["clouds"][:len(clouds)].tobytes() == clouds.tobytes()
        assert (got["clouds"][len(clouds):] == -7.0).all()
        assert [int(x) for x in pn[1:]] == [int(r["n_inliers"]) for r in got["res"]]


# ----------------------------------------------------------------------------------- 4. pipeline
@pytest.mark.gpu
def test_inlier_clouds_feed_the_batched_icp(gpu_ctx, oracle_mod):
    """Three frames of 512 points: the packed clouds and descriptors equal the twin's bit for bit, and
    icp4r_align_batch_device over the one buffer (src = pair_* + 1, tgt = pair_*) equals oracle.align on
    the twin's clouds, frame by frame, bit for bit."""
    import torch

    import icp4r
    from icp4r import reve

    frames, _ = synth.make_sequence(40, frames=3, n=512, el_deg=30.0, dynamic=0.3)
    ns, n = 3, 512
    rec = np.concatenate(frames)
    off, cnt = np.arange(ns, dtype=np.int64) * n, np.full(ns, n, np.int32)
    p = reve.default_params(seed=17)
    ts = reve_twin.estimate_batch(rec, off, cnt, n, _twin_params(p))
    tw = [synth.records_to_xyzi(f)[t["mask"] != 0] for f, t in zip(frames, ts)]
    assert all(250 < len(c) < n for c in tw)
    dev = torch.device("cuda", 0)
    rec_d = torch.from_numpy(rec).to(dev)
    off_d, cnt_d = torch.from_numpy(off).to(dev), torch.from_numpy(cnt).to(dev)
    res_d = torch.zeros(ns * 88, dtype=torch.uint8, device=dev)
    clouds_d = torch.zeros((ns * n, 4), dtype=torch.float32, device=dev)
    poff_d = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
    pn_d = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
    icp_d = torch.zeros(ns * 96, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    reve.inlier_clouds_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), ns, n, res_d.data_ptr(),
                                    clouds_d.data_ptr(), poff_d.data_ptr(), pn_d.data_ptr(), params=p, ctx=gpu_ctx, stream=st)
    b = icp4r.Batch()
    b.src = b.tgt = clouds_d.data_ptr()
    b.src_off, b.src_n = poff_d.data_ptr() + 8, pn_d.data_ptr() + 4
    b.tgt_off, b.tgt_n = poff_d.data_ptr(), pn_d.data_ptr()
    b.npairs, b.max_src_n, b.max_tgt_n = ns, n, n
    gpu_ctx.align_batch_device(b, icp4r.default_params(), icp_d.data_ptr(), stream=st)  # no host round trip between
    stream.synchronize()
    torch.cuda.synchronize()
    pn, po, clouds = pn_d.cpu().numpy(), poff_d.cpu().numpy(), clouds_d.cpu().numpy()
    want = np.concatenate(tw)
    assert pn.tolist() == [len(tw[0])] + [len(c) for c in tw]
    assert po.tolist() == [0, 0, len(tw[0]), len(tw[0]) + len(tw[1])]
    assert clouds[:len(want)].tobytes() == want.tobytes()
    icp = np.frombuffer(icp_d.cpu().numpy().tobytes(), dtype=icp4r.RESULT_DTYPE)
    for k in range(ns):
        o = oracle_mod.align(tw[k], tw[k - 1 if k else 0], numerics=oracle_mod.NUM_F32)
        r = icp[k]
        assert np.array_equal(r["T"].reshape(4, 4).T, o["T"]) and r["fitness"] == o["fitness"], k
        assert r["iterations"] == o["iterations"] and r["status"] == o["status"] == 0, k
    # the one-scan host entry hands back the same cloud
    r1, c1 = reve.inlier_cloud(frames[0], p, ctx=gpu_ctx)
    assert c1.tobytes() == tw[0].tobytes() and r1.n_inliers == len(tw[0])


# ----------------------------------------------------------------------------------- 5. known answers
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seq0", "movers1", "still"])
def test_device_reproduces_the_twins_known_answers(gpu_ctx, kind):
    from icp4r import reve

    rec = _scan(kind)
    r, mask = reve.estimate(rec, ctx=gpu_ctx, want_mask=True)
    assert (r.n_valid, r.n_inliers, r.accepted, r.best, r.zero_velocity, r.success) == KNOWN[kind]
    assert int(mask.sum()) == r.n_inliers and r.status == 0
    if kind == "seq0":
        assert r.n_inliers == 1825 and np.abs(r.velocity() - [5, 0, 0]).max() < 1e-3 and r.iterations == 37
    if kind == "movers1":
        assert 1450 <= r.n_inliers <= 1560 and np.abs(r.velocity() - [5, 0, 0]).max() < 2e-3
    if kind == "still":
        assert r.n_inliers == 1792 and (r.velocity() == 0).all() and (r.stddev() == 0.025).all()
    t = reve_twin.estimate(rec)
    row = np.frombuffer(bytes(r), dtype=reve.REVE_RESULT_DTYPE)[0]
    _check_scan(row, mask, t, kind)
