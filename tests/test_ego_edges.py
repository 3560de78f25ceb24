"""Radar ego velocity: the branches tests/test_ego.py does not reach, against the oracle.

Explicit `iterations` (max_h, the grid and the score row stride then come from it, not from n) at the
hypothesis-tile (kEgoHyp = 1024) and point-tile (kEgoPts = 512) edges; scans below 5 points (no
hypothesis at all); a winner that is a real first-of-many tie; the batch entry point against the
oracle, with empty, tiny and oversized scans and guard bytes around its outputs; feature edge cases.

Bars are those of tests/test_ego.py with the GPU's features fed to the oracle: every score, the
winner, iterations, n, n_static and the mask identical, A and b within 1e-12 relative.  Vxyz: within
max(1e-9, 16 c n_static 2^-53) max|V|, c = cond(KtK) rebuilt here in float64 — both sides sum the
normal equations in double in different orders (n_static 2^-53 relative, amplified by c in the
solve; 16x for the different reduction trees); for a few thousand well-spread points this is the
1e-9 of test_ego.py.  Where c > 1e12 or the oracle's V is not finite, only the pattern of non-finite
components is compared.
"""
import numpy as np
import pytest

from icp4r import synth

DEG2RAD = 0.017453293  # PCL 1.8's DEG2RAD, the constant of both sides
E_INVALID, E_EMPTY = -1, -2


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _check_v(feat, mask, v_gpu, v_ref):
    """The derived Vxyz bar of the module docstring."""
    f = feat[mask.astype(bool)].astype(np.float64)
    a, be = f[:, 1] * DEG2RAD, f[:, 2] * DEG2RAD
    K = np.stack([np.cos(a) * np.cos(be), np.sin(a) * np.cos(be), np.sin(be)], 1)
    KtK = K.T @ K
    c = np.linalg.cond(KtK) if np.isfinite(KtK).all() else np.inf
    v_gpu, v_ref = np.asarray(v_gpu, np.float64), np.asarray(v_ref, np.float64)
    if not c <= 1e12 or not np.isfinite(v_ref).all():
        assert np.array_equal(np.isfinite(v_gpu), np.isfinite(v_ref)), (v_gpu, v_ref, c)
        return
    bar = max(1e-9, 16.0 * c * len(f) * 2.0 ** -53) * np.abs(v_ref).max()
    assert np.abs(v_gpu - v_ref).max() <= bar, (v_gpu, v_ref, c, bar)


def _check_result(oracle_mod, feat, r, mask, scores, iterations=None, sigma=0.5, seed=None):
    """One scan's result (ctypes struct or record of EGO_RESULT_DTYPE fields as attributes) against
    the oracle run on the same features."""
    n = len(feat)
    kw = {} if seed is None else {"seed": seed}
    A, b, best, bh, osc = oracle_mod.ego_ransac(feat, iterations=iterations, sigma=sigma, **kw)
    H = iterations if iterations else int(n * 0.2)
    assert len(osc) == H
    if scores is not None:
        assert np.array_equal(scores, osc)
    assert (r.best, r.score, r.iterations, r.n, r.status) == (bh, best, H, n, 0)
    if bh < 0:
        assert r.A == 0.0 and r.b == 0.0
    else:
        assert abs(r.A - A) <= 1e-12 * abs(A) and abs(r.b - b) <= 1e-12 * max(abs(b), 1e-3)
    V, omask, ns = oracle_mod.ego_split_lsq(feat, r.A, r.b)
    assert np.array_equal(mask, omask) and r.n_static == ns
    _check_v(feat, omask, np.array(r.v, np.float64), V)
    return bh, osc


class _Row:
    """Attribute access to one record of EGO_RESULT_DTYPE."""

    def __init__(self, rec):
        for k in rec.dtype.names:
            setattr(self, k, rec[k].tolist())


# ------------------------------------------------------------------------------------------- B1
@pytest.mark.gpu
@pytest.mark.parametrize("n,iterations", [(513, 1), (513, 1024), (513, 1025), (513, 2049), (512, 1025), (511, 1025)])
def test_explicit_iterations_and_tile_edges(gpu_ctx, oracle_mod, n, iterations):
    from icp4r import ego

    rec = synth.make_sequence(13, frames=1, n=513)[0][0][:n]
    _, feat = ego.radar_features(rec, ctx=gpu_ctx)
    r, mask, scores = ego.ego_velocity(rec, params=ego.default_params(iterations=iterations), ctx=gpu_ctx,
                                       want_mask=True, want_scores=True)
    assert len(scores) == iterations
    bh, osc = _check_result(oracle_mod, feat, r, mask, scores, iterations=iterations)
    assert bh >= 0 and osc.max() > 0.8 * n


# ------------------------------------------------------------------------------------------- B2
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 10])
def test_tiny_scans(gpu_ctx, oracle_mod, n):
    """Below 5 points (int)(0.2 n) = 0: no hypothesis, best = -1, A = b = 0 and the split runs with
    that model.  n = 5, 9, 10 have 1, 1, 2 hypotheses; the single one of n = 9 scores nothing."""
    from icp4r import ego

    rec = synth.make_sequence(12, frames=1, n=64)[0][0][:n]
    _, feat = ego.radar_features(rec, ctx=gpu_ctx)
    r, mask, scores = ego.ego_velocity(rec, ctx=gpu_ctx, want_mask=True, want_scores=True)
    assert len(scores) == int(n * 0.2) == {1: 0, 2: 0, 3: 0, 4: 0, 5: 1, 9: 1, 10: 2}[n]
    bh, _ = _check_result(oracle_mod, feat, r, mask, scores)
    assert (bh >= 0) == (n in (5, 10))
    if n < 5:
        assert (r.best, r.score, r.A, r.b, r.iterations, r.status) == (-1, 0.0, 0.0, 0.0, 0, 0)


# ------------------------------------------------------------------------------------------- B3
@pytest.mark.gpu
def test_first_of_many_tied_maxima_wins(gpu_ctx, oracle_mod):
    """make_sequence(21, n=513, doppler_noise=0, dynamic=0.8), sigma 0.1, 4096 hypotheses: on the CPU
    oracle the maximum 121 is reached first at h* = 43 and by 218 later hypotheses, 43 of them with
    (h mod 256) below (h* mod 256) — the select workgroup strides by 256, so a reduction that
    preferred a lower thread id, or a later tie, picks another winner."""
    from icp4r import ego

    rec = synth.make_sequence(21, frames=1, n=513, doppler_noise=0.0, dynamic=0.8)[0][0]
    _, feat = ego.radar_features(rec, ctx=gpu_ctx)
    p = ego.default_params(iterations=4096, sigma=0.1)
    r, mask, scores = ego.ego_velocity(rec, params=p, ctx=gpu_ctx, want_mask=True, want_scores=True)
    _, _, best, hstar, osc = oracle_mod.ego_ransac(feat, iterations=4096, sigma=0.1)
    ties = np.nonzero(osc == osc.max())[0]
    print("B3 case: best", best, "h*", hstar, "ties", len(ties), "lower residue",
          int(((ties % 256) < (hstar % 256)).sum()))
    assert hstar > 0 and hstar == ties[0] and len(ties) >= 10
    assert ((ties % 256) < (hstar % 256)).any()
    assert r.best == hstar
    _check_result(oracle_mod, feat, r, mask, scores, iterations=4096, sigma=0.1)


# ------------------------------------------------------------------------------------------- B4
BATCH_CNT = [600, 0, 3, 513, 5, 700, 600]
BATCH_MAX_N = 650
GUARD = 256
SENTINEL = 0xA5


def _run_batch(gpu_ctx, frames, iterations, stream=None):
    """The batch on guarded device buffers: (results bytes, mask bytes), guards included."""
    import torch

    from icp4r import ego

    cnt = np.array([len(f) for f in frames], np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    dev = torch.device("cuda", 0)
    rec_d = torch.from_numpy(np.concatenate(frames)).to(dev)
    off_d, cnt_d = torch.from_numpy(off).to(dev), torch.from_numpy(cnt).to(dev)
    res_d = torch.full((GUARD + 72 * len(frames) + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    mask_d = torch.full((GUARD + int(cnt.sum()) + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = ego.default_params(seed=1234, iterations=iterations)
    ego.ego_velocity_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), len(frames), BATCH_MAX_N,
                                  res_d.data_ptr() + GUARD, params=p, mask_ptr=mask_d.data_ptr() + GUARD, ctx=gpu_ctx,
                                  stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    else:
        gpu_ctx.synchronize()
    return res_d.cpu().numpy(), mask_d.cpu().numpy()


@pytest.fixture(scope="module")
def batch_frames():
    frames, _ = synth.make_sequence(6, frames=len(BATCH_CNT), n=max(BATCH_CNT))
    return [f[:c] for f, c in zip(frames, BATCH_CNT)]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [0, 1025])
def test_batch_against_the_oracle(gpu_ctx, oracle_mod, batch_frames, iterations):
    import torch

    from icp4r import ego

    res_b, mask_b = _run_batch(gpu_ctx, batch_frames, iterations)
    for buf in (res_b, mask_b):  # guard bytes on both sides of both outputs
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all()
    res = np.frombuffer(res_b[GUARD:-GUARD].tobytes(), dtype=ego.EGO_RESULT_DTYPE)
    mask = mask_b[GUARD:-GUARD]
    off = np.concatenate([[0], np.cumsum(BATCH_CNT)[:-1]])
    for s, rec in enumerate(batch_frames):
        row, m = _Row(res[s]), mask[off[s]:off[s] + len(rec)]
        if len(rec) == 0:
            assert row.status == E_EMPTY and row.n == 0
        elif len(rec) > BATCH_MAX_N:
            assert row.status == E_INVALID
            assert (m == SENTINEL).all()  # nothing is computed for a scan above max_n
        else:
            _, feat = ego.radar_features(rec, ctx=gpu_ctx)
            _check_result(oracle_mod, feat, row, m, None, iterations=iterations or None,
                          seed=1234 + (s << 32))
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert stream.cuda_stream != 0
    res_s, mask_s = _run_batch(gpu_ctx, batch_frames, iterations, stream=stream)
    assert res_s.tobytes() == res_b.tobytes() and mask_s.tobytes() == mask_b.tobytes()


@pytest.mark.gpu
def test_batch_host_side_errors(gpu_ctx, batch_frames):
    import torch

    from icp4r import ICP4RError, ego

    dev = torch.device("cuda", 0)
    rec_d = torch.from_numpy(batch_frames[0]).to(dev)
    off_d = torch.zeros(1, dtype=torch.int64, device=dev)
    cnt_d = torch.tensor([len(batch_frames[0])], dtype=torch.int32, device=dev)
    res_d = torch.full((72,), SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr())
    ego.ego_velocity_batch_device(*args, 0, BATCH_MAX_N, res_d.data_ptr(), ctx=gpu_ctx)  # nscans = 0: OK, no work
    gpu_ctx.synchronize()
    assert (res_d.cpu().numpy() == SENTINEL).all()
    for bad in ({"dynamic_threshold": float("nan")}, {"sigma": 0.0}, {"sigma": -0.5}, {"sigma": float("nan")}):
        with pytest.raises(ICP4RError) as ei:
            ego.ego_velocity_batch_device(*args, 1, BATCH_MAX_N, res_d.data_ptr(), params=ego.default_params(**bad),
                                          ctx=gpu_ctx)
        assert ei.value.code == E_INVALID
    gpu_ctx.synchronize()
    assert (res_d.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------------- B5
def _edge_records():
    rows = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],   # the six axis directions
            [-1, -0.0, 0], [-1, 0.0, 0],                                            # arfa -180 / +180
            [0, 0, 2.5], [0, 0, -2.5],                                              # on the z axis
            [0, 0, 0],                                                              # the origin: beta = asin(0/0)
            [1e20, 0, 1],                                                           # x*x overflows float
            [1e-20, 0, 0], [1e-20, 1e-20, 1e-20]]                                   # denormal squares
    rng = np.random.default_rng(55)
    rec = np.zeros((len(rows) + 300, 5), np.float32)
    rec[: len(rows), :3] = np.array(rows, np.float32)
    rec[len(rows):, :3] = rng.uniform(-60, 60, (300, 3)).astype(np.float32)
    rec[:, 3] = rng.uniform(0, 30, len(rec)).astype(np.float32)
    rec[:, 4] = rng.uniform(-5, 5, len(rec)).astype(np.float32)
    return rec, len(rows)


@pytest.mark.gpu
def test_feature_edge_records(gpu_ctx, oracle_mod):
    """distance and v_r exact, arfa and beta within 4 ulp, NaN in exactly the same entries."""
    from icp4r import ego

    rec, nhand = _edge_records()
    assert np.signbit(rec[6, 1]) and not np.signbit(rec[7, 1])
    xyzi, feat = ego.radar_features(rec, ctx=gpu_ctx)
    of = oracle_mod.ego_features(rec)
    assert xyzi.tobytes() == rec[:, :4].tobytes()
    print("hand-written rows, GPU:\n", feat[:nhand], "\noracle:\n", of[:nhand])
    assert of[6, 1] == -180.0 and of[7, 1] == 180.0 and np.isnan(of[10, 2]) and np.isinf(of[11, 0])
    assert of[12, 0] > 0 and of[13, 0] > 0 and of[12, 2] == 0.0  # the oracle keeps the denormal squares
    assert np.array_equal(np.isnan(feat), np.isnan(of))
    assert np.array_equal(feat[:, 0], of[:, 0], equal_nan=True) and np.array_equal(feat[:, 3], of[:, 3])
    ok = ~np.isnan(of)
    for col in (1, 2):
        u = _ulps(feat[ok[:, col], col], of[ok[:, col], col])
        assert u.max() <= 4, (col, int(u.max()), np.nonzero(u > 4)[0])


@pytest.mark.gpu
def test_record_at_the_origin(gpu_ctx, oracle_mod):
    """One record of a normal scan moved to the sensor origin: beta = NaN, so the point is never an
    inlier, is marked static (!(NaN > 0.2)) and makes the normal equations, and Vxyz, NaN."""
    from icp4r import ego

    rec = synth.make_sequence(13, frames=1, n=513)[0][0].copy()
    j = 200
    rec[j, :3] = 0.0
    _, feat = ego.radar_features(rec, ctx=gpu_ctx)
    assert np.isnan(feat[j, 2]) and np.isnan(feat).sum() == 1
    r, mask, scores = ego.ego_velocity(rec, ctx=gpu_ctx, want_mask=True, want_scores=True)
    bh, osc = _check_result(oracle_mod, feat, r, mask, scores)
    assert bh >= 0 and mask[j] == 1
    # never an inlier: the winner's score (identical to the oracle's, above) is the float64 numpy
    # count over the other 512 points; the point's own delta is NaN
    f = feat.astype(np.float64)
    with np.errstate(invalid="ignore"):
        delta = np.cos(f[:, 2] * DEG2RAD) * f[:, 3] - r.A * np.cos(f[:, 1] * DEG2RAD + r.b)
        inl = np.abs(delta) < 0.5
    assert np.isnan(delta[j]) and not inl[j]
    assert r.score == inl.sum() == np.delete(inl, j).sum() and scores.max() <= 512
    V = oracle_mod.ego_split_lsq(feat, r.A, r.b)[0]
    assert np.isnan(V).all() and np.isnan(np.array(r.v)).all()
