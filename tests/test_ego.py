"""Radar ego velocity: the node's parse, fitSineRansac, static split and least
squares (src/iterative_closest_point.cpp:354-431) — oracle known answers on CPU, HIP product parity
on the GPU.

Parity status: unpinned by the reference (no tests or fixtures; the node needs ROS/PCL).  The oracle
(oracle/ego_oracle.c) is pinned by analytic known answers: a synthetic sequence with a known sensor
velocity (icp4r.synth.make_sequence) must come back as Vxyz = -v_sensor.  Bars (GPU vs oracle):
features within 4 float ulp (the device rounds the double atan2 / asin; glibc's float versions, which the
node calls, are off by an ulp in ~16 % / ~4 % of cases); with identical features, every
hypothesis score and the winner identical, A and b within 1e-12, the static mask identical and Vxyz
within 1e-9 (both sum the normal equations in double, in different orders).

tests/test_ego_edges.py holds the branches these scans do not reach, under the same bars: explicit
`iterations` at the hypothesis- and point-tile edges, scans below 5 points, a winner that is the first
of many tied maxima, the batch entry point against the oracle (empty, tiny and oversized scans,
guard bytes, a caller's stream) and feature edge records; for small or ill-conditioned scans its
Vxyz bar is derived from cond(KtK).  The map tests' edge-filter bar is in tests/test_map_exact.py.
"""
import numpy as np
import pytest

from icp4r import synth

TOL_V_KAT = 0.05  # m/s: Doppler noise 0.02 m/s over ~1800 static points, planar-model residual


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ---------------------------------------------------------------------------------------------- oracle
def test_oracle_features_known_answers(oracle_mod):
    rec = np.array([[1, 0, 0, 5, 0.5], [0, 2, 0, 1, -1], [3, 0, 3, 0, 2], [-1, -1, 0, 0, 0]], np.float32)
    f = oracle_mod.ego_features(rec)
    assert f[0, 0] == 1.0 and f[0, 1] == 0.0 and f[0, 2] == 0.0 and f[0, 3] == np.float32(0.5)
    assert f[1, 0] == 2.0 and abs(f[1, 1] - 90.0) < 1e-5 and f[1, 2] == 0.0
    assert abs(f[2, 2] - 45.0) < 1e-5 and abs(f[2, 0] - np.sqrt(18.0)) < 1e-6
    assert abs(f[3, 1] + 135.0) < 1e-5


def test_oracle_hypothesis_stream(oracle_mod):
    L = oracle_mod.lib()
    idx = [L.ego_hyp_index(7, k, 100) for k in range(1000)]
    assert min(idx) >= 0 and max(idx) <= 99  # never points[num] (the reference's inclusive draw)
    assert idx == [L.ego_hyp_index(7, k, 100) for k in range(1000)]  # reproducible
    assert len(set(idx)) > 90


@pytest.mark.parametrize("seq", [0, 1, 2])
def test_oracle_recovers_known_velocity(oracle_mod, seq):
    frames, v = synth.make_sequence(seq, frames=2, n=2048, speed=4.0 + seq)
    for rec in frames:
        f = oracle_mod.ego_features(rec)
        A, b, best, bh, scores = oracle_mod.ego_ransac(f)
        assert len(scores) == int(len(rec) * 0.2) and bh >= 0 and best == scores.max()
        assert bh == int(np.argmax(scores))  # the first strict maximum
        V, mask, ns = oracle_mod.ego_split_lsq(f, A, b)
        assert np.abs(V - (-v)).max() < TOL_V_KAT, (V, v)
        assert ns == int(mask.sum()) and 0.8 * len(rec) < ns < len(rec)
        assert abs(abs(A) - np.linalg.norm(v)) < 0.1


def test_oracle_degenerate_cases(oracle_mod):
    # a hypothesis whose two points coincide is 0/0: NaN model, score 0 (as in the reference)
    rec = np.tile(np.array([[10, 1, 0, 1, -3]], np.float32), (5, 1))
    f = oracle_mod.ego_features(rec)
    A, b, best, bh, scores = oracle_mod.ego_ransac(f, iterations=8)
    assert best == 0.0 and bh == -1 and A == 0.0 and b == 0.0 and (scores == 0).all()
    A, b, best, bh, scores = oracle_mod.ego_ransac(np.zeros((0, 4), np.float32))
    assert bh == -1 and len(scores) == 0


# ---------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("seq", [0, 3])
def test_gpu_features_match_oracle(gpu_ctx, oracle_mod, seq):
    from icp4r import ego

    frames, _ = synth.make_sequence(seq, frames=1, n=8192)
    rec = frames[0]
    xyzi, feat = ego.radar_features(rec, ctx=gpu_ctx)
    of = oracle_mod.ego_features(rec)
    assert (xyzi == rec[:, :4]).all()
    assert (feat[:, 0] == of[:, 0]).all() and (feat[:, 3] == of[:, 3]).all()  # sqrtf, v_r: exact
    ua, ub = _ulps(feat[:, 1], of[:, 1]), _ulps(feat[:, 2], of[:, 2])
    assert ua.max() <= 4 and ub.max() <= 4, (ua.max(), ub.max())
    assert (ua == 0).mean() > 0.7 and (ub == 0).mean() > 0.7  # glibc's float atan2/asin are ~1 ulp


@pytest.mark.gpu
@pytest.mark.parametrize("seq,n", [(0, 2048), (1, 8192), (2, 1000)])
def test_gpu_ransac_lsq_match_oracle(gpu_ctx, oracle_mod, seq, n):
    """Same features in (the GPU's): every score, the winner, the model, the mask and Vxyz agree."""
    from icp4r import ego

    frames, v = synth.make_sequence(seq, frames=1, n=n)
    rec = frames[0]
    _, feat = ego.radar_features(rec, ctx=gpu_ctx)
    r, mask, scores = ego.ego_velocity(rec, ctx=gpu_ctx, want_mask=True, want_scores=True)
    A, b, best, bh, osc = oracle_mod.ego_ransac(feat)
    assert (scores == osc).all()
    assert r.best == bh and r.score == best and r.iterations == int(n * 0.2)
    assert abs(r.A - A) <= 1e-12 * abs(A) and abs(r.b - b) <= 1e-12 * max(abs(b), 1e-3)
    V, omask, ns = oracle_mod.ego_split_lsq(feat, r.A, r.b)
    assert (mask == omask).all() and r.n_static == ns
    assert np.abs(r.velocity() - V).max() <= 1e-9 * np.abs(V).max()
    assert np.abs(r.velocity() - (-v)).max() < TOL_V_KAT


@pytest.mark.gpu
def test_gpu_end_to_end_vs_oracle(gpu_ctx, oracle_mod):
    """Records in, each side with its own parse: the GPU's Vxyz against the oracle's."""
    from icp4r import ego

    frames, v = synth.make_sequence(5, frames=4, n=4096)
    for rec in frames:
        r, _, _ = ego.ego_velocity(rec, ctx=gpu_ctx)
        f = oracle_mod.ego_features(rec)
        A, b, best, bh, _ = oracle_mod.ego_ransac(f)
        V, _, ns = oracle_mod.ego_split_lsq(f, A, b)
        assert abs(r.score - best) <= 2 and abs(r.n_static - ns) <= 2
        assert np.abs(r.velocity() - V).max() < 1e-3


@pytest.mark.gpu
def test_gpu_batch_equals_single(gpu_ctx):
    import torch

    from icp4r import ego

    frames, _ = synth.make_sequence(6, frames=5, n=3000)
    frames = [frames[0], frames[1][:1500], frames[2][:7], frames[3], frames[4][:2999]]
    cnt = np.array([len(f) for f in frames], np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    dev = torch.device("cuda", 0)
    rec_d = torch.from_numpy(np.concatenate(frames)).to(dev)
    off_d, cnt_d = torch.from_numpy(off).to(dev), torch.from_numpy(cnt).to(dev)
    res_d = torch.zeros((len(frames), 72), dtype=torch.uint8, device=dev)
    mask_d = torch.zeros(int(cnt.sum()), dtype=torch.uint8, device=dev)
    p = ego.default_params(seed=1234)
    ego.ego_velocity_batch_device(rec_d.data_ptr(), off_d.data_ptr(), cnt_d.data_ptr(), len(frames), int(cnt.max()),
                                  res_d.data_ptr(), params=p, mask_ptr=mask_d.data_ptr(), ctx=gpu_ctx)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    res = np.frombuffer(res_d.cpu().numpy().tobytes(), dtype=ego.EGO_RESULT_DTYPE)
    mask = mask_d.cpu().numpy()
    for s, rec in enumerate(frames):
        single, m, _ = ego.ego_velocity(rec, params=ego.default_params(seed=1234 + (s << 32)), ctx=gpu_ctx,
                                        want_mask=True)
        assert bytes(single) == res[s].tobytes()
        assert (m == mask[off[s]:off[s] + cnt[s]]).all()


@pytest.mark.gpu
def test_gpu_ego_errors(gpu_ctx):
    from icp4r import ICP4RError, ego

    with pytest.raises(ICP4RError):
        ego.ego_velocity(np.zeros((0, 5), np.float32), ctx=gpu_ctx)
    with pytest.raises(ICP4RError):
        ego.ego_velocity(np.zeros((10, 5), np.float32), params=ego.default_params(sigma=0.0), ctx=gpu_ctx)
