"""Voxelized GICP (fast_gicp::FastVGICP; include/icp4r/icp4r_vgicp.h) on the CPU: the numpy twin
tests/vgicp_twin.py pinned to the C oracle and to known answers.  tests/test_vgicp_gpu.py holds the device
against this twin.

Parity status: unpinned by the reference (fast_gicp is not available); parity is to the restatement in
icp4r_vgicp.h.

Known answers, measured on the twin alone (oracle covariances, k = 20, PLANE; the scenes of
tests/test_gicp.py: synth.make_pair(seed, 1500, clutter=0, noise=0.005), seeds 0, 1, 2; bars TOL_KAT_T =
0.02 m and TOL_KAT_R = 0.2 deg of that file).  DIRECT1 and DIRECT7 meet them at resolution 1.0.  DIRECT27 at
resolution 1.0 does not on the twin (seed 1: 2.95 cm, 6.3e-4 rad; seeds 0 and 2: 1.80 cm and 0.25 cm —
27 one-metre cells blur a 10 m scene), so DIRECT27 is checked at resolution 0.5, where it does.  The
twin's measured errors are KAT_MEASURED below.
"""
import numpy as np
import pytest

import vgicp_twin as tw
from helpers import pose_err
from test_gicp import TOL_KAT_R, TOL_KAT_T, _scene


# ------------------------------------------------------------------------------- crafted clouds (also GPU)
def crafted_clouds():
    """name -> (points (n, 3) float32, resolution): the voxel map's edge cases."""
    rng = np.random.default_rng(11)
    out = {}
    out["one_voxel"] = (rng.uniform(0.05, 0.95, (37, 3)).astype(np.float32), 1.0)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(3), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    out["own_voxels"] = ((g[rng.permutation(len(g))] + 0.5).astype(np.float32), 1.0)
    # negative coordinates: floor(-0.25) = -1 where truncation gives 0
    out["negative"] = (rng.uniform(-2.9, 2.9, (200, 3)).astype(np.float32), 1.0)
    # exactly on k * resolution (0.5 is exact in float and double): the point belongs to cell k
    k = rng.integers(-4, 5, (120, 3))
    out["on_faces"] = ((k * 0.5).astype(np.float32), 0.5)
    # resolution 0.3: p / 0.3 in double of the float point
    out["res_0p3"] = (np.concatenate([rng.uniform(-3, 3, (300, 3)), np.arange(-10, 11)[:, None] * [0.3, 0.3, 0.3]])
                      .astype(np.float32), 0.3)
    return out


def random_spd(rng, n):
    a = rng.normal(0, 1, (n, 3, 3))
    return a @ np.swapaxes(a, 1, 2) + 1e-3 * np.eye(3)


# ------------------------------------------------------------------------------- the twin's solver
def _gicp_functions(src, tgt, CA, CB, max_d2=np.inf):
    """GICP's point-to-point linearisation (icp4r_gicp.h) for the twin's LM driver."""
    s32, t32 = src.astype(np.float32), tgt.astype(np.float32)
    a, b = s32.astype(np.float64), t32.astype(np.float64)

    def nearest(R, t):
        Rf, tf = R.astype(np.float32), t.astype(np.float32)
        x = np.empty_like(s32)
        for r in range(3):
            v = Rf[r, 0] * s32[:, 0]
            v = v + Rf[r, 1] * s32[:, 1]
            v = v + Rf[r, 2] * s32[:, 2]
            x[:, r] = v + tf[r]
        d = x[:, None, :] - t32[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = d2.argmin(1)  # the lowest index among equal distances
        ok = d2[np.arange(len(j)), j].astype(np.float64) < max_d2
        return np.nonzero(ok)[0], j[ok]

    def linearize(R, t):
        i, j = nearest(R, t)
        M = tw.inv3(CB[j] + R @ CA[i] @ R.T)
        ta = np.stack([R[r, 0] * a[i, 0] + R[r, 1] * a[i, 1] + R[r, 2] * a[i, 2] + t[r] for r in range(3)], 1)
        e = b[j] - ta
        J = np.concatenate([tw.skew(ta), np.broadcast_to(-np.eye(3), (len(i), 3, 3))], 2)
        H = np.einsum("nki,nkl,nlj->ij", J, M, J)
        g = np.einsum("nki,nkl,nl->i", J, M, e)
        return H, g, float(np.einsum("nk,nkl,nl->", e, M, e)), len(i), (i, j, M)

    def error(R, t, kept):
        i, j, M = kept
        ta = np.stack([R[r, 0] * a[i, 0] + R[r, 1] * a[i, 1] + R[r, 2] * a[i, 2] + t[r] for r in range(3)], 1)
        e = b[j] - ta
        return float(np.einsum("nk,nkl,nl->", e, M, e))

    return linearize, error


@pytest.mark.parametrize("seed,guess", [(0, False), (3, False), (4, True)])
def test_twin_lm_driver_reproduces_the_gicp_oracle(oracle_mod, seed, guess):
    """The twin's Levenberg-Marquardt loop on GICP's own linearisation and the oracle's covariances is the
    C oracle's registration: pose within 1e-9, the same iteration count and flags."""
    src, tgt, T = _scene(seed, 400)
    G = None
    if guess:
        G = np.eye(4, dtype=np.float32)
        c, s = np.cos(0.1), np.sin(0.1)
        G[:2, :2] = [[c, -s], [s, c]]
        G[:3, 3] = [0.2, -0.1, 0.05]
    CA = oracle_mod.gicp_covariances(src, 5, oracle_mod.GICP_REG_PLANE)
    CB = oracle_mod.gicp_covariances(tgt, 5, oracle_mod.GICP_REG_PLANE)
    lin, err = _gicp_functions(src, tgt, CA, CB)
    r = tw.lm_align(lin, err, G)
    o = oracle_mod.gicp_align(src, tgt, guess=G, k=5)
    dt, dr = pose_err(r["T"], o["T"])
    print(f"seed {seed}: dt {dt:.3e} dr {dr:.3e} iterations {r['iterations']}/{o['iterations']}")
    assert dt < 1e-9 and dr < 1e-9
    assert r["iterations"] == o["iterations"] and r["converged"] == o["converged"]
    assert r["lm_failed"] == o["lm_failed"] and r["n_valid"] == o["n_valid"]


# ------------------------------------------------------------------------------- the voxel map
@pytest.mark.parametrize("name", sorted(crafted_clouds()))
def test_twin_voxel_map_crafted(name):
    pts, res = crafted_clouds()[name]
    rng = np.random.default_rng(5)
    C = random_spd(rng, len(pts))
    vm = tw.voxel_map(pts, C, res)
    assert int(vm.num.sum()) == len(pts)
    assert [tuple(c) for c in vm.coords] == sorted(tuple(c) for c in vm.coords)  # lexicographic, unique
    assert len({tuple(c) for c in vm.coords}) == len(vm.coords)
    # a direct computation: membership by floor of the double quotient, means by numpy
    cell = np.floor(pts.astype(np.float64) / res).astype(np.int64)
    for v, c in enumerate(vm.coords):
        member = np.all(cell == c, axis=1)
        assert member.sum() == vm.num[v]
        np.testing.assert_allclose(vm.mean[v], pts[member].astype(np.float64).mean(0), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(vm.cov[v], C[member].mean(0), rtol=1e-13, atol=1e-15)
    if name == "one_voxel":
        assert len(vm.coords) == 1 and tuple(vm.coords[0]) == (0, 0, 0)
    if name == "own_voxels":
        assert len(vm.coords) == len(pts) and np.all(vm.num == 1)
        np.testing.assert_array_equal(vm.mean, pts[np.lexsort(pts.T[::-1])].astype(np.float64))
    if name == "negative":
        assert vm.coords.min() == -3  # floor(-2.x) = -3; truncation would stop at -2
        assert (np.trunc(pts.astype(np.float64)) != np.floor(pts.astype(np.float64))).any()
    if name == "on_faces":
        np.testing.assert_array_equal(vm.mean, vm.coords * 0.5)  # a point on k * resolution lies in cell k


def test_twin_voxel_map_range():
    far = np.array([[0.0, 0.0, 0.0], [2.0 ** 20, 0.0, 0.0]], np.float32)
    with pytest.raises(ValueError):
        tw.voxel_map(far, np.tile(np.eye(3), (2, 1, 1)), 1.0)
    edge = np.array([[2.0 ** 20 - 1, -(2.0 ** 20), 0.0]], np.float32)
    vm = tw.voxel_map(edge, np.eye(3)[None], 1.0)
    assert tuple(vm.coords[0]) == (2 ** 20 - 1, -(2 ** 20), 0)


def test_twin_offsets():
    assert tw.offsets(tw.DIRECT7) == [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    o = tw.offsets(tw.DIRECT27)
    assert len(o) == 27 and o[0] == (-1, -1, -1) and o[1] == (-1, -1, 0) and o[13] == (0, 0, 0) and o[26] == (1, 1, 1)


# ------------------------------------------------------------------------------- known answers
# (mode, resolution) -> per seed 0, 1, 2 the twin's (translation error m, rotation error rad)
KAT_MEASURED = {
    (tw.DIRECT1, 1.0): [(7.75e-4, 2.36e-5), (5.26e-4, 2.26e-5), (2.04e-4, 1.42e-5)],
    (tw.DIRECT7, 1.0): [(1.138e-2, 2.31e-4), (1.117e-2, 2.34e-4), (1.57e-3, 2.60e-5)],
    (tw.DIRECT27, 0.5): [(2.12e-3, 4.41e-5), (5.69e-3, 1.17e-4), (1.38e-3, 2.16e-5)],
}
KAT_CASES = sorted(KAT_MEASURED)


def _covs(oracle_mod, src, tgt, k=20):
    return (oracle_mod.gicp_covariances(src, k, oracle_mod.GICP_REG_PLANE),
            oracle_mod.gicp_covariances(tgt, k, oracle_mod.GICP_REG_PLANE))


@pytest.mark.parametrize("mode,resolution", KAT_CASES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twin_recovers_known_transform(oracle_mod, seed, mode, resolution):
    src, tgt, T = _scene(seed)
    CA, CB = _covs(oracle_mod, src, tgt)
    r = tw.align(src, tgt, CA, CB, resolution=resolution, mode=mode)
    dt, dr = pose_err(r["T"].astype(np.float32), T)
    print(f"KAT mode {mode} resolution {resolution} seed {seed}: dt {dt:.4e} m dr {dr:.4e} rad, "
          f"iterations {r['iterations']}, correspondences {r['n_valid']}")
    assert r["converged"] and not r["lm_failed"]
    assert dt < TOL_KAT_T and dr < TOL_KAT_R, (dt, dr)
    # the recorded answer (the twin is deterministic up to the BLAS's summation order)
    wt, wr = KAT_MEASURED[(mode, resolution)][seed]
    assert abs(dt - wt) <= 0.02 * wt + 1e-6 and abs(dr - wr) <= 0.02 * wr + 1e-7, (dt, dr, wt, wr)


def test_twin_identity_and_out_of_reach(oracle_mod):
    src, _, _ = _scene(1, 800)
    CA, _ = _covs(oracle_mod, src, src, 5)
    r = tw.align(src, src, CA, CA, resolution=1.0, mode=tw.DIRECT1)
    assert r["converged"] and r["iterations"] == 0 and not r["lm_failed"]
    assert r["n_valid"] == len(src)  # every point finds its own voxel
    dt, dr = pose_err(r["T"], np.eye(4))
    assert dt < 5e-4 and dr < 2e-3  # one step below the convergence epsilons
    # the target out of reach of every neighbourhood: no correspondence, the first step is the identity
    G = np.eye(4, dtype=np.float32)
    G[:3, 3] = [0.25, -0.5, 0.125]
    for mode in (tw.DIRECT1, tw.DIRECT27):
        r = tw.align(src, src + np.float32(100.0), CA, CA, resolution=1.0, mode=mode, guess=G)
        assert r["n_valid"] == 0 and r["converged"] and r["iterations"] == 0 and not r["lm_failed"]
        np.testing.assert_array_equal(r["T"], G.astype(np.float64))


# ------------------------------------------------------------------------------- the interface (no GPU)
def test_abi_version_and_exports():
    import ctypes as C
    import os
    import re

    import icp4r
    from icp4r import vgicp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "icp4r", "icp4r_vgicp.h")).read()
    decl = sorted(re.findall(r"^\s*(?:int|void)\s+(icp4r_\w+)\s*\(", hdr, re.M))
    assert decl == sorted(vgicp.VGICP_EXPORTED_SYMBOLS) and len(decl) == 4
    L = icp4r.load()
    for name in decl:
        assert hasattr(L, name), name
    assert re.search(r"#define\s+ICP4R_ABI_VERSION\s+6\b", open(os.path.join(root, "include", "icp4r", "icp4r.h")).read())
    L.icp4r_abi_version.restype = C.c_int
    assert L.icp4r_abi_version() == 6
    # the defaults and the struct's layout: the GICP parameters first, unchanged
    p = vgicp.default_params()
    assert (p.voxel_resolution, p.neighbor_search, p.voxel_accumulation) == (1.0, vgicp.DIRECT1, vgicp.ADDITIVE)
    assert p.gicp.k_correspondences == 20 and p.gicp.max_iterations == 64
    assert C.sizeof(vgicp.VgicpParams) == C.sizeof(vgicp.GicpParams) + 8 + 4 + 4 + 32
    assert vgicp.default_params(k_correspondences=5, voxel_resolution=0.3).gicp.k_correspondences == 5
