"""Map-maintenance semantics of the scan-to-map store, pinned to the reference's own code: ikd-Tree's
Delete_Point_Boxes, Box_Search, Radius_Search and Add_Points(.., true).

tests/golden/ikd_edit.npz holds outputs recorded from the vendored third_party/ikd-Tree
(tests/golden/make_ikd_golden.md).  tests/map_edit_twin.py, a sequential numpy restatement of the rules,
must reproduce every recorded array exactly; it is the checker a device implementation of these calls
is to be held to (rows, order and counts; the intensity carries the point's index, as in
tests/test_map_exact.py).  The store itself does not implement the calls yet.
"""
import os

import numpy as np
import pytest

import map_edit_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ikd_edit.npz")
CASES = ("a", "b", "c", "d")  # 600 + 900 and 1,400 + 3,000 points, ds 0.5 and 0.3
F = np.float32
ALL = np.array([-np.inf] * 3 + [np.inf] * 3, F)


@pytest.fixture(scope="module")
def fx():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _indexed(xyz, first=0):
    out = np.zeros((len(xyz), 4), F)
    out[:, :3] = xyz
    out[:, 3] = np.arange(first, first + len(xyz), dtype=F)
    return out


def _case(fx, c):
    b, a = fx[f"{c}_build"], fx[f"{c}_add"]
    return _indexed(b), _indexed(a, len(b)), float(fx[f"{c}_ds"])


# ---------------------------------------------------------------------------------------------- CPU
def test_twin_matches_reference_fixture(fx):
    """The sequential twin reproduces every array recorded from the reference's ikd-Tree, exactly."""
    for c in CASES:
        store, add, ds = _case(fx, c)
        s, counter = tw.add_points_downsample(store, add, ds)
        assert counter == int(fx[f"{c}_counter"]), c
        assert np.array_equal(s[:, 3].astype(np.int32), fx[f"{c}_survivors"]), c
        r = tw.radius_search(s, fx["center"], fx["radius"])
        assert np.array_equal(r[:, 3].astype(np.int32), fx[f"{c}_radius"]), c
        left, deleted = tw.delete_boxes(s, fx["boxes"])
        assert deleted == int(fx[f"{c}_deleted"]), c
        assert np.array_equal(left[:, 3].astype(np.int32), fx[f"{c}_after_delete"]), c
        assert np.array_equal(tw.box_search(s, ALL), s)


def test_fixture_inputs_respect_conditions(fx):
    """The recorded inputs: sizes, at most 1e-3 of each cloud removed by the generator, ds = 0.3 points at
    least 1e-4 ds from box faces, no point with d^2 within 1e-5 (relative) of the radius query's r^2."""
    assert os.path.getsize(GOLDEN) < 256 * 1024
    r2 = float(fx["radius"]) ** 2
    for c, (nb, na) in zip(CASES, ((600, 900), (600, 900), (1400, 3000), (1400, 3000))):
        b, a, ds = fx[f"{c}_build"], fx[f"{c}_add"], float(fx[f"{c}_ds"])
        assert (len(b), len(a)) == (nb, na) and ds == float(F(0.5 if c in "ac" else 0.3))
        rb, ra = fx[f"{c}_removed"]
        assert rb <= 1e-3 * nb and ra <= 1e-3 * na, (c, rb, ra)
        for p in (b, a):
            d2 = tw.calc_dist(p, fx["center"]).astype(np.float64)
            assert (np.abs(d2 - r2) > 1e-5 * r2).all()
            if ds != 0.5:
                q = p.astype(np.float64) / ds
                assert (np.abs(q - np.round(q)) >= 1e-4).all()
        assert int(fx[f"{c}_counter"]) > 0 and len(fx[f"{c}_survivors"]) < nb + na  # boxes do collide


def test_twin_known_answers():
    """The rules' consequences (tests/map_edit_twin.py), stated on the twin."""
    e = np.zeros((0, 4), F)
    mid = [0.25, 0.25, 0.25]
    near, far = [0.26, 0.25, 0.25, 1], [0.4, 0.25, 0.25, 2]
    s, k = tw.add_points_downsample(e, np.array([far, near], F), 0.5)
    assert k == 2 and s[:, 3].tolist() == [1.0]
    s, k = tw.add_points_downsample(np.array([near], F), np.array([far], F), 0.5)  # lone nearer holder
    assert k == 0 and s[:, 3].tolist() == [1.0]
    a, b = [0.25 - 0.125, 0.25, 0.25, 1], [0.25 + 0.125, 0.25, 0.25, 2]  # mirrored about the centre: a tie
    assert tw.calc_dist(np.array(a, F), np.array(mid, F)) == tw.calc_dist(np.array(b, F), np.array(mid, F))
    s, k = tw.add_points_downsample(e, np.array([a, b], F), 0.5)
    assert k == 2 and s[:, 3].tolist() == [2.0]  # the later arrival
    s, k = tw.add_points_downsample(np.array([a], F), np.array([b], F), 0.5)
    assert k == 1 and s[:, 3].tolist() == [2.0]  # an arrival beats the holder on a tie
    s, k = tw.add_points_downsample(np.array([near], F), np.array([[0.26 + 4e-7, 0.25, 0.25, 9]], F), 0.5)
    assert k == 1 and s[:, 3].tolist() == [1.0]  # same_point: counted, the stored point's values stay
    s, d = tw.delete_boxes(np.array([[0, 0, 0, 0], [1, 1, 1, 1]], F), [[0, 0, 0, 1, 1, 1]])
    assert d == 1 and s[:, 3].tolist() == [1.0]  # on min: deleted; on max: kept
