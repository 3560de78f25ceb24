"""A map store may outlive its context (include/icp4r/icp4r_map.h): icp4r_destroy frees the device side
of the context's maps and detaches them; a detached map refuses every call and its destroy only frees
the host struct.  These tests own their contexts — the session's gpu_ctx is never closed here.
"""
import numpy as np
import pytest

ALL = np.array([-np.inf] * 3 + [np.inf] * 3, np.float32)
DETACHED = "the map's context was destroyed"


def _ten():
    pts = np.zeros((10, 4), np.float32)
    pts[:, 0] = np.arange(10)
    pts[:, 3] = np.arange(10)
    return pts


@pytest.fixture
def own_ctx():
    import torch

    import icp4r

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime first, as in the session fixture
    torch.cuda.synchronize()
    made = []

    def make():
        made.append(icp4r.Context(0))
        return made[-1]

    yield make
    for c in made:
        c.close()  # a second close is a no-op


@pytest.mark.gpu
def test_context_closed_before_its_tree(own_ctx):
    import icp4r
    from icp4r.mapstore import KD_TREE

    ctx = own_ctx()
    tree = KD_TREE(ctx=ctx)
    try:
        tree.Build(_ten())
        assert tree.size() == 10 and len(tree.Box_Search(ALL)) == 10
        ctx.close()
        for call in (tree.size, lambda: tree.Box_Search(ALL), lambda: tree.Radius_Search([0, 0, 0], 1.0),
                     lambda: tree.Build(_ten()), lambda: tree.Add_Points(_ten()), lambda: tree.Delete_Point_Boxes(ALL),
                     tree.points_device, tree.time_ms):
            with pytest.raises(icp4r.ICP4RError, match=DETACHED) as e:
                call()
            assert e.value.code == icp4r.E_INVALID
    finally:
        tree.close()
    assert not tree.handle
    tree.close()  # a second close is a no-op


@pytest.mark.gpu
def test_tree_closed_before_its_context(own_ctx):
    from icp4r.mapstore import KD_TREE

    ctx = own_ctx()
    tree = KD_TREE(ctx=ctx)
    try:
        tree.Build(_ten())
        assert np.array_equal(tree.Box_Search(ALL), _ten())
    finally:
        tree.close()
    ctx.close()
    tree.close()


@pytest.mark.gpu
def test_two_maps_one_closed_before_and_one_after_the_context(own_ctx):
    import icp4r
    from icp4r.mapstore import KD_TREE

    ctx = own_ctx()
    first, second = KD_TREE(ctx=ctx), KD_TREE(ctx=ctx)
    try:
        first.Build(_ten())
        second.Build(_ten()[:4])
        first.close()
        assert second.size() == 4 and np.array_equal(second.Box_Search(ALL), _ten()[:4])
        ctx.close()
        with pytest.raises(icp4r.ICP4RError, match=DETACHED):
            second.size()
    finally:
        first.close()
        second.close()
    # the context is gone; a new one on the same device works and so does a tree on it
    ctx2 = own_ctx()
    third = KD_TREE(ctx=ctx2)
    try:
        third.Build(_ten())
        assert third.size() == 10
    finally:
        third.close()
