"""common.metrics.instance_metrics without a GPU: the brute-force form of tests/instance_forms.py on hand-computed cases, the
at-most-one-partner property of the match rule on the random pairs of the GPU tests, and every ValueError of the public function
(the argument checks run before any GPU work)."""
import math

import numpy as np
import pytest
import torch

from tests import instance_forms as F

SHAPE = (1, 5, 7)
ONE = 1 << 32


def _maps():
    return torch.zeros(SHAPE, dtype=torch.int64), torch.zeros(SHAPE, dtype=torch.int64)


def _nan_where(x, where):
    assert np.array_equal(np.isnan(x), where), (x, where)


def test_identical_maps_match_every_component_at_iou_one():
    pred, _ = _maps()
    pred[0, 0, 0:3] = 1
    pred[0, 2:4, 2:4] = 1
    pred[0, 4, 6] = 2
    pred[0, 0, 6] = -100
    b = F.instance_brute(pred, pred.clone(), 3)
    assert b.components[0].tolist() == [[0, 0], [2, 2], [1, 1]]
    assert b.matched[0].tolist() == [0, 2, 1] and b.overlapping[0].tolist() == [[0, 0], [2, 2], [1, 1]]
    assert b.iou_fixed[0].tolist() == [0, 2 * ONE, ONE]
    assert b.pq[0, 1:].tolist() == [1.0, 1.0] and b.sq[0, 1:].tolist() == [1.0, 1.0] and b.f1[0, 1:].tolist() == [1.0, 1.0]
    for q in F.QUOTIENTS:                                                      # the background class: zeros and NaN
        _nan_where(getattr(b, q)[0], np.array([True, False, False]))
    assert np.array_equal(b.pred_status, (pred.numpy() > 0).astype(np.uint8))
    assert np.array_equal(b.target_status, b.pred_status)


@pytest.mark.parametrize("k", [1, 2], ids=["class1", "class2"])
def test_half_overlap_does_not_match_and_three_of_five_matches_below_point_six(k):
    pred, target = _maps()
    pred[0, 1, 1:3] = k                          # two voxels against one of them: IoU == 0.5 exactly
    target[0, 1, 1] = k
    pred[0, 3, 1:6] = k                          # five voxels against three of them: IoU == 0.6
    target[0, 3, 1:4] = k
    at_half = F.instance_brute(pred, target, 3, 0.5)
    assert at_half.components[0, k].tolist() == [2, 2] and at_half.overlapping[0, k].tolist() == [2, 2]
    assert at_half.matched[0, k] == 1 and at_half.pairs[0, k] == 2 and at_half.half_pairs[0, k] == 1
    assert at_half.iou_fixed[0, k] == (3 << 32) // 5
    assert at_half.f1[0, k] == np.float32(0.5) and at_half.precision[0, k] == np.float32(0.5)
    assert at_half.sq[0, k] == np.float32(float((3 << 32) // 5) * 2.0 ** -32)
    assert at_half.pq[0, k] == np.float32(2.0 * float((3 << 32) // 5) * 2.0 ** -32 / 4.0)
    assert at_half.pred_status[0, 1, 1] == 2 and at_half.pred_status[0, 3, 5] == 1 and at_half.target_status[0, 3, 1] == 1
    other = 3 - k
    assert at_half.components[0, other].tolist() == [0, 0] and math.isnan(at_half.f1[0, other])
    above = F.instance_brute(pred, target, 3, 0.6)
    assert above.matched[0, k] == 0 and above.iou_fixed[0, k] == 0 and above.overlapping[0, k].tolist() == [2, 2]
    assert above.f1[0, k] == 0.0 and above.pq[0, k] == 0.0 and math.isnan(above.sq[0, k])
    assert set(above.pred_status[0][pred[0].numpy() > 0].tolist()) == {2}


def test_a_class_in_one_map_only_and_classes_never_pair():
    pred, target = _maps()
    pred[0, 1:3, 1:3] = 1                        # the same voxels, another class: no pair
    target[0, 1:3, 1:3] = 2
    pred[0, 4, 0:2] = 1
    b = F.instance_brute(pred, target, 3)
    assert b.components[0].tolist() == [[0, 0], [2, 0], [0, 1]]
    assert int(b.matched.sum()) == 0 and int(b.overlapping.sum()) == 0 and int(b.pairs.sum()) == 0
    assert b.precision[0, 1] == 0.0 and math.isnan(b.recall[0, 1]) and b.f1[0, 1] == 0.0 and b.pq[0, 1] == 0.0
    assert math.isnan(b.precision[0, 2]) and b.recall[0, 2] == 0.0 and math.isnan(b.sq[0, 2])
    assert set(b.pred_status[0][pred[0].numpy() > 0].tolist()) == {3}


@pytest.mark.parametrize("shape,K", [((3, 36, 57), 3), ((1, 65, 129), 4), ((2, 6, 10, 70), 3)], ids=["3x36x57", "1x65x129", "2x6x10x70"])
def test_a_component_matches_at_most_one_partner(shape, K):
    pred, target = F.lesion_pairs(shape, K, seed=K)
    for c in range(1, len(shape)):
        roots = (F.roots_of(pred, c, 0, K), F.roots_of(target, c, 0, K))
        for threshold in (0.5, 0.55):
            b = F.instance_brute(pred, target, K, threshold, c, roots=roots)
            assert b.most_partners == 1 and int(b.matched.sum()) > 0
            assert np.all(b.matched <= b.overlapping.min(axis=2)) and np.all(b.overlapping <= b.components)
            assert np.all(b.pairs >= b.overlapping.max(axis=2))


def test_the_workspace_query_and_the_argument_checks_of_the_c_abi_run_on_the_host():
    import ctypes
    from advchain_amd import _lib
    lib = _lib.load()
    for N, sp in ((2, (5, 7)), (32, (256, 256)), (4, (128, 128, 64)), (1, (9, 17, 129))):
        V = int(np.prod(sp))
        words = N * (3 * max(2 * V, 64) + 6 * V + 2 * -(-V // 2048))          # table, state words, two labelling workspaces
        assert lib.advchain_instance_match_workspace(N, len(sp), _lib.dims_array(sp)) == words
        assert lib.advchain_components_workspace(N, len(sp), _lib.dims_array(sp)) == N * (2 * V + -(-V // 2048))
        if V >= 2048:                                                           # (8 bytes per started chunk of 2048 voxels)
            assert 48.0 < 4.0 * words / (N * V) < 48.01                         # the bytes per voxel DESIGN.md states
    assert lib.advchain_instance_match_workspace(64, 3, _lib.dims_array((512, 512, 512))) == -1
    assert lib.advchain_instance_match_workspace(0, 2, _lib.dims_array((8, 8))) == -1
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    dims = _lib.dims_array((2, 2))

    def call(K=2, connectivity=1, threshold=0.5, pred=p):
        return lib.advchain_instance_match(pred, p, p, p, p, p, p, p, p, p, p, None, None, p, 1, K, 2, dims, connectivity, 0,
                                           threshold, None)

    for kwargs, word in ((dict(K=0), b"K must be"), (dict(K=65536), b"K must be"), (dict(threshold=0.49), b"iou_threshold"),
                         (dict(threshold=1.0), b"iou_threshold"), (dict(threshold=float("nan")), b"iou_threshold"),
                         (dict(connectivity=3), b"connectivity"), (dict(pred=None), b"null pointer")):
        assert call(**kwargs) == -1 and word in lib.advchain_last_error(), kwargs


def test_every_value_error_comes_before_any_gpu_work():
    import advchain.common.metrics as M
    y = torch.zeros(1, 5, 7, dtype=torch.int64)
    for bad in (0.49, 1.0, float("nan"), float("inf"), True, "0.5", None):
        with pytest.raises(ValueError, match="iou_threshold"):
            M.instance_metrics(y, y, 2, iou_threshold=bad)
    with pytest.raises(ValueError, match="differ in shape"):
        M.instance_metrics(y, torch.zeros(1, 5, 8, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="labels"):
        M.instance_metrics(torch.zeros(5, 7, dtype=torch.int64), torch.zeros(5, 7, dtype=torch.int64), 2)
    for bad in (0, 3, True, 1.0):
        with pytest.raises(ValueError, match="connectivity"):
            M.instance_metrics(y, y, 2, connectivity=bad)
    with pytest.raises(ValueError, match="background"):
        M.instance_metrics(y, y, 2, background=0.5)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="num_classes"):
            M.instance_metrics(y, y, bad)
    with pytest.raises(NotImplementedError):
        M.instance_metrics(y, y, 65536)
    with pytest.raises(M.ops._lib.AdvchainHipError):                            # valid arguments: only the device is missing
        M.instance_metrics(y, y, 2)
    assert M.InstanceMetrics is M.ops.InstanceMetrics and M.InstanceMetrics._fields[:4] == F.INTEGERS
