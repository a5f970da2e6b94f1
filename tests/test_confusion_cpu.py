"""common.metrics.confusion_matrix / overlap_metrics / overlap_scores without a GPU: the numpy forms of tests/confusion_forms.py
against sklearn and against hand cases whose answers are written out, the identities between the matrix and the set sizes, the
argmax rule the kernel documents (torch.argmax on the CPU), every refusal of the Python layer (all before any GPU work) and the
argument checks of the C entries."""
import ctypes

import numpy as np
import pytest
import torch

from tests.confusion_forms import (SCORES, argmax_form, confusion_form, label_patterns, logits_patterns, overlap_form, scores_form,
                                   table_form)


def _M():
    import advchain.common.metrics as M
    return M


@pytest.mark.parametrize("K,shape", [(2, (2, 5, 7)), (4, (3, 36, 57)), (20, (2, 6, 10, 70))])
def test_form_against_sklearn(K, shape):
    sk = pytest.importorskip("sklearn.metrics")
    g = torch.Generator().manual_seed(K)
    p, y = torch.randint(0, K, shape, generator=g), torch.randint(0, K, shape, generator=g)
    got = confusion_form(p, y, K)
    for n in range(shape[0]):
        want = sk.confusion_matrix(y[n].reshape(-1).numpy(), p[n].reshape(-1).numpy(), labels=list(range(K)))
        assert np.array_equal(got.matrix[n].numpy(), want)
    assert int(got.pred_only.sum()) == 0 and int(got.target_only.sum()) == 0
    assert got.counted.tolist() == [p[0].numel()] * shape[0]
    whole = confusion_form(p, y, K, reduce_batch=True)
    assert np.array_equal(whole.matrix.numpy(), sk.confusion_matrix(y.reshape(-1).numpy(), p.reshape(-1).numpy(), labels=list(range(K))))


def test_form_on_hand_cases():
    K = 3
    #                     v: 0  1  2  3     4  5     6    7
    y = torch.tensor([[[0, 0, 1, 2, -100, 1, K + 3, -100]]])
    p = torch.tensor([[[0, 1, 1, 0, 2, K + 3, 2, -100]]])
    off = confusion_form(p, y, K)                       # nothing left out: -100 is a counted voxel of no class
    assert off.matrix.tolist() == [[[1, 1, 0], [0, 1, 0], [1, 0, 0]]]
    assert off.pred_only.tolist() == [[0, 0, 2]]        # v4 (target -100) and v6 (target K + 3) predicted as class 2
    assert off.target_only.tolist() == [[0, 1, 0]]      # v5: target 1, pred K + 3
    assert off.counted.tolist() == [8]
    on = confusion_form(p, y, K, ignore_index=-100)     # v4 and v7 left out
    assert on.matrix.tolist() == off.matrix.tolist()
    assert on.pred_only.tolist() == [[0, 0, 1]]
    assert on.target_only.tolist() == [[0, 1, 0]]
    assert on.counted.tolist() == [6]
    o = overlap_form(p, y, K, ignore_index=-100)
    assert o.overlap.tolist() == [[[2, 2, 1], [2, 2, 1], [1, 1, 0]]]      # |A|, |B|, |A n B| of classes 0, 1, 2
    # class 0: TP 1, FP 1, FN 1, TN 6 - 3 = 3
    assert o.dice[0].tolist() == [0.5, 0.5, 0.0]
    assert torch.equal(o.iou[0], torch.tensor([1 / 3, 1 / 3, 0.0], dtype=torch.float64).float())
    assert o.precision[0].tolist() == [0.5, 0.5, 0.0] and o.recall[0].tolist() == [0.5, 0.5, 0.0]
    assert o.specificity[0].tolist() == [0.75, 0.75, 0.800000011920929]   # class 2: TN 4, FP 1
    ignore_pred = confusion_form(p, y, K, ignore_index=K + 3)             # ignore_index looks at the target only: v6 goes
    assert ignore_pred.counted.tolist() == [7] and ignore_pred.target_only.tolist() == [[0, 1, 0]]
    empty = overlap_form(torch.zeros(1, 1, 4, dtype=torch.int64), torch.zeros(1, 1, 4, dtype=torch.int64), 2)
    assert empty.dice[0, 0] == 1 and all(torch.isnan(getattr(empty, s)[0, 1]) for s in SCORES[:4])
    assert torch.isnan(empty.specificity[0, 0]) and empty.specificity[0, 1] == 1      # class 0: every counted voxel is in B


@pytest.mark.parametrize("ignore", [None, -100])
@pytest.mark.parametrize("K,shape", [(1, (2, 5, 7)), (4, (3, 36, 57)), (20, (2, 6, 10, 70)), (4, (1, 5, 1, 3))])
def test_identities(K, shape, ignore):
    for name, (p, y) in label_patterns(K, shape).items():
        c = confusion_form(p, y, K, ignore)
        o = overlap_form(p, y, K, ignore)
        keep = torch.ones_like(y, dtype=torch.bool) if ignore is None else y != ignore
        for k in range(K):
            a = ((p == k) & keep).flatten(1).sum(1)
            b = ((y == k) & keep).flatten(1).sum(1)
            assert torch.equal(c.matrix[:, :, k].sum(1) + c.pred_only[:, k], a), name
            assert torch.equal(c.matrix[:, k, :].sum(1) + c.target_only[:, k], b), name
            assert torch.equal(o.overlap[:, k, 0], a) and torch.equal(o.overlap[:, k, 1], b), name
            assert torch.equal(o.overlap[:, k, 2], ((p == k) & (y == k) & keep).flatten(1).sum(1)), name
        total = c.matrix.sum((1, 2)) + c.pred_only.sum(1) + c.target_only.sum(1)
        assert bool((total <= c.counted).all()), name
        assert torch.equal(c.counted, keep.flatten(1).sum(1)), name
        if name in ("one_class", "uniform", "blobs"):
            assert torch.equal(total, c.counted), name
            again = scores_form(o.overlap, c.matrix.sum((1, 2)))
            for s, t in zip(SCORES, again):
                assert torch.equal(torch.nan_to_num(t, nan=-1.0), torch.nan_to_num(getattr(o, s), nan=-1.0)), (name, s)


def test_the_argmax_rule_is_that_of_torch_on_the_cpu():
    inf, nan = float("inf"), float("nan")
    rows = torch.tensor([[1.0, 3.0, 3.0, 2.0],          # the first maximum
                         [0.0, nan, inf, nan],          # a NaN is above +inf; the first NaN
                         [-inf, -inf, -inf, -inf],      # all -inf: class 0
                         [inf, 1.0, inf, 0.0],
                         [-inf, -1.0, -1.0, -inf],
                         [nan, nan, nan, nan]])
    want = [1, 1, 0, 0, 1, 0]
    for dtype in (torch.float32, torch.bfloat16):
        logits = rows.t().reshape(1, 4, 1, 6).to(dtype)
        assert argmax_form(logits).reshape(-1).tolist() == want
    for K in (2, 4, 20):                                # half-integers are exact in bf16: the same argmax in both dtypes
        f = logits_patterns(K, (2, 9, 11), torch.float32)["half_integers"]
        b = logits_patterns(K, (2, 9, 11), torch.bfloat16)["half_integers"]
        assert torch.equal(b.float(), f) and torch.equal(argmax_form(b), argmax_form(f))


def test_value_errors_come_before_any_gpu_work():
    M = _M()
    y = torch.zeros(2, 4, 6, dtype=torch.int64)
    logits = torch.zeros(2, 3, 4, 6)
    for fn in (M.confusion_matrix, M.overlap_metrics):
        for bad in (lambda: fn(y[:, :3], y, 3),                                    # shapes
                    lambda: fn(y, y[0], 3),
                    lambda: fn(y.reshape(2, 2, 2, 3, 2), y.reshape(2, 2, 2, 3, 2), 3),
                    lambda: fn(logits[:, :, :3], y, 3),
                    lambda: fn(logits[:1], y, 3),
                    lambda: fn(y[:, :0], y[:, :0], 3),
                    lambda: fn(logits, y, 4),                                      # K != num_classes
                    lambda: fn(logits.half(), y, 3),                               # dtypes
                    lambda: fn(logits.double(), y, 3),
                    lambda: fn(y.int(), y, 3),
                    lambda: fn(y, y.int(), 3),
                    lambda: fn(y, y.float(), 3),
                    lambda: fn([[0]], y, 3),
                    lambda: fn(y, y, 0),
                    lambda: fn(y, y, 3.0),
                    lambda: fn(y, y, True),
                    lambda: fn(y, y, 3, return_labels=True),                       # a label map is its own argmax
                    lambda: fn(y, y, 3, ignore_index=True),
                    lambda: fn(y, y, 3, ignore_index=-100.0),
                    lambda: fn(y, y, 3, ignore_index=2 ** 63)):
            with pytest.raises(ValueError):
                bad()
    with pytest.raises(ValueError, match="overlap_metrics"):
        M.confusion_matrix(y, y, 1025)
    C = M.Confusion
    z = lambda *s: torch.zeros(s, dtype=torch.int64)
    for out, reduce_batch in ((C(z(2, 3, 3), z(2, 3), z(2, 3), z(2), None), True),            # the shapes of the other mode
                              (C(z(3, 3), z(3), z(3), z(), None), False),
                              (C(z(2, 3, 3), z(2, 3), z(2, 4), z(2), None), False),
                              (C(z(2, 3, 3).int(), z(2, 3), z(2, 3), z(2), None), False),
                              (C(z(2, 3, 6)[:, :, ::2], z(2, 3), z(2, 3), z(2), None), False),
                              ((z(2, 3, 3), z(2, 3), z(2, 3), z(2), None), False),
                              (z(2, 3, 3), False)):
        with pytest.raises(ValueError):
            M.confusion_matrix(y, y, 3, reduce_batch=reduce_batch, out=out)
    for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(2, 3, 3),
                torch.zeros(0, 3, 3, dtype=torch.int64), [[1]]):
        with pytest.raises(ValueError):
            M.overlap_scores(bad)


def test_cpu_tensors_are_refused():
    from advchain_amd import _lib
    M = _M()
    y = torch.zeros(2, 4, 6, dtype=torch.int64)
    C = M.Confusion
    out = C(torch.zeros(2, 3, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64),
            torch.zeros(2, dtype=torch.int64), None)
    for call in (lambda: M.confusion_matrix(y, y, 3), lambda: M.confusion_matrix(torch.zeros(2, 3, 4, 6), y, 3, return_labels=True),
                 lambda: M.confusion_matrix(y, y, 3, out=out), lambda: M.overlap_metrics(y, y, 3, ignore_index=-100),
                 lambda: M.overlap_metrics(torch.zeros(2, 3, 4, 6, dtype=torch.bfloat16), y, 3),
                 lambda: M.overlap_scores(torch.zeros(3, 3, dtype=torch.int64))):
        with pytest.raises(_lib.AdvchainHipError):
            call()


def test_constants_follow_the_kernel():
    from advchain_amd import _lib, ops
    lib = _lib.load()
    got = [lib.advchain_confusion_limit(i) for i in range(5)]
    assert got == [ops.CONFUSION_TILE, ops.CONFUSION_MAX_BLOCKS, ops.CONFUSION_LDS_MAX_K, ops.CONFUSION_MAX_K, ops.OVERLAP_LDS_MAX_K]
    assert lib.advchain_confusion_limit(5) == -1 and lib.advchain_confusion_limit(-1) == -1
    assert 4 * (ops.CONFUSION_LDS_MAX_K + 1) ** 2 <= 160 * 1024 // 2          # two workgroups' tables in the LDS of a CU
    assert 2 * ops.CONFUSION_TILE * ops.CONFUSION_MAX_BLOCKS + 1 <= 300000     # the largest test shape stays small


def test_c_entries_check_their_arguments():
    from advchain_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    dims = _lib.dims_array((4, 4))

    def confusion(pred=p, kind=0, target=p, labels=None, matrix=p, N=1, K=2, ndim=2, dims=dims, has_ignore=0, flags=0):
        return lib.advchain_confusion(pred, kind, target, labels, matrix, p, p, p, N, K, ndim, dims, has_ignore, -100, flags, None)

    def overlap(pred=p, kind=0, target=p, labels=None, dice=p, N=1, K=2, ndim=2, dims=dims, has_ignore=0, flags=0):
        return lib.advchain_overlap(pred, kind, target, labels, p, p, dice, p, p, p, p, N, K, ndim, dims, has_ignore, -100, flags, None)

    for fn, word in ((confusion, b"confusion"), (overlap, b"overlap")):
        for kwargs in (dict(pred=None), dict(target=None), dict(kind=3), dict(kind=-1), dict(labels=p), dict(kind=1, labels=odd),
                       dict(target=odd), dict(pred=odd), dict(K=0), dict(N=0), dict(N=65536), dict(ndim=1), dict(ndim=4),
                       dict(dims=None), dict(dims=_lib.dims_array((4, 0))), dict(has_ignore=2), dict(flags=4), dict(flags=-1)):
            rc = fn(**kwargs)
            assert rc == -1 and word in lib.advchain_last_error(), kwargs
    assert confusion(K=1025) == -1 and b"1..1024" in lib.advchain_last_error()
    assert confusion(matrix=None) == -1 and confusion(matrix=odd) == -1
    assert overlap(K=65536) == -1 and b"1..65535" in lib.advchain_last_error()
    assert overlap(dice=None) == -1
    assert overlap(flags=2) == -1 and b"cleared" in lib.advchain_last_error()

    def scores(matrix=p, overlap=p, R=1, K=2):
        return lib.advchain_overlap_scores(matrix, overlap, p, p, p, p, p, p, R, K, None)

    for kwargs in (dict(matrix=None), dict(overlap=None), dict(matrix=odd), dict(R=0), dict(K=0), dict(K=65536), dict(R=2 ** 31),
                   dict(R=2 ** 20, K=1024)):
        assert scores(**kwargs) == -1 and b"overlap_scores" in lib.advchain_last_error(), kwargs
