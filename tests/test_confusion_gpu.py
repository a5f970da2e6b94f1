"""common.metrics.confusion_matrix / overlap_metrics / overlap_scores on the HIP kernels (csrc/seg_confusion.hip) against the
numpy forms of tests/confusion_forms.py.

Everything is an integer or a once-rounded fp64 quotient of integers, so every comparison is torch.equal (the NaN masks of the
scores are compared as well as the values): there are no tolerances.

Shapes: less than a wave; tails; one tile plus one voxel; with one entry, exactly two tiles for each of the capped workgroups plus
one voxel (both from ops.CONFUSION_TILE / ops.CONFUSION_MAX_BLOCKS); axes of one.  Class counts on both sides of the limit of the
LDS matrix (ops.CONFUSION_LDS_MAX_K), of the LDS overlap counters (ops.OVERLAP_LDS_MAX_K) and at the largest matrix."""
import functools

import pytest
import torch

from tests.confusion_forms import (SCORES, argmax_form, confusion_form, label_patterns, logits_patterns, overlap_form)
from tests.surface_forms import CASES, case_id, pair_of

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
COUNTS = ["matrix", "pred_only", "target_only", "counted"]


def _M():
    import advchain.common.metrics as M
    return M


def _ops():
    from advchain_amd import ops
    return ops


ONE_TILE, TWO_ROUNDS = (1, 25, 41), (1, 65, 4033)
SMALL = [(2, 5, 7), (3, 36, 57), (2, 6, 10, 70), ONE_TILE, (1, 1, 9), (1, 5, 1, 3)]
SHAPES = SMALL + [TWO_ROUNDS]
LDS_K = 127


def shape_id(shape):
    return "x".join(map(str, shape))


def test_tile_shapes_follow_the_kernel():
    ops = _ops()
    assert ops.CONFUSION_LDS_MAX_K == LDS_K
    one, two = ONE_TILE[1] * ONE_TILE[2], TWO_ROUNDS[1] * TWO_ROUNDS[2]
    assert one == ops.CONFUSION_TILE + 1
    assert TWO_ROUNDS[0] == 1 and two == 2 * ops.CONFUSION_TILE * ops.CONFUSION_MAX_BLOCKS + 1
    assert 3000 > ops.OVERLAP_LDS_MAX_K and ops.CONFUSION_MAX_K == 1024


def _equal_scores(got, want, what):
    got = got.cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), what


def _check_confusion(got, want, what):
    for f in COUNTS:
        t = getattr(got, f)
        assert t.is_cuda and t.dtype == torch.int64 and t.shape == getattr(want, f).shape, (what, f)
        assert torch.equal(t.cpu(), getattr(want, f)), (what, f)


def _check_overlap(got, want, what):
    for f in ("overlap", "counted"):
        t = getattr(got, f)
        assert t.is_cuda and t.dtype == torch.int64 and t.shape == getattr(want, f).shape, (what, f)
        assert torch.equal(t.cpu(), getattr(want, f)), (what, f)
    for s in SCORES:
        _equal_scores(getattr(got, s), getattr(want, s), (what, s))


@functools.lru_cache(maxsize=4)
def _patterns(K, shape):
    return label_patterns(K, shape)


MATRIX_CASES = [(K, s) for s in SHAPES for K in (1, 2, 4, 20, LDS_K, LDS_K + 1)] + [(1024, (2, 5, 7))]


@pytest.mark.parametrize("K,shape", MATRIX_CASES, ids=["K%d-%s" % (K, shape_id(s)) for K, s in MATRIX_CASES])
def test_matrix_from_labels(K, shape):
    M = _M()
    for name, (p, y) in _patterns(K, shape).items():
        pd, yd = p.to(DEV), y.to(DEV)
        for ignore in (None, -100):
            got = M.confusion_matrix(pd, yd, K, ignore_index=ignore)
            assert got.labels is None
            _check_confusion(got, confusion_form(p, y, K, ignore), (name, ignore))


OVERLAP_CASES = [(K, s) for s in SHAPES for K in (1, 2, 4, 20, LDS_K + 1)] + \
                [(1024, (2, 5, 7)), (2048, (2, 5, 7)), (2049, (2, 5, 7)), (3000, (3, 36, 57))]


@pytest.mark.parametrize("K,shape", OVERLAP_CASES, ids=["K%d-%s" % (K, shape_id(s)) for K, s in OVERLAP_CASES])
def test_overlap_from_labels(K, shape):
    M = _M()
    for name, (p, y) in _patterns(K, shape).items():
        pd, yd = p.to(DEV), y.to(DEV)
        for ignore in (None, -100):
            got = M.overlap_metrics(pd, yd, K, ignore_index=ignore)
            assert got.labels is None
            _check_overlap(got, overlap_form(p, y, K, ignore), (name, ignore))


LOGIT_CASES = [(K, s) for s in [(2, 5, 7), (3, 36, 57), (2, 6, 10, 70), ONE_TILE, (1, 5, 1, 3)] for K in (1, 2, 4, 20)] + \
              [(LDS_K + 1, (2, 5, 7)), (4, TWO_ROUNDS)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K,shape", LOGIT_CASES, ids=["K%d-%s" % (K, shape_id(s)) for K, s in LOGIT_CASES])
def test_from_logits(K, shape, dtype):
    """The argmax map equals torch.argmax of the CPU copy; the counts equal the form on it and the label route on those labels."""
    M = _M()
    y = _patterns(K, shape)["blocks_target"][1]
    yd = y.to(DEV)
    for name, x in logits_patterns(K, shape, dtype).items():
        labels = argmax_form(x)
        xd = x.to(DEV)
        for ignore in (None, -100):
            got = M.confusion_matrix(xd, yd, K, ignore_index=ignore, return_labels=True)
            assert got.labels.dtype == torch.int64 and torch.equal(got.labels.cpu(), labels), name
            _check_confusion(got, confusion_form(labels, y, K, ignore), (name, ignore))
            route = M.confusion_matrix(got.labels, yd, K, ignore_index=ignore)
            for f in COUNTS:
                assert torch.equal(getattr(route, f), getattr(got, f)), (name, f)
            assert M.confusion_matrix(xd, yd, K, ignore_index=ignore).labels is None
            o = M.overlap_metrics(xd, yd, K, ignore_index=ignore, return_labels=True)
            assert torch.equal(o.labels.cpu(), labels), name
            _check_overlap(o, overlap_form(labels, y, K, ignore), (name, ignore))
    if K > 1:
        half = {d: logits_patterns(K, shape, d)["half_integers"] for d in (torch.float32, torch.bfloat16)}
        a = M.confusion_matrix(half[torch.float32].to(DEV), yd, K, return_labels=True)
        b = M.confusion_matrix(half[torch.bfloat16].to(DEV), yd, K, return_labels=True)
        assert torch.equal(a.labels, b.labels) and torch.equal(a.matrix, b.matrix)
        ties = (half[torch.float32].max(1).values.unsqueeze(1) == half[torch.float32]).sum(1) > 1
        assert int(ties.sum()) > 0 or ties.numel() < 64                    # (seven values: a tie in one voxel of 7 at K = 2)


def _offset_copy(t):
    """The same values one element further into a fresh storage: no 16-byte access is possible."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("shape", [(4, 36, 56), (2, 6, 10, 72)], ids=shape_id)
def test_offset_and_non_contiguous_inputs_give_the_same_results(shape):
    """Voxel counts that are multiples of four, so that the aligned call takes the 16-byte loads and the views cannot."""
    M = _M()
    K = 4
    p, y = _patterns(K, shape)["blocks_both"]
    pd, yd = p.to(DEV), y.to(DEV)
    want = M.confusion_matrix(pd, yd, K, ignore_index=-100)
    _check_confusion(want, confusion_form(p, y, K, -100), "aligned")
    want_o = M.overlap_metrics(pd, yd, K, ignore_index=-100)
    pt = pd.transpose(1, 2).contiguous().transpose(1, 2)
    yt = yd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not pt.is_contiguous() and not yt.is_contiguous()
    for pv, yv in ((_offset_copy(pd), _offset_copy(yd)), (_offset_copy(pd), yd), (pd, _offset_copy(yd)), (pt, yt)):
        got = M.confusion_matrix(pv, yv, K, ignore_index=-100)
        for f in COUNTS:
            assert torch.equal(getattr(got, f), getattr(want, f)), f
        got_o = M.overlap_metrics(pv, yv, K, ignore_index=-100)
        assert torch.equal(got_o.overlap, want_o.overlap) and torch.equal(got_o.counted, want_o.counted)
    for dtype in (torch.float32, torch.bfloat16):
        x = logits_patterns(K, shape, dtype)["specials"].to(DEV)
        want = M.confusion_matrix(x, yd, K, ignore_index=-100, return_labels=True)
        assert torch.equal(want.labels.cpu(), argmax_form(x))
        xt = x.transpose(1, 2).contiguous().transpose(1, 2)
        assert not xt.is_contiguous()
        for xv, yv in ((_offset_copy(x), yd), (x, _offset_copy(yd)), (_offset_copy(x), _offset_copy(yd)), (xt, yt)):
            got = M.confusion_matrix(xv, yv, K, ignore_index=-100, return_labels=True)
            for f in COUNTS + ["labels"]:
                assert torch.equal(getattr(got, f), getattr(want, f)), (dtype, f)


@pytest.mark.parametrize("K,shape", [(4, (3, 36, 57)), (LDS_K + 1, (2, 6, 10, 70))], ids=["lds", "global"])
def test_reduce_batch_is_the_sum_over_the_entries(K, shape):
    M = _M()
    p, y = _patterns(K, shape)["blocks_both"]
    pd, yd = p.to(DEV), y.to(DEV)
    for ignore in (None, -100):
        per, whole = M.confusion_matrix(pd, yd, K, ignore_index=ignore), M.confusion_matrix(pd, yd, K, ignore_index=ignore, reduce_batch=True)
        for f in COUNTS:
            assert torch.equal(getattr(whole, f), getattr(per, f).sum(0)), f
        _check_confusion(whole, confusion_form(p, y, K, ignore, reduce_batch=True), ignore)
        per, whole = M.overlap_metrics(pd, yd, K, ignore_index=ignore), M.overlap_metrics(pd, yd, K, ignore_index=ignore, reduce_batch=True)
        assert torch.equal(whole.overlap, per.overlap.sum(0)) and torch.equal(whole.counted, per.counted.sum(0))
        _check_overlap(whole, overlap_form(p, y, K, ignore, reduce_batch=True), ignore)


@pytest.mark.parametrize("reduce_batch", [True, False], ids=["dataset", "per-entry"])
def test_out_accumulates_over_batches(reduce_batch):
    M = _M()
    K, dims = 4, (36, 57)
    batches = [_patterns(K, (n,) + dims)[name] for n, name in zip((3, 1, 2) if reduce_batch else (3, 3, 3),
                                                                   ("blocks_both", "uniform", "blocks_target"))]
    acc = None
    for p, y in batches:
        got = M.confusion_matrix(p.to(DEV), y.to(DEV), K, ignore_index=-100, reduce_batch=reduce_batch, out=acc)
        if acc is not None:
            assert all(a is b for a, b in zip(got[:4], acc[:4]))
        acc = got
    forms = [confusion_form(p, y, K, -100, reduce_batch=reduce_batch) for p, y in batches]
    for i, f in enumerate(COUNTS):
        assert torch.equal(getattr(acc, f).cpu(), sum(form[i] for form in forms)), f
    with pytest.raises(ValueError):
        M.confusion_matrix(batches[0][0].to(DEV), batches[0][1].to(DEV), K + 1, reduce_batch=reduce_batch, out=acc)


@pytest.mark.parametrize("K,shape", [(1, (2, 5, 7)), (4, (3, 36, 57)), (20, (2, 6, 10, 70)), (300, (3, 36, 57))],
                         ids=lambda v: shape_id(v) if isinstance(v, tuple) else "K%d" % v)
def test_scores_of_a_matrix_equal_overlap_metrics_when_no_label_is_out_of_range(K, shape):
    M = _M()
    for name in ("one_class", "uniform", "blobs"):
        p, y = _patterns(K, shape)[name]
        pd, yd = p.to(DEV), y.to(DEV)
        want = M.overlap_metrics(pd, yd, K)
        got = M.overlap_scores(M.confusion_matrix(pd, yd, K).matrix)
        assert torch.equal(got.overlap, want.overlap) and torch.equal(got.counted, want.counted), name
        for s in SCORES:
            _equal_scores(getattr(got, s), getattr(want, s).cpu(), (name, s))
        whole = M.overlap_scores(M.confusion_matrix(pd, yd, K, reduce_batch=True).matrix)
        _check_overlap(whole, overlap_form(p, y, K, reduce_batch=True), name)
        stacked = M.overlap_scores(torch.stack([M.confusion_matrix(pd, yd, K).matrix] * 2, 1))
        assert stacked.dice.shape == (shape[0], 2, K) and torch.equal(stacked.overlap[:, 1], want.overlap)


@pytest.mark.parametrize("K,shape", CASES, ids=[case_id(c) for c in CASES])
def test_overlap_and_dice_equal_those_of_the_surface_metrics(K, shape):
    M = _M()
    p, y = pair_of(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    want, got = M.surface_distance_metrics(pd, yd, K), M.overlap_metrics(pd, yd, K)
    assert torch.equal(got.overlap, want.overlap)
    _equal_scores(got.dice, want.dice.cpu(), "dice")


def _bits(result):
    return [None if t is None else (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().clone() for t in result]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_runs_are_bitwise_identical_and_a_captured_graph_replays_them():
    M = _M()
    K, shape = 4, (3, 36, 57)
    p, y = _patterns(K, shape)["blocks_both"]
    other = _patterns(K, shape)["uniform"]
    pd, yd = p.to(DEV), y.to(DEV)
    xd = logits_patterns(K, shape, torch.bfloat16)["specials"].to(DEV)

    def step():
        c = M.confusion_matrix(pd, yd, K, ignore_index=-100)
        o = M.overlap_metrics(xd, yd, K, ignore_index=-100, return_labels=True)
        return tuple(c) + tuple(o) + tuple(M.overlap_scores(c.matrix))

    eager = _bits(step())
    assert _same(eager, _bits(step()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert _same(_bits(static), eager)
    g.replay()
    torch.cuda.synchronize()
    assert _same(_bits(static), eager)
    with torch.no_grad():
        pd.copy_(other[0].to(DEV))
        yd.copy_(other[1].to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert _same(_bits(static), _bits(step()))
    _check_confusion(M.Confusion(*static[:5]), confusion_form(other[0], other[1], K, -100), "new contents")


def test_refusals_on_the_device():
    M = _M()
    y = torch.zeros(2, 4, 6, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        M.confusion_matrix(y, y, 3, return_labels=True)
    with pytest.raises(ValueError):
        M.confusion_matrix(torch.zeros(2, 3, 4, 6, device=DEV, dtype=torch.float16), y, 3)
    with pytest.raises(ValueError):
        M.confusion_matrix(y, y, 3, out=M.Confusion(*[torch.zeros(s, dtype=torch.int64) for s in ((2, 3, 3), (2, 3), (2, 3), (2,))], None))
    x = torch.zeros(2, 3, 4, 6, device=DEV, requires_grad=True)
    got = M.overlap_metrics(x, y, 3)
    assert not got.dice.requires_grad and got.dice[:, 0].tolist() == [1.0, 1.0]
