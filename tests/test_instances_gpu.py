"""common.metrics.instance_metrics on the HIP kernels (csrc/seg_components.hip: the labelling passes, then k_inst_pair / k_inst_match
/ k_inst_finish / k_inst_status) against the brute-force form of tests/instance_forms.py.  The integers are compared with
torch.equal; the fp32 quotients too, against the fp64-then-fp32 brute force, with the NaN positions compared separately.

Shapes: smaller than a wave, tails in both axes, one axis far longer than any tile, several slabs, and per dimensionality the one
with exactly two tiles along every tiled axis plus one voxel, from ops.COMPONENTS_TILE: (1, 65, 129) and (1, 9, 17, 129).  Every
case runs at every connectivity valid for its rank."""
import functools

import numpy as np
import pytest
import torch

from tests import components_forms as C
from tests import instance_forms as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")

SHAPES = [(2, 5, 7), (3, 36, 57), (1, 65, 129), (1, 600, 9), (2, 6, 10, 70), (1, 9, 17, 129), (1, 20, 20, 40)]
SHAPE_IDS = [C.shape_id(s) for s in SHAPES]
TWO_TILES = [(1, 65, 129), (1, 9, 17, 129)]
# (2, 5, 7) is two cells of the lesion generator: too few for every kind of pair to turn up, it runs without the non-vacuity check
RICH = [s for s in SHAPES if s != (2, 5, 7)]


def _M():
    import advchain.common.metrics as M
    return M


def test_tile_shapes_follow_the_kernel():
    from advchain_amd import ops
    assert [C.two_tiles_and_one(ops.COMPONENTS_TILE[nd]) for nd in (2, 3)] == TWO_TILES
    assert all(s in SHAPES for s in TWO_TILES)


def _classes(shape):
    return 4 if shape in TWO_TILES else 3


@functools.lru_cache(maxsize=None)
def _pair(name, shape):
    """(pred, target, K) on the CPU; never modified."""
    if name == "lesion":
        K = _classes(shape)
        return F.lesion_pairs(shape, K, seed=K) + (K,)
    if name in ("percolation", "sparse"):                                       # (0.59 is one cluster on the cubic lattice: 0.32 too)
        x = C.percolation(shape) if name == "percolation" else C.percolation(shape, p=0.32)
        return x, F.flipped(x, 0.03, seed=3), 2
    if name == "alternating":
        x = F.alternating(shape)
        return x, x.clone(), 3
    if name == "boards":                                                        # classes 1 and 2 against 2 and 1: no voxel agrees
        x = 1 + C.checkerboard(shape)
        return x, 3 - x, 3
    if name == "three":
        return C.three_classes(shape, seed=2), C.three_classes(shape, seed=5), 3
    if name == "background":
        return torch.zeros(shape, dtype=torch.int64), torch.zeros(shape, dtype=torch.int64), 3
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _roots(name, shape, connectivity, background, K):
    pred, target, _ = _pair(name, shape)
    return F.roots_of(pred, connectivity, background, K), F.roots_of(target, connectivity, background, K)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, connectivity, threshold=0.5, background=0, K=None):
    pred, target, K0 = _pair(name, shape)
    K = K0 if K is None else K
    return F.instance_brute(pred, target, K, threshold, connectivity, background, roots=_roots(name, shape, connectivity, background, K))


def _connectivities(shape):
    return range(1, len(shape))


def _check(got, want, shape, K, what, maps=True):
    M = _M()
    N = shape[0]
    assert isinstance(got, M.InstanceMetrics), what
    for name in F.INTEGERS:
        g, w = getattr(got, name), torch.from_numpy(getattr(want, name))
        assert g.dtype == torch.int64 and g.is_cuda and g.shape == w.shape, (what, name)
        assert torch.equal(g.cpu(), w), (what, name, g.cpu().tolist(), w.tolist())
    for name in F.QUOTIENTS:
        g, w = getattr(got, name), torch.from_numpy(getattr(want, name))
        assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == (N, K), (what, name)
        g = g.cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, name, g.tolist(), w.tolist())
        assert torch.equal(torch.nan_to_num(g, nan=-1.0), torch.nan_to_num(w, nan=-1.0)), (what, name, g.tolist(), w.tolist())
    if maps:
        for name in ("pred_status", "target_status"):
            g, w = getattr(got, name), torch.from_numpy(getattr(want, name))
            assert g.dtype == torch.uint8 and g.is_cuda and tuple(g.shape) == shape, (what, name)
            assert torch.equal(g.cpu(), w), (what, name)
    else:
        assert got.pred_status is None and got.target_status is None, what


def _run(name, shape, threshold=0.5, background=0, K=None, connectivities=None):
    M = _M()
    pred, target, K0 = _pair(name, shape)
    K = K0 if K is None else K
    pd, td = pred.to(DEV), target.to(DEV)
    refs = {}
    for c in connectivities or _connectivities(shape):
        what = "%s %s connectivity %d threshold %r" % (name, shape, c, threshold)
        want = _reference(name, shape, c, threshold, background, K)
        got = M.instance_metrics(pd, td, K, iou_threshold=threshold, connectivity=c, background=background, return_maps=True)
        _check(got, want, shape, K, what)
        refs[c] = want
    return refs


def _total(b):
    return dict(TP=int(b.matched.sum()), nP=int(b.components[..., 0].sum()), nT=int(b.components[..., 1].sum()),
                overlap_p=int(b.overlapping[..., 0].sum()), overlap_t=int(b.overlapping[..., 1].sum()), pairs=int(b.pairs.sum()),
                half=int(b.half_pairs.sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("threshold", [0.5, 0.55])
def test_lesion_pairs(threshold, shape):
    refs = _run("lesion", shape, threshold)
    if shape not in RICH:
        return
    for c, b in refs.items():
        t = _total(b)                                                          # the reference itself: the case is not vacuous
        assert t["TP"] > 0 and t["nP"] - t["TP"] > 0 and t["nT"] - t["TP"] > 0, (c, t)
        assert t["overlap_p"] > t["TP"] and t["overlap_t"] > t["TP"], (c, t)
        assert t["pairs"] > t["overlap_p"] and t["pairs"] > t["overlap_t"], (c, t)   # a one-to-many overlap in both directions
        assert b.most_partners == 1
        if len(shape) == 3:
            assert t["half"] > 0, (c, t)                                        # IoU == 0.5 exactly: the strict inequality decides


def test_the_two_thresholds_differ_in_the_reference():
    differ = [shape for shape in RICH
              if _total(_reference("lesion", shape, 1, 0.5))["TP"] != _total(_reference("lesion", shape, 1, 0.55))["TP"]]
    assert differ, "no lesion case has a pair with an IoU in (0.5, 0.55]"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_large_tortuous_clusters(shape):
    refs = _run("percolation", shape)
    if shape in RICH:
        assert any(_total(b)["pairs"] > max(_total(b)["overlap_p"], _total(b)["overlap_t"]) for b in refs.values())
    if len(shape) == 4:
        _run("sparse", shape)


@pytest.mark.parametrize("shape", TWO_TILES, ids=[C.shape_id(s) for s in TWO_TILES])
def test_the_table_holds_one_pair_per_voxel_and_none(shape):
    V = int(np.prod(shape[1:]))
    b = _run("alternating", shape, connectivities=[1])[1]                       # every voxel a component and a pair of its own
    assert int(b.pairs.sum()) == V and int(b.matched.sum()) == V and int(b.iou_fixed.sum()) == V << 32
    assert int((b.pred_status == 1).sum()) == V
    _run("alternating", shape)                                                  # (two components from connectivity 2 on)
    for c, b in _run("boards", shape).items():
        assert int(b.pairs.sum()) == 0 and int(b.matched.sum()) == 0, c
        assert int((b.pred_status == 3).sum()) == V and int((b.target_status == 3).sum()) == V, c


def test_entries_do_not_mix():
    M = _M()
    shape = (1, 36, 57)
    singles = [_pair(name, shape)[:2] for name in ("lesion", "percolation", "alternating")]
    pred = torch.cat([p for p, _ in singles]).to(DEV)
    target = torch.cat([t for _, t in singles]).to(DEV)
    for c in (1, 2):
        whole = M.instance_metrics(pred, target, 3, connectivity=c, return_maps=True)
        parts = [M.instance_metrics(pred[n:n + 1], target[n:n + 1], 3, connectivity=c, return_maps=True) for n in range(3)]
        for name in M.InstanceMetrics._fields:
            a, b = getattr(whole, name), torch.cat([getattr(p, name) for p in parts])
            assert torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0)), (name, c)
        assert int(whole.matched.sum()) > 0


@pytest.mark.parametrize("shape", [(3, 36, 57), (2, 6, 10, 70)], ids=["2d", "3d"])
def test_conventions(shape):
    refs = _run("three", shape, background=2)                                   # class 0 is a class, class 2 is not
    assert all(int(b.components[:, 2].sum()) == 0 and int(b.components[:, 0].sum()) > 0 for b in refs.values())
    _run("percolation", shape, K=1, background=1)                               # K = 1: the voxels of class 0
    refs = _run("percolation", shape, K=1)                                      # ... and with class 0 the background: nothing
    assert all(int(b.components.sum()) == 0 and np.isnan(b.f1).all() for b in refs.values())
    refs = _run("lesion", shape, K=5)                                           # classes 3 and 4 are in neither map
    for b in refs.values():
        assert int(b.components[:, 3:].sum()) == 0 and all(np.isnan(getattr(b, q)[:, 3:]).all() for q in F.QUOTIENTS)
    refs = _run("background", shape)
    assert all(int(b.components.sum()) == 0 and int((b.pred_status != 0).sum()) == 0 for b in refs.values())


def test_the_status_maps_are_optional():
    shape = (3, 36, 57)
    pred, target, K = _pair("lesion", shape)
    got = _M().instance_metrics(pred.to(DEV), target.to(DEV), K)
    _check(got, _reference("lesion", shape, 1), shape, K, "no maps", maps=False)


def test_two_calls_give_the_same_bits():
    M = _M()
    for shape in ((1, 65, 129), (1, 20, 20, 40)):
        pred, target, K = _pair("percolation", shape)
        pred, target = pred.to(DEV), target.to(DEV)
        full = len(shape) - 1
        a = M.instance_metrics(pred, target, K, connectivity=full, return_maps=True)
        b = M.instance_metrics(pred, target, K, connectivity=full, return_maps=True)
        for name, s, t in zip(M.InstanceMetrics._fields, a, b):
            assert torch.equal(s.view(torch.uint8), t.view(torch.uint8)), name


def test_a_captured_graph_replays_on_new_contents():
    M = _M()
    shape = (1, 65, 129)
    first, other = _pair("percolation", shape), _pair("lesion", shape)
    K = other[2]
    pred, target = first[0].to(DEV), first[1].to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            M.instance_metrics(pred, target, K, connectivity=2, return_maps=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = M.instance_metrics(pred, target, K, connectivity=2, return_maps=True)
    g.replay()
    torch.cuda.synchronize()
    _check(static, _reference("percolation", shape, 2, K=K), shape, K, "graph, first contents")
    with torch.no_grad():
        pred.copy_(other[0].to(DEV))
        target.copy_(other[1].to(DEV))
    g.replay()
    torch.cuda.synchronize()
    _check(static, _reference("lesion", shape, 2), shape, K, "graph, new contents")
    eager = M.instance_metrics(pred, target, K, connectivity=2, return_maps=True)
    for name, a, b in zip(M.InstanceMetrics._fields, static, eager):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name


def _offset_copy(t):
    """The same values one element (8 bytes) behind a 16-byte boundary of a fresh storage."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    buf[1:] = t.reshape(-1)
    view = buf[1:].view(t.shape)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


@pytest.mark.parametrize("shape", [(3, 36, 57), (2, 6, 10, 70)], ids=["2d", "3d"])
def test_offset_and_non_contiguous_inputs_give_the_same_result(shape):
    M = _M()
    pred, target, K = _pair("lesion", shape)
    pred, target = pred.to(DEV), target.to(DEV)
    full = len(shape) - 1
    want = _reference("lesion", shape, full)
    strided = [t.transpose(-1, -2).contiguous().transpose(-1, -2) for t in (pred, target)]
    assert not strided[0].is_contiguous()
    for p, t in ((_offset_copy(pred), _offset_copy(target)), strided, (pred, strided[1])):
        got = M.instance_metrics(p, t, K, connectivity=full, return_maps=True)
        _check(got, want, shape, K, "layout")
        assert not got.f1.requires_grad


def test_refusals_on_the_device():
    M = _M()
    from advchain_amd._lib import AdvchainHipError
    y = torch.zeros(1, 8, 8, device=DEV, dtype=torch.int64)
    for bad in (y.int(), y.float()):
        with pytest.raises(RuntimeError, match="int64"):
            M.instance_metrics(bad, y, 2)
        with pytest.raises(RuntimeError, match="int64"):
            M.instance_metrics(y, bad, 2)
    with pytest.raises(AdvchainHipError):
        M.instance_metrics(y.cpu(), y, 2)
    with pytest.raises(AdvchainHipError):
        M.instance_metrics(y, y.cpu(), 2)
    with pytest.raises(ValueError, match="iou_threshold"):
        M.instance_metrics(y, y, 2, iou_threshold=0.49)


def test_keep_largest_in_front_leaves_one_predicted_component_per_class():
    import advchain.common.postprocess as P
    M = _M()
    shape = (3, 36, 57)
    pred, target, K = _pair("lesion", shape)
    pd, td = pred.to(DEV), target.to(DEV)
    before = M.instance_metrics(pd, td, K)
    assert int(before.components[..., 0].max()) > 1
    after = M.instance_metrics(P.keep_largest_component(pd, K), td, K)
    assert int(after.components[..., 0].max()) == 1
    assert torch.equal(after.components[..., 1], before.components[..., 1])
    assert torch.equal(after.components[..., 0], (before.components[..., 0] > 0).long())
