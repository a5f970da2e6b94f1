"""connected_components / keep_largest_component / remove_small_components on the HIP kernels (csrc/seg_components.hip) against
the brute-force forms of tests/components_forms.py.  Every output is an integer: every comparison is torch.equal.

Shapes: components_forms.SHAPES, plus per dimensionality one with exactly two tiles along every tiled axis and a tail of one
voxel, derived from ops.COMPONENTS_TILE -- (32, 64) in 2D, (4, 8, 64) in 3D: (1, 65, 129) and (1, 9, 17, 129).  Every map runs at
every connectivity valid for its rank."""
import functools

import pytest
import torch

from tests import components_forms as F
from tests.surface_forms import speck_pair

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _P():
    import advchain.common.postprocess as P
    return P


def _tile(shape):
    from advchain_amd import ops
    return ops.COMPONENTS_TILE[len(shape) - 1]


@functools.lru_cache(maxsize=None)
def _shapes():
    from advchain_amd import ops
    return tuple(F.SHAPES) + tuple(F.two_tiles_and_one(ops.COMPONENTS_TILE[nd]) for nd in (2, 3))


# the two-tile shapes are spelt out so that the ids exist at collection; test_tile_shapes_follow_the_kernel holds them to ops
ALL_SHAPES = list(F.SHAPES) + [(1, 65, 129), (1, 9, 17, 129)]
SHAPE_IDS = [F.shape_id(s) for s in ALL_SHAPES]


def test_tile_shapes_follow_the_kernel():
    assert list(_shapes()) == ALL_SHAPES


@functools.lru_cache(maxsize=None)
def _map(pattern, shape):
    tile = _tile(shape)
    if pattern.startswith("blocks"):
        return F.blocks(int(pattern[6:]), shape)
    if pattern == "percolation":
        return F.percolation(shape)
    if pattern == "sparse":
        return F.percolation(shape, p=0.32)
    if pattern == "three":
        return F.three_classes(shape)
    if pattern == "serpentine":
        return F.serpentine(shape)
    if pattern == "double":
        return F.double_serpentine(shape)
    if pattern == "u":
        return F.u_shape(shape)
    if pattern == "checkerboard":
        return F.checkerboard(shape)
    if pattern == "lines":
        return F.crossing_lines(shape, tile)
    if pattern.startswith("pair-"):
        return F.corner_pairs(shape, tile)[pattern[5:]][0]
    return F.trivial_maps(shape)[pattern]


@functools.lru_cache(maxsize=None)
def _reference(pattern, shape, connectivity, background=0, num_classes=None):
    return F.components_brute(_map(pattern, shape), connectivity, background, num_classes)


def _connectivities(shape):
    return range(1, len(shape))


def _check_components(got, want, x, what):
    P = _P()
    labels, count, sizes = want
    assert isinstance(got, P.Components), what
    assert got.labels.dtype == torch.int32 and got.count.dtype == torch.int64 and got.sizes.dtype == torch.int32, what
    assert got.labels.device == x.device and got.count.device == x.device and got.sizes.device == x.device, what
    assert got.labels.shape == x.shape and got.sizes.shape == x.shape and tuple(got.count.shape) == (x.shape[0],), what
    assert torch.equal(got.count.cpu(), count), (what, got.count.tolist(), count.tolist())
    assert torch.equal(got.labels.cpu(), labels), what
    assert torch.equal(got.sizes.cpu(), sizes), what


def _run(pattern, shape, num_classes=None, background=0):
    P = _P()
    x = _map(pattern, shape).to(DEV)
    counts = {}
    for c in _connectivities(shape):
        what = "%s %s connectivity %d" % (pattern, shape, c)
        got = P.connected_components(x, connectivity=c, background=background, num_classes=num_classes, return_sizes=True)
        want = _reference(pattern, shape, c, background, num_classes)
        _check_components(got, want, x, what)
        counts[c] = want[1]
    return counts


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("K", [1, 4, 20])
def test_random_blocks(K, shape):
    _run("blocks%d" % K, shape, num_classes=K)
    _run("blocks%d" % K, shape, num_classes=None)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_near_percolation_mask_and_three_classes(shape):
    _run("percolation", shape)
    if len(shape) == 4:
        _run("sparse", shape)                 # (0.59 is far above the threshold of the cubic lattice, 0.31: one cluster)
    _run("three", shape)
    _run("three", shape, num_classes=2, background=1)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_serpentines_and_u_shape(shape):
    full = len(shape) - 1
    assert _run("serpentine", shape)[1].tolist() == [1] * shape[0]
    double = _run("double", shape)
    if shape[-1] >= 3:
        assert double[1].tolist() == [2] * shape[0] and double[full].tolist() == [2] * shape[0]
    assert _run("u", shape)[1].tolist() == [1] * shape[0]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_checkerboard_and_crossing_lines(shape):
    full = len(shape) - 1
    board = _run("checkerboard", shape)
    per_entry = int(_map("checkerboard", shape)[0].sum())
    assert board[1].tolist() == [per_entry] * shape[0] and board[full].tolist() == [1] * shape[0]
    lines = _run("lines", shape)
    voxels = int((_map("lines", shape)[0] > 0).sum())
    assert lines[1].tolist() == [voxels] * shape[0] and lines[full].tolist() == [2] * shape[0]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_pairs_across_tile_corners_and_edges(shape):
    names = ["corner", "anti-corner"] if len(shape) == 3 else ["edge-zy", "edge-zx", "edge-yx", "corner"]
    for name in names:
        joined_from = F.corner_pairs(shape, _tile(shape))[name][1]
        counts = _run("pair-" + name, shape)
        for c in _connectivities(shape):
            assert counts[c].tolist() == [1 if c >= joined_from else 2] * shape[0], (name, c)      # 18 neighbours: no corner


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_trivial_maps(shape):
    V = 1
    for s in shape[1:]:
        V *= s
    assert _run("background", shape)[1].tolist() == [0] * shape[0]
    assert _run("full", shape)[1].tolist() == [1] * shape[0]
    assert _run("single", shape)[1].tolist() == [1] * shape[0]
    got = _P().connected_components(_map("full", shape).to(DEV), return_sizes=True)
    assert bool((got.sizes == V).all()) and bool((got.labels == 1).all())


def test_sizes_are_optional():
    got = _P().connected_components(_map("percolation", (3, 36, 57)).to(DEV))
    assert got.sizes is None and torch.equal(got.labels.cpu(), _reference("percolation", (3, 36, 57), 1)[0])


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_keep_largest_component(shape):
    P = _P()
    for pattern, K in (("blocks4", 4), ("blocks20", 20), ("percolation", 2), ("three", 3)):
        x = _map(pattern, shape)
        for c in _connectivities(shape):
            got = P.keep_largest_component(x.to(DEV), K, connectivity=c)
            assert got.dtype == torch.int64 and got.is_cuda and got.shape == x.shape
            assert torch.equal(got.cpu(), F.keep_largest_brute(x, K, c, components=_reference(pattern, shape, c, 0, K))), (pattern, c)
    x = _map("three", shape)
    got = P.keep_largest_component(x.to(DEV), 3, connectivity=1, background=2)
    assert torch.equal(got.cpu(), F.keep_largest_brute(x, 3, 1, background=2, components=_reference("three", shape, 1, 2, 3)))


def test_keep_largest_ties_absent_classes_and_labels_without_a_class():
    P = _P()
    x = torch.zeros(2, 40, 70, dtype=torch.int64)
    x[0, 3, 2:7] = 1                       # five voxels: the earlier of two equals wins
    x[0, 35, 60:65] = 1                    # five voxels in another tile
    x[0, 20, 10:14] = 1
    x[0, 10:13, 66] = 3
    x[0, 30, 30] = 3
    x[0, 0, 0] = -100
    x[0, 39, 69] = 9                       # outside [0, 5): copied
    x[1, 5:9, 5:9] = 2                     # classes 1, 3 and 4 are absent from entry 1
    got = P.keep_largest_component(x.to(DEV), 5).cpu()
    want = x.clone()
    want[0, 35, 60:65] = 0
    want[0, 20, 10:14] = 0
    want[0, 30, 30] = 0
    assert torch.equal(got, want) and torch.equal(got, F.keep_largest_brute(x, 5))
    got = P.keep_largest_component(x.to(DEV), 5, background=2).cpu()          # class 0 is now a class; class 2 is left alone
    assert torch.equal(got, F.keep_largest_brute(x, 5, background=2))
    assert torch.equal(got[1], x[1]) and int((got[0] == 2).sum()) == 5 + 4 + 1


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_remove_small_components(shape):
    P = _P()
    for pattern, K in (("blocks4", 4), ("percolation", None), ("three", None)):
        x = _map(pattern, shape)
        for c in _connectivities(shape):
            for min_size in (1, 2, 50):
                for num_classes in ((None, K) if K else (None,)):
                    got = P.remove_small_components(x.to(DEV), min_size, connectivity=c, num_classes=num_classes)
                    assert got.dtype == torch.int64 and got.is_cuda and got.shape == x.shape
                    want = F.remove_small_brute(x, min_size, c, num_classes=num_classes,
                                                components=_reference(pattern, shape, c, 0, num_classes))
                    assert torch.equal(got.cpu(), want), (pattern, c, min_size)
                    if min_size == 1:
                        # a label that num_classes makes background is in no component: it is copied, like everything else
                        assert torch.equal(got.cpu(), x)
    x = _map("three", shape)
    got = P.remove_small_components(x.to(DEV), 3, background=1, num_classes=3)
    assert torch.equal(got.cpu(), F.remove_small_brute(x, 3, 1, background=1, num_classes=3))


def test_two_calls_give_the_same_bits():
    P = _P()
    for shape in ((1, 70, 130), (1, 20, 20, 40)):
        x = _map("percolation", shape).to(DEV)
        full = len(shape) - 1
        a = P.connected_components(x, connectivity=full, return_sizes=True)
        b = P.connected_components(x, connectivity=full, return_sizes=True)
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        assert torch.equal(P.keep_largest_component(x, 2, connectivity=full), P.keep_largest_component(x, 2, connectivity=full))
        assert torch.equal(P.remove_small_components(x, 9), P.remove_small_components(x, 9))


def test_a_captured_graph_replays_keep_largest_on_new_contents():
    P = _P()
    shape = (1, 70, 130)
    x = _map("percolation", shape).to(DEV)
    other = _map("three", shape)
    eager = P.keep_largest_component(x, 3, connectivity=2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            P.keep_largest_component(x, 3, connectivity=2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = P.keep_largest_component(x, 3, connectivity=2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    with torch.no_grad():
        x.copy_(other.to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, P.keep_largest_component(x, 3, connectivity=2))
    assert torch.equal(static.cpu(), F.keep_largest_brute(other, 3, 2))


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
    P = _P()
    x = _map("blocks4", shape).to(DEV)
    full = len(shape) - 1
    layouts = [_offset_copy(x), x.transpose(-1, -2).contiguous().transpose(-1, -2)]
    assert not layouts[1].is_contiguous()
    want = P.connected_components(x, connectivity=full, num_classes=4, return_sizes=True)
    kept = P.keep_largest_component(x, 4, connectivity=full)
    small = P.remove_small_components(x, 5, connectivity=full)
    for v in layouts:
        assert torch.equal(v, x)
        got = P.connected_components(v, connectivity=full, num_classes=4, return_sizes=True)
        assert all(torch.equal(s, t) for s, t in zip(got, want))
        assert torch.equal(P.keep_largest_component(v, 4, connectivity=full), kept)
        assert torch.equal(P.remove_small_components(v, 5, connectivity=full), small)


def test_refusals_on_the_device():
    P = _P()
    from advchain_amd._lib import AdvchainHipError
    y = torch.zeros(1, 8, 8, device=DEV, dtype=torch.int64)
    for bad in (y.int(), y.float()):
        with pytest.raises(RuntimeError, match="int64"):
            P.connected_components(bad)
        with pytest.raises(RuntimeError, match="int64"):
            P.keep_largest_component(bad, 2)
        with pytest.raises(RuntimeError, match="int64"):
            P.remove_small_components(bad, 2)
    with pytest.raises(AdvchainHipError):
        P.keep_largest_component(y.cpu(), 2)
    assert not P.keep_largest_component(y, 2).requires_grad


def test_the_filter_takes_the_speck_out_of_the_hausdorff_distance():
    P = _P()
    import advchain.common.metrics as M
    pred, target = speck_pair((1, 40, 12))
    pd, yd = pred.to(DEV), target.to(DEV)
    before = M.surface_distance_metrics(pd, yd, 2)
    assert float(before.hausdorff[0, 1]) > 30.0
    filtered = P.keep_largest_component(pd, 2)
    changed = filtered != pd
    assert int(changed.sum()) == 1 and filtered[changed].tolist() == [0]       # the speck is background now, -100 is copied
    after = M.surface_distance_metrics(filtered, yd, 2)
    assert float(after.hausdorff[0, 1]) == 0.0 and float(after.dice[0, 1]) == 1.0
