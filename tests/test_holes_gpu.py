"""fill_holes / find_holes on the HIP kernels (csrc/seg_components.hip) against the brute-force form of tests/holes_forms.py.
Every output is an integer: every comparison is torch.equal, for the filled map, `fill`, `count` and `voxels`, at every
connectivity valid for the rank.

Shapes: components_forms.SHAPES plus (1, 65, 129) and (1, 9, 17, 129), two tiles and one voxel along every tiled axis
(ops.COMPONENTS_TILE).  At connectivity 2 and 3 a random 3D map has next to no holes: in 3D the coverage at full connectivity
rests on the constructed maps, which put the voxels that decide on the seams of the tiles."""
import functools

import pytest
import torch

from tests import components_forms as F
from tests import holes_forms as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
# spelt out so that the ids exist at collection; test_box_shapes_follow_the_kernel holds them to ops.COMPONENTS_TILE
BOX = {2: (1, 65, 129), 3: (1, 9, 17, 129)}
ALL_SHAPES = list(F.SHAPES) + [BOX[2], BOX[3]]
SHAPE_IDS = [F.shape_id(s) for s in ALL_SHAPES]


def _P():
    import advchain.common.postprocess as P
    return P


def _tile(shape):
    from advchain_amd import ops
    return ops.COMPONENTS_TILE[len(shape) - 1]


def test_box_shapes_follow_the_kernel():
    from advchain_amd import ops
    assert BOX == {nd: F.two_tiles_and_one(ops.COMPONENTS_TILE[nd]) for nd in (2, 3)}


@functools.lru_cache(maxsize=None)
def _map(pattern, shape):
    if pattern.startswith("blocks"):
        return F.blocks(int(pattern[6:]), shape)
    if pattern == "percolation":
        return F.percolation(shape)
    if pattern == "three":
        return F.three_classes(shape)
    tile = _tile(shape)
    nd = len(shape) - 1
    return {"box": lambda: H.hollow_box(shape), "island": lambda: H.box_with_island(shape),
            "leak": lambda: H.leaky_box(shape), "leak-far": lambda: H.leaky_box(shape, far=True),
            "contact-x": lambda: H.border_contact(shape, tile, nd - 1, False),
            "contact-z": lambda: H.border_contact(shape, tile, 0, True),
            "snake": lambda: H.serpentine_hole(shape), "snake-odd": lambda: H.serpentine_hole(shape, odd_voxel=True),
            "poison": lambda: H.poisoned_hole(shape, tile, False), "poison-diagonal": lambda: H.poisoned_hole(shape, tile, True),
            "sizes": lambda: H.two_sizes(shape, tile, 5), "mixed": lambda: H.mixed_entries((3,) + shape[1:]),
            "background": lambda: torch.zeros(shape, dtype=torch.int64), "full": lambda: torch.ones(shape, dtype=torch.int64)}[pattern]()


@functools.lru_cache(maxsize=None)
def _reference(pattern, shape, K, connectivity, background=0, max_size=None):
    return H.fill_holes_brute(_map(pattern, shape), K, connectivity, background, max_size)


def _check(pattern, shape, K, connectivity, background=0, max_size=None):
    """Both functions against the form; returns the form's (out, fill, count, voxels)."""
    P = _P()
    x = _map(pattern, shape).to(DEV)
    what = "%s %s K=%d connectivity %d background %d max_size %s" % (pattern, shape, K, connectivity, background, max_size)
    want = _reference(pattern, shape, K, connectivity, background, max_size)
    out = P.fill_holes(x, K, connectivity=connectivity, background=background, max_size=max_size)
    h = P.find_holes(x, K, connectivity=connectivity, background=background, max_size=max_size)
    assert isinstance(h, P.Holes), what
    assert out.dtype == torch.int64 and h.fill.dtype == torch.int64 and h.count.dtype == torch.int64 and h.voxels.dtype == torch.int64
    assert out.device == x.device and all(t.device == x.device for t in h), what
    assert out.shape == x.shape and h.fill.shape == x.shape and tuple(h.count.shape) == tuple(h.voxels.shape) == (x.shape[0], K)
    assert torch.equal(h.count.cpu(), want[2]), (what, h.count.tolist(), want[2].tolist())
    assert torch.equal(h.voxels.cpu(), want[3]), (what, h.voxels.tolist(), want[3].tolist())
    assert torch.equal(h.fill.cpu(), want[1]), what
    assert torch.equal(out.cpu(), want[0]), what
    assert torch.equal(out, torch.where(h.fill >= 0, h.fill, x)), what
    return want


def _connectivities(shape):
    return range(1, len(shape))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_near_percolation_mask(shape):
    for c in _connectivities(shape):
        _check("percolation", shape, 2, c)
        for max_size in (1, 3):
            _check("percolation", shape, 2, c, max_size=max_size)
    if shape in ((1, 65, 129), (3, 36, 57), (1, 9, 17, 129), (2, 6, 10, 70)):                # (not vacuous: asserted on the form)
        assert int(_reference("percolation", shape, 2, 1)[2].sum()) >= 50
        if len(shape) == 4:
            assert H.kinds(_map("percolation", shape), 2, 1, max_size=3)[H.TOO_LARGE] >= 1


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_three_classes_and_another_background(shape):
    for c in _connectivities(shape):
        _check("three", shape, 3, c)
        _check("three", shape, 3, c, background=2)
        _check("three", shape, 2, c)                           # class 2 is outside [0, K): whatever touches it stays
    _check("three", shape, 3, 1, background=7)                 # no voxel is background
    if shape in ((1, 65, 129), (3, 36, 57)):
        kinds = H.kinds(_map("three", shape), 3, 1)
        assert kinds[H.FILLED] >= 1 and kinds[H.BORDER] >= 1 and kinds[H.MIXED] >= 1


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("K", [1, 4, 20])
def test_random_blocks(K, shape):
    for c in _connectivities(shape):
        _check("blocks%d" % K, shape, K, c)
    _check("blocks%d" % K, shape, K, 1, background=-100)       # a background outside [0, K): the -100 specks are the holes
    _check("blocks%d" % K, shape, K, 1, background=K + 3, max_size=1)


@pytest.mark.parametrize("nd", [2, 3])
def test_hollow_box_island_and_leaks(nd):
    shape = BOX[nd]
    cavity = H.cavity_voxels(shape)
    for c in range(1, nd + 1):
        assert _check("box", shape, 2, c)[3].tolist() == [[0, cavity]]
        island = _check("island", shape, 3, c)
        assert island[2].tolist() == [[0, 0, 1]] and int(island[0][(0,) + (2,) * nd]) == 0
        assert _check("island", shape, 2, c)[2].tolist() == [[0, 0]]
        for name in ("leak", "leak-far"):
            assert _check(name, shape, 2, c)[3].tolist() == [[0, cavity if c < nd else 0]], (name, c)
    assert _check("box", shape, 2, 1, max_size=cavity)[3].tolist() == [[0, cavity]]
    assert _check("box", shape, 2, 1, max_size=cavity - 1)[3].tolist() == [[0, 0]]


@pytest.mark.parametrize("nd", [2, 3])
def test_one_voxel_on_the_border_and_the_serpentine(nd):
    shape = BOX[nd]
    for c in range(1, nd + 1):
        for name in ("contact-x", "contact-z"):
            assert _check(name, shape, 2, c)[2].tolist() == [[0, 0]]
        snake = _check("snake", shape, 2, c)
        if c == 1:
            assert snake[2].tolist() == [[0, 1]] and bool((snake[0] == 1).all())
        odd = _check("snake-odd", shape, 3, c)
        if c == 1:
            assert odd[2].tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("nd", [2, 3])
def test_labels_without_a_class_sizes_and_trivial_entries(nd):
    shape = BOX[nd]
    for c in range(1, nd + 1):
        assert _check("poison", shape, 2, c)[2].tolist() == [[0, 0]]
        assert _check("poison-diagonal", shape, 2, c)[2].tolist() == [[0, 1 if c < nd else 0]]
        assert _check("sizes", shape, 2, c)[3].tolist() == [[0, 11]]
        assert _check("sizes", shape, 2, c, max_size=5)[3].tolist() == [[0, 5]]
        assert _check("sizes", shape, 2, c, max_size=6)[3].tolist() == [[0, 11]]
        assert _check("sizes", shape, 2, c, max_size=4)[3].tolist() == [[0, 0]]
        assert _check("sizes", shape, 2, c, max_size=2 ** 62)[3].tolist() == [[0, 11]]
        assert _check("background", shape, 2, c)[2].tolist() == [[0, 0]]
        assert _check("full", shape, 2, c)[2].tolist() == [[0, 0]]
        mixed = _check("mixed", shape, 2, c)
        assert mixed[2].tolist() == [[0, 1], [0, 0], [0, 0]] and mixed[3].tolist() == [[0, H.cavity_voxels(shape)], [0, 0], [0, 0]]
    # max_size beyond 2^62 is clamped
    x = _map("sizes", shape).to(DEV)
    assert torch.equal(_P().fill_holes(x, 2, max_size=2 ** 80), _P().fill_holes(x, 2))


def test_two_calls_give_the_same_bits():
    P = _P()
    for pattern, shape in (("percolation", (1, 70, 130)), ("percolation", (1, 20, 20, 40)), ("box", BOX[2]), ("box", BOX[3])):
        x = _map(pattern, shape).to(DEV)
        for c in _connectivities(shape):
            a, b = P.find_holes(x, 2, connectivity=c), P.find_holes(x, 2, connectivity=c)
            assert all(torch.equal(s, t) for s, t in zip(a, b))
            assert torch.equal(P.fill_holes(x, 2, connectivity=c), P.fill_holes(x, 2, connectivity=c))


def test_a_captured_graph_replays_on_new_contents():
    P = _P()
    shape = (1, 70, 130)
    x = _map("percolation", shape).to(DEV)
    other = _map("three", shape)
    eager = P.fill_holes(x, 3, connectivity=2)
    eager_h = P.find_holes(x, 3, connectivity=2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            P.fill_holes(x, 3, connectivity=2)
            P.find_holes(x, 3, connectivity=2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = P.fill_holes(x, 3, connectivity=2)
        static_h = P.find_holes(x, 3, connectivity=2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager) and all(torch.equal(a, b) for a, b in zip(static_h, eager_h))
    with torch.no_grad():
        x.copy_(other.to(DEV))
    g.replay()
    torch.cuda.synchronize()
    want = H.fill_holes_brute(other, 3, 2)
    assert torch.equal(static.cpu(), want[0])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(static_h, want[1:]))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.cpu(), want[0]) and all(torch.equal(a.cpu(), b) for a, b in zip(static_h, want[1:]))


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
    x = _map("three", shape).to(DEV)
    layouts = [_offset_copy(x), x.transpose(-1, -2).contiguous().transpose(-1, -2)]
    assert not layouts[1].is_contiguous()
    want = P.fill_holes(x, 3)
    want_h = P.find_holes(x, 3)
    assert torch.equal(want.cpu(), _reference("three", shape, 3, 1)[0])
    for v in layouts:
        assert torch.equal(v, x)
        assert torch.equal(P.fill_holes(v, 3), want)
        assert all(torch.equal(s, t) for s, t in zip(P.find_holes(v, 3), want_h))


@pytest.mark.parametrize("shape", [(3, 36, 57), (1, 65, 129), (2, 6, 10, 70)], ids=F.shape_id)
def test_filling_is_idempotent_on_the_device(shape):
    P = _P()
    for pattern, K in (("percolation", 2), ("three", 3), ("blocks4", 4)):
        for c in _connectivities(shape):
            x = _map(pattern, shape).to(DEV)
            once = P.fill_holes(x, K, connectivity=c)
            again = P.find_holes(once, K, connectivity=c)
            assert torch.equal(P.fill_holes(once, K, connectivity=c), once)
            assert int(again.count.sum()) == 0 and int(again.voxels.sum()) == 0 and bool((again.fill == -1).all())


@pytest.mark.parametrize("shape", [(1, 65, 129), (1, 9, 17, 129)], ids=["2d", "3d"])
def test_the_component_functions_still_equal_their_forms(shape):
    """The tile and seam kernels are shared with fill_holes; this guards their other instantiation from within this file."""
    P = _P()
    x = _map("blocks4", shape)
    xd = x.to(DEV)
    for c in _connectivities(shape):
        for K in (4, None):
            want = F.components_brute(x, c, 0, K)
            got = P.connected_components(xd, connectivity=c, num_classes=K, return_sizes=True)
            assert all(torch.equal(g.cpu(), w) for g, w in zip((got.labels, got.count, got.sizes), want)), (c, K)
            assert torch.equal(P.remove_small_components(xd, 5, connectivity=c, num_classes=K).cpu(),
                               F.remove_small_brute(x, 5, c, num_classes=K, components=want)), (c, K)
        assert torch.equal(P.keep_largest_component(xd, 4, connectivity=c).cpu(), F.keep_largest_brute(x, 4, c)), c


def test_refusals_on_the_device():
    P = _P()
    y = torch.zeros(1, 8, 8, device=DEV, dtype=torch.int64)
    for bad in (y.int(), y.float()):
        with pytest.raises(RuntimeError, match="int64"):
            P.fill_holes(bad, 2)
        with pytest.raises(RuntimeError, match="int64"):
            P.find_holes(bad, 2)
    assert not P.fill_holes(y.requires_grad_(False), 2).requires_grad


def test_filling_the_cavity_takes_the_inner_surface_out_of_the_hausdorff_distance():
    P = _P()
    import advchain.common.metrics as M
    shape = (1, 24, 28, 30)
    grids = torch.meshgrid(*[torch.arange(s, dtype=torch.float32) for s in shape[1:]], indexing="ij")
    r2 = sum((g - (s - 1) / 2.0) ** 2 for g, s in zip(grids, shape[1:]))
    target = (r2 <= 9.0 ** 2).long().unsqueeze(0)
    pred = target.clone()
    pred[r2.unsqueeze(0) <= 3.0 ** 2] = 0                                         # a cavity in the middle of the ball
    assert int(target.sum()) > int(pred.sum()) > 0
    pd, yd = pred.to(DEV), target.to(DEV)
    before = M.surface_distance_metrics(pd, yd, 2)
    assert float(before.hausdorff[0, 1]) > 0.0 and float(before.dice[0, 1]) < 1.0
    filled = P.fill_holes(pd, 2)
    assert torch.equal(filled, yd)
    h = P.find_holes(pd, 2)
    assert h.count.tolist() == [[0, 1]] and h.voxels.tolist() == [[0, int(target.sum()) - int(pred.sum())]]
    after = M.surface_distance_metrics(filled, yd, 2)
    assert float(after.hausdorff[0, 1]) == 0.0 and float(after.dice[0, 1]) == 1.0
