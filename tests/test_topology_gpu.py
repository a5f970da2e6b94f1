"""common.metrics.betti_numbers / betti_error on the HIP kernels (csrc/seg_components.hip: k_betti_euler, the labelling passes with
k_betti_roots, in 3D the kComplement labelling per class with k_betti_border, k_betti_finish) against the reference form of
tests/topology_forms.py (numpy and scipy.ndimage.label).  Everything is an integer and is compared with torch.equal.

Shapes: those of tests/test_instances_gpu.py -- smaller than a wave, tails in both axes, one axis far longer than any tile, several
slabs, and per dimensionality the one with exactly two tiles along every tiled axis plus one voxel, from ops.COMPONENTS_TILE (the
window pass uses the same tiles): (1, 65, 129) and (1, 9, 17, 129) -- and axes of one voxel.  Every case runs at every valid
connectivity: 1 and 2 in 2D, 1 and 3 in 3D."""
import functools

import pytest
import torch

from tests import components_forms as C
from tests import topology_forms as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")

SHAPES = [(2, 5, 7), (3, 36, 57), (1, 65, 129), (1, 600, 9), (2, 6, 10, 70), (1, 9, 17, 129), (1, 1, 9), (1, 1, 1, 9), (1, 5, 1, 3)]
SHAPE_IDS = [C.shape_id(s) for s in SHAPES]
TWO_TILES = [(1, 65, 129), (1, 9, 17, 129)]
PATTERNS = ["percolation", "sparse", "three", "checkerboard", "ones", "zeros", "ignored", "blocks"]
# the hand shapes of tests/test_topology_cpu.py across the first tile seam of every axis that has one: name -> (shape, mask)
HANDS = {"ring 3x3": ((1, 65, 129), T.RING_3X3), "diamond ring": ((1, 65, 129), T.DIAMOND_RING),
         "checker 2x2": ((2, 36, 70), T.CHECKER_2X2), "solid torus": ((1, 9, 21, 80), T.solid_torus()),
         "spherical shell": ((1, 15, 15, 75), T.spherical_shell()), "hollow torus": ((1, 13, 31, 90), T.hollow_torus()),
         "cube hollow torus": ((2, 6, 10, 70), T.cube_hollow_torus())}
EXPECTED = {h[0]: h[2:] for h in T.HAND_2D + T.HAND_3D}


def _M():
    import advchain.common.metrics as M
    return M


def test_tile_shapes_follow_the_kernel():
    from advchain_amd import ops
    assert [C.two_tiles_and_one(ops.COMPONENTS_TILE[nd]) for nd in (2, 3)] == TWO_TILES
    assert all(s in SHAPES for s in TWO_TILES)


@functools.lru_cache(maxsize=None)
def _map(pattern, shape):
    """(labels, K) on the CPU; never modified."""
    if pattern == "percolation":                                                # many loops in 2D, one tortuous cluster in 3D
        return C.percolation(shape), 2
    if pattern == "sparse":                                                     # many components; in 3D the complement has loops
        return C.percolation(shape, p=0.32), 2
    if pattern == "three":
        return C.three_classes(shape), 3
    if pattern == "checkerboard":
        return C.checkerboard(shape), 2
    if pattern == "ones":                                                       # a class that fills the image: the closed cells on
        return torch.ones(shape, dtype=torch.int64), 3                          # its high faces are counted; classes 0, 2 are empty
    if pattern == "zeros":
        return torch.zeros(shape, dtype=torch.int64), 2
    if pattern == "ignored":                                                    # every voxel outside [0, K): in no class
        x = torch.full(shape, -100, dtype=torch.int64)
        x.reshape(-1)[::3] = 5
        return x, 2
    if pattern == "blocks":                                                     # 5 % of the voxels at -100 and one at K + 3
        return C.blocks(4, shape), 4
    if pattern in HANDS:
        shape, mask = HANDS[pattern]
        tile = (32, 64) if mask.ndim == 2 else (4, 8, 64)
        at = tuple(T.across_seam(e, t, s) for e, t, s in zip(mask.shape, tile, shape[1:]))
        return T.embedded(shape, mask, at), 2
    raise KeyError(pattern)


@functools.lru_cache(maxsize=None)
def _reference(pattern, shape, connectivity):
    x, K = _map(pattern, shape)
    return T.betti_form(x, K, connectivity)


def _connectivities(shape):
    return T.valid_connectivities(len(shape) - 1)


def _check(got, want, what):
    M = _M()
    assert isinstance(got, M.Betti), what
    for name, g, w in zip(M.Betti._fields, got, want):
        assert g.dtype == torch.int64 and g.is_cuda and g.shape == w.shape, (what, name, g.shape)
        assert torch.equal(g.cpu(), w), (what, name, g.cpu().tolist(), w.tolist())


def _run(pattern, shape):
    x, K = _map(pattern, shape)
    xd = x.to(DEV)
    for c in _connectivities(x.shape):
        what = "%s %s connectivity %d" % (pattern, shape, c)
        _check(_M().betti_numbers(xd, K, connectivity=c), _reference(pattern, shape, c), what)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_against_the_reference_form(pattern, shape):
    _run(pattern, shape)


@pytest.mark.parametrize("pattern", sorted(HANDS))
def test_hand_shapes_across_the_tile_seams(pattern):
    _run(pattern, None)
    x, K = _map(pattern, None)
    for c, want in zip(_connectivities(x.shape), EXPECTED[pattern]):            # the reference itself gives the known numbers
        betti, euler = _reference(pattern, None, c)
        assert all(betti[n, 1].tolist() == list(want) for n in range(x.shape[0])), (pattern, c, betti.tolist())


def test_the_cases_are_not_vacuous():
    """Over the suite every Betti number that can be non-zero reaches 2 in both dimensionalities (the reference's own values), and
    the filled and the empty classes give the values their definitions state."""
    most = {2: [0, 0, 0], 3: [0, 0, 0]}
    for pattern in PATTERNS:
        for shape in SHAPES:
            for c in _connectivities(shape):
                top = _reference(pattern, shape, c)[0].amax(dim=(0, 1)).tolist()
                most[len(shape) - 1] = [max(a, b) for a, b in zip(most[len(shape) - 1], top)]
    assert min(most[2][:2]) >= 2 and most[2][2] == 0 and min(most[3]) >= 2, most
    for shape in SHAPES:
        for c in _connectivities(shape):
            betti, euler = _reference("ones", shape, c)
            assert betti[:, 1].tolist() == [[1, 0, 0]] * shape[0] and euler[:, 1].tolist() == [1] * shape[0]
            assert int(betti[:, [0, 2]].abs().sum()) == 0 and int(euler[:, [0, 2]].abs().sum()) == 0
            betti, euler = _reference("ignored", shape, c)
            assert int(betti.abs().sum()) == 0 and int(euler.abs().sum()) == 0


@pytest.mark.parametrize("shape", [(3, 36, 57), (2, 6, 10, 70)], ids=["2d", "3d"])
def test_the_error_is_that_of_two_calls_and_zero_for_a_map_with_itself(shape):
    M = _M()
    pred, K = _map("three", shape)
    target = C.three_classes(shape, seed=5)
    pd, td = pred.to(DEV), target.to(DEV)
    for c in _connectivities(shape):
        got = M.betti_error(pd, td, K, connectivity=c)
        assert isinstance(got, M.BettiError)
        want = T.error_form(pred, target, K, c)
        for name, g, w in zip(M.BettiError._fields, got, want):
            assert g.dtype == torch.int64 and g.is_cuda and g.shape == w.shape, (name, c)
            assert torch.equal(g.cpu(), w), (name, c, g.cpu().tolist(), w.tolist())
        assert int(got.total.sum()) > 0                                         # (the two maps differ in topology)
        a, b = M.betti_numbers(pd, K, connectivity=c), M.betti_numbers(td, K, connectivity=c)
        assert torch.equal(got.betti, torch.stack([a.betti, b.betti], dim=2))
        assert torch.equal(got.euler, torch.stack([a.euler, b.euler], dim=2))
        assert torch.equal(got.error, (a.betti - b.betti).abs())
        same = M.betti_error(pd, pd.clone(), K, connectivity=c)
        assert int(same.error.abs().sum()) == 0 and int(same.total.abs().sum()) == 0
        assert torch.equal(same.betti[:, :, 0], a.betti) and torch.equal(same.betti[:, :, 1], a.betti)


def test_two_calls_give_the_same_bits():
    M = _M()
    for shape in ((1, 65, 129), (1, 9, 17, 129)):
        x, K = _map("percolation", shape)
        xd = x.to(DEV)
        for c in _connectivities(shape):
            a, b = M.betti_numbers(xd, K, connectivity=c), M.betti_numbers(xd, K, connectivity=c)
            assert torch.equal(a.betti, b.betti) and torch.equal(a.euler, b.euler), (shape, c)


@pytest.mark.parametrize("shape", [(3, 36, 57), (2, 6, 10, 70)], ids=["2d", "3d"])
def test_class_counts_above_the_lds_table_take_the_global_route_to_the_same_numbers(shape):
    """Up to 2048 classes a workgroup sums in LDS, above every window and wave adds to global memory: the same labels give the same
    numbers on both routes, in the rows of the classes that are there; every other row is zero."""
    M = _M()
    x, _ = _map("three", shape)
    moved = x.clone()
    moved[x == 1] = 2047
    moved[x == 2] = 2999
    xd, md = x.to(DEV), moved.to(DEV)
    rows = torch.tensor([0, 2047, 2999], device=DEV)
    for c in _connectivities(shape):
        small = M.betti_numbers(xd, 3, connectivity=c)
        _check(small, _reference("three", shape, c), "small")
        for K in ((2048, 2049, 3000) if len(shape) == 3 else (2049,)):            # (a 3D map costs a labelling per class)
            got = M.betti_numbers(md, K, connectivity=c)
            there = rows[rows < K]
            assert torch.equal(got.betti[:, there], small.betti[:, :len(there)]), (K, c)
            assert torch.equal(got.euler[:, there], small.euler[:, :len(there)]), (K, c)
            rest = torch.ones(K, dtype=torch.bool, device=DEV)
            rest[there] = False
            assert int(got.betti[:, rest].abs().sum()) == 0 and int(got.euler[:, rest].abs().sum()) == 0, (K, c)


@pytest.mark.parametrize("shape", [(1, 65, 129), (2, 6, 10, 70)], ids=["2d", "3d"])
def test_a_captured_graph_replays_on_new_contents(shape):
    M = _M()
    full = len(shape) - 1
    first, other = _map("percolation", shape)[0], _map("three", shape)[0]
    K = 3
    pred, target = first.to(DEV), other.to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            M.betti_error(pred, target, K, connectivity=full)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = M.betti_error(pred, target, K, connectivity=full)
    g.replay()
    torch.cuda.synchronize()
    for name, a, w in zip(M.BettiError._fields, static, T.error_form(first, other, K, full)):
        assert torch.equal(a.cpu(), w), ("graph, first contents", name)
    with torch.no_grad():
        pred.copy_(other.to(DEV))
        target.copy_(C.three_classes(shape, seed=7).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    for name, a, w in zip(M.BettiError._fields, static, T.error_form(other, C.three_classes(shape, seed=7), K, full)):
        assert torch.equal(a.cpu(), w), ("graph, new contents", name)
    eager = M.betti_error(pred, target, K, connectivity=full)
    for name, a, b in zip(M.BettiError._fields, static, eager):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("shape", [(3, 36, 57), (2, 6, 10, 70)], ids=["2d", "3d"])
def test_non_contiguous_inputs_give_the_same_result(shape):
    M = _M()
    x, K = _map("blocks", shape)
    xd = x.to(DEV)
    strided = xd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not strided.is_contiguous()
    wide = torch.zeros(shape[:-1] + (shape[-1] + 3,), dtype=torch.int64, device=DEV)
    wide[..., 1:-2] = xd
    view = wide[..., 1:-2]
    assert not view.is_contiguous()
    for c in _connectivities(shape):
        want = _reference("blocks", shape, c)
        for v in (strided, view):
            got = M.betti_numbers(v, K, connectivity=c)
            _check(got, want, "layout")
            assert not got.betti.requires_grad
        both = M.betti_error(strided, view, K, connectivity=c)
        assert int(both.error.abs().sum()) == 0 and torch.equal(both.betti[:, :, 0].cpu(), want[0])


def test_entries_do_not_mix():
    M = _M()
    for shape in ((1, 36, 57), (1, 6, 10, 70)):
        singles = [_map(p, shape)[0] for p in ("percolation", "three", "checkerboard")]
        xd = torch.cat(singles).to(DEV)
        for c in _connectivities(shape):
            whole = M.betti_numbers(xd, 3, connectivity=c)
            parts = [M.betti_numbers(xd[n:n + 1], 3, connectivity=c) for n in range(3)]
            assert torch.equal(whole.betti, torch.cat([p.betti for p in parts])), (shape, c)
            assert torch.equal(whole.euler, torch.cat([p.euler for p in parts])), (shape, c)


def test_refusals_on_the_device():
    M = _M()
    from advchain_amd._lib import AdvchainHipError
    y = torch.zeros(1, 8, 8, device=DEV, dtype=torch.int64)
    for bad in (y.int(), y.float()):
        with pytest.raises(RuntimeError, match="int64"):
            M.betti_numbers(bad, 2)
        with pytest.raises(RuntimeError, match="int64"):
            M.betti_error(y, bad, 2)
    with pytest.raises(AdvchainHipError):
        M.betti_error(y.cpu(), y, 2)
    with pytest.raises(AdvchainHipError):
        M.betti_error(y, y.cpu(), 2)
    with pytest.raises(ValueError, match="18-adjacency"):
        M.betti_numbers(y.unsqueeze(0), 2, connectivity=2)


def test_a_tensor_on_a_device_that_is_not_current():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second device")
    M = _M()
    shape = (2, 6, 10, 70)
    x, K = _map("three", shape)
    xd = x.to(torch.device("cuda", 1))
    assert torch.cuda.current_device() == 0
    got = M.betti_numbers(xd, K, connectivity=3)
    assert got.betti.device == xd.device
    _check(got, _reference("three", shape, 3), "second device")
