"""erosion / dilation / opening / closing on the HIP kernels (csrc/seg_morph.hip) against the brute-force form of
tests/morph_forms.py.  Every output is an integer label map: every comparison is torch.equal.

Shapes: the four of tests/test_morph_cpu.py -- (1, 65, 129) and (1, 9, 17, 129) are two tiles and one voxel along the tiled axis
of ops.MORPH_TILE -- and the 1-wide axes.  The radii bring ties on the sphere (1, 2, 5), balls of 13 and 81 offsets in 2D,
R2 = 5 (2.24), a ball wider than most 3D axes here (7) and one above the image diagonal (on small shapes: the form enumerates
the ball).  With a sampling every squared length is a multiple of 1/16 and 2.3^2 = 5.29 is far from each
(asserted below), so no membership can flip in fp32 and the comparison stays exact."""
import functools

import pytest
import torch

from tests import morph_forms as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
OPS = ("erosion", "dilation", "opening", "closing")
# spelt out so that the ids exist at collection; test_box_shapes_follow_the_kernel holds them to ops.MORPH_TILE
BOX = {2: (1, 65, 129), 3: (1, 9, 17, 129)}
MAIN = [(3, 36, 57), BOX[2], (2, 6, 10, 70), BOX[3]]
THIN = [(2, 1, 70), (2, 70, 1), (1, 5, 1, 9)]
SAMPLING = {2: (1.25, 0.5), 3: (1.5, 1.0, 0.75)}


def shape_id(shape):
    return "x".join(map(str, shape))


def _P():
    import advchain.common.postprocess as P
    return P


def test_box_shapes_follow_the_kernel():
    from advchain_amd import ops
    for nd in (2, 3):
        tile = ops.MORPH_TILE[nd]
        assert len(tile) == nd and all(t is None for t in tile[:-1])           # whole lines along every axis but the last
        assert BOX[nd][-1] == 2 * tile[-1] + 1


@functools.lru_cache(maxsize=None)
def _map(pattern, shape):
    if pattern == "blobs3":
        return M.blobs(3, shape)
    if pattern == "blobs20":
        return M.blobs(20, shape)
    if pattern == "odd3":
        return M.with_odd_labels(M.blobs(3, shape), 3)
    if pattern == "percolation":
        return M.percolation(shape)
    if pattern == "background":
        return torch.zeros(shape, dtype=torch.int64)
    if pattern == "full":
        return torch.ones(shape, dtype=torch.int64)
    raise KeyError(pattern)


@functools.lru_cache(maxsize=None)
def _reference(name, pattern, shape, radius, K, sampling, background):
    return M.BRUTE[name](_map(pattern, shape), radius, K, sampling, background)


def _check(pattern, shape, K, radius, sampling=None, background=0, ops=OPS):
    P = _P()
    x = _map(pattern, shape).to(DEV)
    out = {}
    for name in ops:
        what = "%s %s %s K=%d radius %r sampling %r background %d" % (name, pattern, shape, K, radius, sampling, background)
        got = getattr(P, name)(x, radius, K, sampling=sampling, background=background)
        assert got.dtype == torch.int64 and got.shape == x.shape and got.device == x.device and not got.requires_grad, what
        assert got.data_ptr() != x.data_ptr(), what
        want = _reference(name, pattern, shape, radius, K, sampling, background)
        differ = int((got.cpu() != want).sum())
        assert differ == 0, (what, differ)
        assert torch.equal(got.cpu(), want), what
        out[name] = want
    return out


def _above_the_diagonal(shape):
    return float(sum((s - 1) ** 2 for s in shape[1:])) ** 0.5 + 1.5


@pytest.mark.parametrize("shape", MAIN + THIN, ids=shape_id)
def test_three_class_blobs_at_every_radius(shape):
    for radius in (0, 0.5, 1, 1.5, 2, 2.24, 5, 7):
        got = _check("blobs3", shape, 3, radius)
        if radius < 1:
            assert all(torch.equal(g, _map("blobs3", shape)) for g in got.values())
    if shape in THIN:
        _check("blobs3", shape, 3, _above_the_diagonal(shape))


@pytest.mark.parametrize("shape", [(2, 9, 13), (1, 4, 6, 9)], ids=shape_id)
def test_a_radius_above_the_image_diagonal(shape):
    """(small shapes: the form enumerates every offset that fits in the image)"""
    for pattern, K in (("blobs3", 3), ("odd3", 3), ("percolation", 2)):
        _check(pattern, shape, K, _above_the_diagonal(shape))
        _check(pattern, shape, K, 1e200)


@pytest.mark.parametrize("shape", MAIN + THIN, ids=shape_id)
def test_twenty_classes_and_the_mask(shape):
    for radius in (1.5, 2, 5):
        _check("blobs20", shape, 20, radius)
    for radius in (1, 2):
        _check("percolation", shape, 2, radius)
    if shape == (3, 36, 57):
        x = _map("blobs20", shape)
        assert len(torch.unique(x)) == 20
        for name in OPS:
            assert int((_reference(name, "blobs20", shape, 2, 20, None, 0) != x).sum()) >= 20, name


@pytest.mark.parametrize("shape", MAIN, ids=shape_id)
def test_labels_outside_the_classes_and_other_backgrounds(shape):
    x = _map("odd3", shape)
    assert int((x == -100).sum()) > 0 and int((x == 6).sum()) > 0
    for radius in (1.5, 5):
        got = _check("odd3", shape, 3, radius)
        for name in OPS:                                                         # copied, never changed, never grown
            assert torch.equal(got[name] == -100, x == -100) and torch.equal(got[name] == 6, x == 6), name
    for background in (2, -1):
        _check("odd3", shape, 3, 2, background=background)
    _check("odd3", shape, 2, 2)                                                  # class 2 is outside [0, 2)


@pytest.mark.parametrize("shape", MAIN + THIN, ids=shape_id)
def test_sampling(shape):
    nd = len(shape) - 1
    sampling, radius = SAMPLING[nd], 2.3
    assert M.smallest_relative_gap(radius, shape[1:], sampling) > 1e-3
    _check("blobs3", shape, 3, radius, sampling=sampling)
    _check("odd3", shape, 3, radius, sampling=sampling, background=2)
    _check("blobs20", shape, 20, radius, sampling=sampling)
    _check("blobs3", shape, 3, 0.4, sampling=sampling)                         # below every spacing: a copy


@pytest.mark.parametrize("nd", [2, 3])
def test_all_background_and_all_one_class(nd):
    for shape in (BOX[nd], THIN[nd - 1]):
        for radius in (1, 5, _above_the_diagonal(shape) if shape in THIN else 40):
            if radius == 40:                                  # (the form would enumerate a huge ball: the outcome is known)
                P = _P()
                for pattern in ("background", "full"):
                    x = _map(pattern, shape).to(DEV)
                    for name in OPS:
                        assert torch.equal(getattr(P, name)(x, radius, 2), x), (name, pattern)
                continue
            for pattern in ("background", "full"):
                got = _check(pattern, shape, 2, radius)
                assert all(torch.equal(g, _map(pattern, shape)) for g in got.values())


@pytest.mark.parametrize("nd", [2, 3])
def test_constructed_maps_for_the_rules(nd):
    P = _P()
    shape = (1, 21, 41) if nd == 2 else (1, 9, 21, 41)

    def run(name, x, radius, K):
        got = getattr(P, name)(x.to(DEV), radius, K).cpu()
        assert torch.equal(got, M.BRUTE[name](x, radius, K)), (name, radius)
        return got

    x, gap = M.gap_between_two_classes(shape)
    for radius in (1, 2, 5):
        assert int(run("closing", x, radius, 3)[gap]) == 0 and int(run("dilation", x, radius, 3)[gap]) == 1
    x, at = M.tie_at_25(shape)
    assert int(run("dilation", x, 5, 4)[at]) == 1 and int(run("dilation", x, 4.9, 4)[at]) == 0
    x, bridge = M.two_discs_and_a_bridge((1,) + shape[1:-1] + (61,))
    assert torch.equal(run("opening", x, 1, 2) != x, bridge)
    x = M.class_on_the_border(shape)
    eroded = run("erosion", x, 2, 2)
    assert int(eroded[(0,) + (0,) * nd]) == 1 and int((eroded != x).sum()) > 0
    assert torch.equal(run("closing", x, 3, 2), x)


@pytest.mark.parametrize("nd", [2, 3])
def test_the_nearest_other_label_across_a_seam(nd):
    """At exactly `radius` the voxel goes, one offset beyond it stays: across the seams of the tiled axis (64 and 128) and, for
    the whole-line axes, across the middle."""
    from advchain_amd import ops
    P = _P()
    shape = BOX[nd]
    tile = ops.MORPH_TILE[nd]
    seams = [(nd - 1, tile[-1]), (nd - 1, 2 * tile[-1])] + [(a, shape[1 + a] // 2) for a in range(nd - 1)]
    for axis, seam in seams:
        for radius in (1, 3, 5):
            if seam - 1 + radius + 1 >= shape[1 + axis]:
                continue
            for distance, survives in ((radius, 0), (radius + 1, 1)):
                x, at = M.seam_probe(shape, axis, seam, distance)
                got = P.erosion(x.to(DEV), radius, 3).cpu()
                assert int(got[at]) == survives, (axis, seam, radius, distance)
                assert torch.equal(got, M.erosion_brute(x, radius, 3)), (axis, seam, radius, distance)
                grown = P.dilation((x == 2).long().to(DEV) * 2, radius, 3).cpu()      # the lone voxel of class 2 reaches as far
                assert int(grown[at]) == (0 if survives else 2), (axis, seam, radius, distance)


def test_two_calls_give_the_same_bits():
    P = _P()
    for shape in (BOX[2], (2, 6, 10, 70)):
        x = _map("blobs20", shape).to(DEV)
        for name in OPS:
            for sampling in (None, SAMPLING[len(shape) - 1]):
                a, b = (getattr(P, name)(x, 2.3, 20, sampling=sampling) for _ in range(2))
                assert torch.equal(a, b), (name, sampling)


def test_a_captured_graph_replays_every_function():
    P = _P()
    shape = (3, 36, 57)
    x = _map("blobs3", shape).to(DEV)
    eager = {name: getattr(P, name)(x, 2, 3) for name in OPS}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for name in OPS:
            getattr(P, name)(x, 2, 3)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = {name: getattr(P, name)(x, 2, 3) for name in OPS}
    g.replay()
    torch.cuda.synchronize()
    for name in OPS:
        assert torch.equal(static[name], eager[name]), name
        assert torch.equal(static[name].cpu(), _reference(name, "blobs3", shape, 2, 3, None, 0)), name


def test_layouts_dtypes_and_no_gradient():
    P = _P()
    shape = (2, 6, 10, 70)
    x = _map("blobs3", shape).to(DEV)
    buf = torch.empty(x.numel() + 1, device=DEV, dtype=torch.int64)
    buf[1:] = x.reshape(-1)
    offset = buf[1:].view(shape)
    strided = x.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert offset.data_ptr() % 16 == 8 and not strided.is_contiguous()
    for name in OPS:
        want = getattr(P, name)(x, 2, 3)
        assert torch.equal(getattr(P, name)(offset, 2, 3), want) and torch.equal(getattr(P, name)(strided, 2, 3), want), name
        for bad in (x.int(), x.float()):
            with pytest.raises(RuntimeError, match="int64"):
                getattr(P, name)(bad, 2, 3)
