"""surface_distance_metrics / hausdorff_distance / average_surface_distance on the HIP kernels (csrc/seg_surface.hip on the fields
of csrc/edt.hip) against the brute-force float64 forms of tests/surface_forms.py: every tile shape of the edge pass and of the
transform, 1 to 300 classes (more than one group of histograms, counters and accumulators), absent classes, -100 and
out-of-range labels, squared distances in every radix digit, the percentile rule at its ends and across digits, the empty-border
conventions, bitwise reproducibility, a captured graph, misaligned and non-contiguous inputs and the device guard.

Bounds.  Counts, overlaps and (unit spacing) the largest squared distances are integers: torch.equal.  Unit spacing: every square
is exact, root, interpolation and mean are taken in fp64 and rounded to fp32 once (half an ulp), so a value is within 1.2e-7
relative of the float64 reference (the one-ulp bound of tests/test_boundary_gpu.py).  With a sampling: SAMPLING_TOL relative
(2e-6) -- order statistics, maxima and means of values that are each within a relative bound stay within it -- and twice that
for the squares.  Zeros, infinities and NaN are compared exactly."""
import functools

import pytest
import torch

from tests.edt_forms import SAMPLING, SAMPLING_TOL
from tests.surface_forms import (CASES, FAR_SHAPE, FIELDS, PERCENTILES, case_id, directed_squares, metrics_of, pair_of, speck_pair)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ULP = 1.2e-7
FLOATS = ["hausdorff", "hausdorff_percentile", "assd", "directed", "dice"]


def _M():
    import advchain.common.metrics as M
    return M


def _relative_close(got, want, tol, what):
    """Zeros, infinities and NaN exactly, everything else within tol relative."""
    got = got.detach().cpu().double()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    special = ((want == 0) | torch.isinf(want)) & ~nan
    assert torch.equal(got[special], want[special]), what
    rest = ~special & ~nan
    rel = (got - want).abs()[rest] / want[rest].abs()
    worst = float(rel.max()) if rel.numel() else 0.0
    print("%s: relative error %.3g (bound %.3g)" % (what, worst, tol))
    assert worst <= tol, (what, worst)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x).cpu(), _bits(y).cpu()) for x, y in zip(a, b))


def _against(got, want, sampled, what):
    N, K = want.dice.shape
    shapes = dict(hausdorff=(N, K), hausdorff_percentile=(N, K), assd=(N, K), directed=(N, K, 2, 3), surface_voxels=(N, K, 2),
                  max_squared=(N, K, 2), overlap=(N, K, 3), dice=(N, K))
    for f in FIELDS:
        t = getattr(got, f)
        assert t.is_cuda and tuple(t.shape) == shapes[f], f
        assert t.dtype == (torch.int64 if f in ("surface_voxels", "overlap") else torch.float64 if f == "max_squared" else torch.float32), f
    assert torch.equal(got.surface_voxels.cpu(), want.surface_voxels), what
    assert torch.equal(got.overlap.cpu(), want.overlap), what
    if sampled:
        _relative_close(got.max_squared, want.max_squared, 2 * SAMPLING_TOL, what + " max_squared")
    else:
        _relative_close(got.max_squared, want.max_squared, 0.0, what + " max_squared")
    for f in FLOATS:
        _relative_close(getattr(got, f), getattr(want, f), ULP if (not sampled or f == "dice") else SAMPLING_TOL, "%s %s" % (what, f))


@functools.lru_cache(maxsize=None)
def _case(K, shape, sampled=False):
    p, y = pair_of(K, shape)
    return p, y, directed_squares(p, y, K, SAMPLING[len(shape) - 1] if sampled else None)


@functools.lru_cache(maxsize=None)
def _reference(K, shape, sampled=False, q=95.0):
    return metrics_of(_case(K, shape, sampled)[2], shape[0], K, q)


ALL_CASES = CASES + [(2, FAR_SHAPE)]


@pytest.mark.parametrize("K,shape", ALL_CASES, ids=[case_id(c) for c in ALL_CASES])
def test_metrics_against_brute_force(K, shape):
    M = _M()
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    want = _reference(K, shape)
    got = M.surface_distance_metrics(pd, yd, K)
    assert isinstance(got, M.SurfaceMetrics)
    _against(got, want, False, "K=%d %s" % (K, shape))
    if K >= 4:                                                # class K-1 is in neither map, class K-2 not in pred
        assert bool(torch.isnan(got.hausdorff[:, K - 1]).all()) and bool(torch.isnan(got.dice[:, K - 1]).all())
        assert bool((got.surface_voxels[:, K - 2, 0] == 0).all())
        present = got.surface_voxels[:, K - 2, 1] > 0
        assert bool(present.any()) and bool(torch.isinf(got.directed[:, K - 2][present]).all())
        assert bool((got.dice[:, K - 2][present] == 0).all())
    if shape == FAR_SHAPE:
        assert float(got.max_squared[0, 0].min()) > 2 ** 24 and float(got.max_squared[0, 0, 0]) % 2 == 1     # no fp32 holds it
    if shape == (1, 600, 9):
        assert float(got.max_squared.max()) > 2 ** 16
    s = SAMPLING[len(shape) - 1]
    _against(M.surface_distance_metrics(pd, yd, K, sampling=s), _reference(K, shape, True), True, "sampling K=%d %s" % (K, shape))


@pytest.mark.parametrize("K,shape", [(4, (3, 36, 57)), (2, (1, 600, 9)), (4, (2, 6, 10, 70)), (2, FAR_SHAPE)],
                         ids=["2d", "column", "3d", "far"])
def test_percentiles(K, shape):
    M = _M()
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    for q in PERCENTILES:
        got = M.surface_distance_metrics(pd, yd, K, percentile=q)
        _against(got, _reference(K, shape, False, q), False, "q=%g K=%d %s" % (q, K, shape))
        if q == 100.0:
            assert _same_bits([got.directed[..., 1], got.hausdorff_percentile], [got.directed[..., 0], got.hausdorff])
        if q == 0.0:
            sq = _case(K, shape)[2]
            for (n, k), v in sq.items():
                if v[2] and v[3]:
                    for d in range(2):
                        assert float(got.directed[n, k, d, 1]) == float(torch.tensor(float(v[d].min()), dtype=torch.float64).sqrt().float())
    got = M.surface_distance_metrics(pd, yd, K, sampling=SAMPLING[len(shape) - 1], percentile=37.5)
    _against(got, _reference(K, shape, True, 37.5), True, "sampling q=37.5 K=%d %s" % (K, shape))


@pytest.mark.parametrize("shape", [(1, 600, 9), FAR_SHAPE], ids=["third-digit", "fourth-digit"])
def test_percentile_between_two_top_digits(shape):
    """The borders of class 1 coincide but for one far speck of pred: with q = 100 (m - 1.5) / (m - 1), j = m - 2 and g = 0.5, the
    two order statistics are 0 and the far distance and the value is their midpoint."""
    M = _M()
    p, y = speck_pair(shape)
    sq = directed_squares(p, y, 2)
    m = sq[(0, 1)][2]
    far = float(sq[(0, 1)][0].max())
    assert m >= 3 and int((sq[(0, 1)][0] == 0).sum()) == m - 1 and far > (2 ** 24 if shape == FAR_SHAPE else 2 ** 16)
    q = 100.0 * (m - 1.5) / (m - 1)
    got = M.surface_distance_metrics(p.to(DEV), y.to(DEV), 2, percentile=q)
    _against(got, metrics_of(sq, 1, 2, q), False, "speck %s" % (shape,))
    assert float(got.max_squared[0, 1, 0]) == far
    assert abs(float(got.directed[0, 1, 0, 1]) / (0.5 * far ** 0.5) - 1) <= ULP
    assert float(got.directed[0, 1, 1, 1]) == 0.0 and float(got.hausdorff_percentile[0, 1]) == float(got.directed[0, 1, 0, 1])


def test_a_segment_with_a_single_border_voxel():
    M = _M()
    y = torch.zeros(1, 9, 70, dtype=torch.int64)
    p = y.clone()
    y[0, 2, 3] = 1
    p[0, 7, 66] = 1
    for q in PERCENTILES:
        got = M.surface_distance_metrics(p.to(DEV), y.to(DEV), 2, percentile=q)
        _against(got, metrics_of(directed_squares(p, y, 2), 1, 2, q), False, "single q=%g" % q)
        assert got.surface_voxels[0, 1].tolist() == [1, 1] and float(got.max_squared[0, 1, 0]) == 25 + 63 * 63
        assert _same_bits([got.directed[0, 1, :, 1]], [got.directed[0, 1, :, 0]])


def test_equal_maps_have_zero_distance_and_unit_dice():
    M = _M()
    for K, shape in ((4, (3, 36, 57)), (4, (2, 6, 10, 70))):
        _, y, _ = _case(K, shape)
        yd = y.to(DEV)
        got = M.surface_distance_metrics(yd, yd.clone(), K)
        there = got.surface_voxels[..., 0] > 0
        assert bool(there.any()) and torch.equal(got.surface_voxels[..., 0], got.surface_voxels[..., 1])
        for f in ("hausdorff", "hausdorff_percentile", "assd"):
            assert bool((getattr(got, f)[there] == 0).all()) and bool(torch.isnan(getattr(got, f)[~there]).all())
        assert bool((got.directed[there] == 0).all()) and bool((got.max_squared[there] == 0).all())
        assert bool((got.dice[there] == 1).all())


def test_empty_borders_and_voxels_without_a_class():
    M = _M()
    y = torch.zeros(2, 5, 5, dtype=torch.int64)
    p = y.clone()
    y[0, 2, 2] = -100                       # no class: its four neighbours become border voxels of class 0
    p[0, 2, 2] = 5                          # out of range (K = 3): the same
    p[1, 1, 1] = 1                          # class 1 in pred only (entry 1); class 2 nowhere
    got = M.surface_distance_metrics(p.to(DEV), y.to(DEV), 3)
    assert got.surface_voxels[0, 0].tolist() == [20, 20] and got.overlap[0, 0].tolist() == [24, 24, 24]
    assert float(got.hausdorff[0, 0]) == 0.0 and float(got.dice[0, 0]) == 1.0
    assert got.surface_voxels[1, 1].tolist() == [1, 0] and got.overlap[1, 1].tolist() == [1, 0, 0]
    for f in ("hausdorff", "hausdorff_percentile", "assd"):
        assert float(getattr(got, f)[1, 1]) == float("inf")
        assert bool(torch.isnan(getattr(got, f)[:, 2]).all())
    assert bool(torch.isinf(got.directed[1, 1]).all()) and bool(torch.isinf(got.max_squared[1, 1]).all())
    assert bool(torch.isnan(got.directed[:, 2]).all()) and bool(torch.isnan(got.max_squared[:, 2]).all())
    assert float(got.dice[1, 1]) == 0.0 and bool(torch.isnan(got.dice[:, 2]).all())
    assert got.surface_voxels[:, 2].tolist() == [[0, 0], [0, 0]]
    _against(got, metrics_of(directed_squares(p, y, 3), 2, 3, 95.0), False, "conventions")


def test_the_short_forms_return_the_fields():
    M = _M()
    K, shape = 4, (3, 36, 57)
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    s = SAMPLING[2]
    for kw in (dict(), dict(sampling=s)):
        full = M.surface_distance_metrics(pd, yd, K, percentile=80.0, **kw)
        assert _same_bits([M.hausdorff_distance(pd, yd, K, **kw)], [full.hausdorff])
        assert _same_bits([M.hausdorff_distance(pd, yd, K, percentile=80.0, **kw)], [full.hausdorff_percentile])
        assert _same_bits([M.average_surface_distance(pd, yd, K, **kw)], [full.assd])
        assert _same_bits([M.average_surface_distance(pd, yd, K, symmetric=False, **kw).contiguous()],
                          [full.directed[:, :, 0, 2].contiguous()])
    assert not M.hausdorff_distance(pd, yd, K).requires_grad


def test_runs_are_bitwise_identical_and_a_captured_graph_replays_them():
    M = _M()
    K, shape = 4, (3, 36, 57)
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)

    def step():
        return tuple(M.surface_distance_metrics(pd, yd, K)) + tuple(M.surface_distance_metrics(pd, yd, K, sampling=(1.5, 0.7),
                                                                                                 percentile=37.5))

    eager = step()
    again = step()
    assert _same_bits(eager, again)
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
    assert _same_bits(static, eager)
    with torch.no_grad():
        pd.copy_(yd)
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(static, step())
    assert float(static[0][0, 0]) == 0.0


def _offset_copy(t):
    """The same values one element further into a fresh storage."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("K,shape", [(4, (3, 36, 57)), (4, (2, 6, 10, 70))], ids=["2d", "3d"])
def test_offset_and_non_contiguous_inputs_give_the_same_bits(K, shape):
    M = _M()
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    want = M.surface_distance_metrics(pd, yd, K)
    assert _same_bits(M.surface_distance_metrics(_offset_copy(pd), _offset_copy(yd), K), want)
    pt = pd.transpose(1, 2).contiguous().transpose(1, 2)
    yt = yd.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not pt.is_contiguous() and not yt.is_contiguous()
    assert _same_bits(M.surface_distance_metrics(pt, yt, K), want)


def test_tensors_on_another_device_than_the_current_one():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    M = _M()
    K, shape = 4, (3, 36, 57)
    p, y, _ = _case(K, shape)
    want = M.surface_distance_metrics(p.to(DEV), y.to(DEV), K)
    assert torch.cuda.current_device() == 0
    got = M.surface_distance_metrics(p.to("cuda:1"), y.to("cuda:1"), K)
    torch.cuda.synchronize("cuda:1")
    assert all(t.device == torch.device("cuda:1") for t in got)
    assert _same_bits(got, want)
    with pytest.raises(RuntimeError, match="same device"):
        M.surface_distance_metrics(p.to("cuda:1"), y.to(DEV), K)


def test_refusals_on_the_device():
    M = _M()
    y = torch.zeros(1, 2, 40000, device=DEV, dtype=torch.int64)
    with pytest.raises(NotImplementedError):
        M.surface_distance_metrics(y, y, 2)
    y = torch.zeros(1, 8, 8, device=DEV, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="int64"):
        M.surface_distance_metrics(y.int(), y, 2)
    with pytest.raises(RuntimeError, match="int64"):
        M.hausdorff_distance(y, y.float(), 2)
