"""contour_loss / One_Hot / cross_entropy_2D on the HIP kernels: parity with the reference (g12), the float64 closed forms at
realistic sizes, bf16 logits, bitwise run-to-run reproducibility, soft-target gradients, masks, ignore_index, NaN labels and
a captured graph."""
import numpy as np
import pytest
import torch

from tests.helpers import Fixture
from tests.seg_loss_forms import ce_closed, contour_closed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
G = Fixture("g12_seg_loss")
META = G.json()


def _L():
    import advchain.common.loss as L
    return L


def _rel(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-30)


def _grad_close(got, want, tol=1e-5):
    got = got.detach().double().cpu()
    want = torch.as_tensor(want).double().cpu()
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max())
    assert err <= tol * scale, (err, scale)


@pytest.mark.parametrize("case", META["contour"], ids=[c["name"] for c in META["contour"]])
def test_contour_matches_reference(case):
    n = case["name"]
    x = G.t(n + "__input", DEV).requires_grad_(True)
    tgt = G.t(n + "__target", DEV)
    soft = not case["one_hot_target"]
    if soft:
        tgt = tgt.requires_grad_(True)
    mask = G.t(n + "__mask", DEV) if case["mask"] else None
    v = _L().contour_loss(x, tgt, ignore_background=case["ignore_background"], one_hot_target=case["one_hot_target"],
                          mask=mask)
    v.backward()
    want = G.f(n + "__value")
    assert v.dtype == torch.float32 and v.dim() == 0
    if n == "c2_lab_noign_softmax":
        assert abs(float(v)) < 1e-10
        return
    assert _rel(v, want) <= 2e-5, (float(v), want)
    _grad_close(x.grad, G.arr(n + "__grad_input"))
    if soft:
        _grad_close(tgt.grad, G.arr(n + "__grad_target"))


@pytest.mark.parametrize("case", META["ce"], ids=[c["name"] for c in META["ce"]])
def test_cross_entropy_matches_reference(case):
    n = case["name"]
    x = G.t(n + "__input", DEV).requires_grad_(True)
    tgt = G.t(n + "__target", DEV)
    soft = tgt.dim() == 4
    if soft:
        tgt = tgt.requires_grad_(True)
    w = None
    if case["weight"] == "tensor":
        w = G.t(n + "__weight", DEV)
    elif case["weight"] == "list":
        w = [float(a) for a in G.arr(n + "__weight")]
    v = _L().cross_entropy_2D(x, tgt, weight=w, size_average=case["size_average"])
    v.backward()
    assert _rel(v, G.f(n + "__value")) <= 2e-5, (float(v), G.f(n + "__value"))
    _grad_close(x.grad, G.arr(n + "__grad_input"))
    if soft:
        _grad_close(tgt.grad, G.arr(n + "__grad_target"))


@pytest.mark.parametrize("case", META["one_hot"], ids=[c["name"] for c in META["one_hot"]])
def test_one_hot_matches_reference(case):
    n = case["name"]
    out = _L().One_Hot(case["depth"])(G.t(n + "__labels", DEV))
    want = G.arr(n + "__out")
    assert out.dtype == torch.float32 and tuple(out.shape) == want.shape
    assert np.array_equal(out.cpu().numpy(), want)


def _grads_of(fn, *leaves):
    v = fn()
    gs = torch.autograd.grad(v, leaves)
    return v.detach(), gs


def _check_against_closed(fn, closed, x, others=(), tol_v=2e-5, tol_g=1e-5):
    v, gs = _grads_of(fn, x, *others)
    x64 = x.detach().double().requires_grad_(True)
    o64 = [o.detach().double().requires_grad_(True) for o in others]
    w, gw = _grads_of(lambda: closed(x64, *o64), x64, *o64)
    assert _rel(v, w) <= tol_v, (float(v), float(w))
    for g, gref in zip(gs, gw):
        _grad_close(g, gref, tol_g)


@pytest.mark.parametrize("shape,ign", [((32, 4, 256, 256), True), ((32, 4, 256, 256), False), ((4, 4, 128, 128, 64), True)])
def test_contour_realistic_sizes_against_closed_form(shape, ign):
    torch.manual_seed(0)
    x = torch.softmax(torch.randn(shape, device=DEV) * 2, 1) if ign else torch.rand(shape, device=DEV)
    x.requires_grad_(True)
    y = torch.randint(0, shape[1], (shape[0],) + shape[2:], device=DEV)
    _check_against_closed(lambda: _L().contour_loss(x, y, ignore_background=ign),
                          lambda a: contour_closed(a, y, ign, True, None), x)


@pytest.mark.parametrize("nd", [2, 3])
def test_contour_soft_target_and_masks(nd):
    torch.manual_seed(1)
    shape = (3, 4, 40, 72) if nd == 2 else (2, 4, 12, 20, 70)
    x = torch.softmax(torch.randn(shape, device=DEV), 1).requires_grad_(True)
    t = torch.softmax(torch.randn(shape, device=DEV) * 3, 1).requires_grad_(True)
    for mc in (None, 1, 3, 4) + ((2,) if nd == 3 else ()):
        m = None if mc is None else torch.rand((shape[0], mc) + shape[2:], device=DEV)
        _check_against_closed(lambda: _L().contour_loss(x, t, one_hot_target=False, mask=m),
                              lambda a, b: contour_closed(a, b, True, False, m), x, (t,))


def test_contour_mask_rules():
    x = torch.softmax(torch.randn(2, 4, 16, 16, device=DEV), 1)
    y = torch.randint(0, 4, (2, 16, 16), device=DEV)
    with pytest.raises(ValueError):
        _L().contour_loss(x, y, mask=torch.rand(2, 2, 16, 16, device=DEV))
    m = torch.rand(2, 1, 16, 16, device=DEV, requires_grad=True)
    with pytest.warns(UserWarning):
        _L().contour_loss(x, y, mask=m)
    v = _L().contour_loss(x, y[:, None], mask=torch.ones(2, 1, 16, 16, device=DEV))
    assert torch.equal(v, _L().contour_loss(x, y))


def test_contour_out_of_range_label_gives_nan():
    x = torch.softmax(torch.randn(2, 4, 16, 16, device=DEV), 1)
    y = torch.randint(0, 4, (2, 16, 16), device=DEV)
    y[1, 3, 5] = 7
    assert torch.isnan(_L().contour_loss(x, y))


@pytest.mark.parametrize("K", [4, 16, 17, 40])
def test_cross_entropy_realistic_sizes_against_closed_form(K):
    torch.manual_seed(K)
    N, H, W = (32, 256, 256) if K == 4 else (4, 128, 96)
    x = (torch.randn(N, K, H, W, device=DEV) * 3).requires_grad_(True)
    y = torch.randint(0, K, (N, H, W), device=DEV)
    y[:, :7] = -100
    w = torch.rand(K, device=DEV) + 0.5
    _check_against_closed(lambda: _L().cross_entropy_2D(x, y, weight=w), lambda a: ce_closed(a, y, w), x)
    _check_against_closed(lambda: _L().cross_entropy_2D(x, y), lambda a: ce_closed(a, y), x)


@pytest.mark.parametrize("W", [64, 61])                 # 61: rows that do not split into 4-pixel groups (scalar kernels)
def test_cross_entropy_soft_target_gradients(W):
    torch.manual_seed(W)
    x = (torch.randn(3, 6, 20, W, device=DEV) * 2).requires_grad_(True)
    t = torch.softmax(torch.randn(3, 6, 20, W, device=DEV), 1).requires_grad_(True)
    wl = [0.5, 1.0, 2.0, 1.5, 0.25, 1.0]
    _check_against_closed(lambda: _L().cross_entropy_2D(x, t, weight=wl), lambda a, b: ce_closed(a, b, wl), x, (t,))
    _check_against_closed(lambda: _L().cross_entropy_2D(x, t, size_average=False),
                          lambda a, b: ce_closed(a, b, None, False), x, (t,))
    y = torch.randint(0, 6, (3, 20, W), device=DEV)
    y[0, 0, :5] = -100
    _check_against_closed(lambda: _L().cross_entropy_2D(x, y, weight=torch.tensor(wl, device=DEV)),
                          lambda a: ce_closed(a, y, wl), x)


def test_cross_entropy_ignore_index_and_nan_label():
    x = torch.randn(2, 4, 16, 16, device=DEV)
    y = torch.full((2, 16, 16), -100, dtype=torch.int64, device=DEV)
    xr = x.clone().requires_grad_(True)
    v = _L().cross_entropy_2D(xr, y)
    v.backward()
    assert float(v) == 0.0 and float(xr.grad.abs().max()) == 0.0
    y = torch.randint(0, 4, (2, 16, 16), device=DEV)
    y[0, 2, 3] = 4
    assert torch.isnan(_L().cross_entropy_2D(x, y))
    with pytest.raises(RuntimeError):
        _L().cross_entropy_2D(x, y.int())
    with pytest.raises(ValueError):
        _L().cross_entropy_2D(x[0], y[0])


@pytest.mark.parametrize("K", [4, 17])
def test_cross_entropy_bf16_logits(K):
    torch.manual_seed(3)
    xb = (torch.randn(8, K, 64, 64, device=DEV) * 3).to(torch.bfloat16).requires_grad_(True)
    y = torch.randint(0, K, (8, 64, 64), device=DEV)
    x32 = xb.detach().float().requires_grad_(True)
    vb = _L().cross_entropy_2D(xb, y)
    v32 = _L().cross_entropy_2D(x32, y)
    assert vb.dtype == torch.float32
    assert _rel(vb, v32) <= 1e-5
    vb.backward()
    v32.backward()
    assert xb.grad.dtype == torch.bfloat16
    _grad_close(xb.grad.float(), x32.grad, 1e-2)        # bf16 rounding of the gradient itself
    t = torch.softmax(torch.randn(8, K, 64, 64, device=DEV), 1)
    assert _rel(_L().cross_entropy_2D(xb, t), _L().cross_entropy_2D(x32, t)) <= 1e-5


def test_runs_are_bitwise_identical():
    torch.manual_seed(4)
    x = (torch.randn(16, 4, 128, 128, device=DEV) * 2).requires_grad_(True)
    y = torch.randint(0, 4, (16, 128, 128), device=DEV)
    p = torch.softmax(torch.randn(4, 4, 32, 48, 40, device=DEV), 1).requires_grad_(True)
    yl = torch.randint(0, 4, (4, 32, 48, 40), device=DEV)
    m = torch.rand(4, 4, 32, 48, 40, device=DEV)
    runs = []
    for _ in range(2):
        a, ga = _grads_of(lambda: _L().cross_entropy_2D(x, y, weight=[1.0, 2.0, 3.0, 0.5]), x)
        b, gb = _grads_of(lambda: _L().contour_loss(p, yl, mask=m), p)
        runs.append((a, ga[0], b, gb[0]))
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_cross_entropy_graph_capture_replays_eager():
    torch.manual_seed(5)
    x = (torch.randn(4, 5, 64, 64, device=DEV) * 2).requires_grad_(True)
    y = torch.randint(0, 5, (4, 64, 64), device=DEV)
    w = torch.rand(5, device=DEV) + 0.5
    v_eager, (g_eager,) = _grads_of(lambda: _L().cross_entropy_2D(x, y, weight=w), x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _grads_of(lambda: _L().cross_entropy_2D(x, y, weight=w), x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        v_static, (g_static,) = _grads_of(lambda: _L().cross_entropy_2D(x, y, weight=w), x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(v_static, v_eager) and torch.equal(g_static, g_eager)
    with torch.no_grad():
        x.mul_(0.5)
    g.replay()
    v2, (g2,) = _grads_of(lambda: _L().cross_entropy_2D(x, y, weight=w), x)
    torch.cuda.synchronize()
    assert torch.equal(v_static, v2) and torch.equal(g_static, g2)
