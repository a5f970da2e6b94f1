"""dice_loss / dice_ce_loss / cross_entropy_3D on the HIP kernels (csrc/seg_dice.hip) against the float64 closed forms of
tests/dice_forms.py: every load path (vector, scalar, tail), run-time K, labels and soft targets, ignored voxels and empty
classes, NaN for bad labels, the fused loss against its definition, bf16 logits and misaligned tensors bit for bit, bitwise
reproducibility, a captured graph, the launch counts and the device guard.

Bounds: a value within 2e-5, absolute, of the float64 closed form, and a gradient within 1e-5 of the largest |expected|; the
closed form evaluated in fp32 stays a factor of ten inside both.  Only the sum over voxels of cross_entropy_3D(size_average=False)
-- thousands, not a mean -- is held to 2e-5 relative, the bound of tests/test_seg_loss_gpu.py for the same sum in 2D."""
import pytest
import torch

from tests.dice_forms import ce_closed_nd, dice_ce_closed, dice_closed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TOL_V, TOL_G = 2e-5, 1e-5


def _L():
    import advchain.common.loss as L
    return L


def _grads_of(fn, *leaves):
    v = fn()
    return v.detach(), torch.autograd.grad(v, leaves)


def _value_close(got, want, what, relative=False):
    got, want = float(got), float(want)
    print("%s: value %.9g, float64 %.9g, |diff| %.3g" % (what, got, want, abs(got - want)))
    assert abs(got - want) <= TOL_V * (abs(want) if relative else 1.0), (what, got, want)


def _grad_close(got, want, what):
    want = want.detach().double()
    err = float((got.detach().double() - want).abs().max())
    scale = max(float(want.abs().max()), 1e-30)
    print("%s: gradient |diff| %.3g of max %.3g" % (what, err, scale))
    assert err <= TOL_G * scale, (what, err, scale)


def _against_closed(fn, closed, x, others, what, relative=False):
    v, gs = _grads_of(fn, x, *others)
    assert v.dtype == torch.float32 and v.dim() == 0
    x64 = x.detach().double().requires_grad_(True)
    o64 = [o.detach().double().requires_grad_(True) for o in others]
    w, gw = _grads_of(lambda: closed(x64, *o64), x64, *o64)
    _value_close(v, w, what, relative)
    for g, gref, leaf in zip(gs, gw, (x,) + tuple(others)):
        assert g.dtype == leaf.dtype and g.shape == leaf.shape
        _grad_close(g, gref, what)


def _case(shape, soft, seed=0):
    """Random logits (loss of order 1); labels leave the last class out and have 10 % of voxels at -100."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    N, K = shape[:2]
    x = (torch.randn(shape, generator=g) * 2).to(DEV).requires_grad_(True)
    if soft:
        t = torch.softmax(torch.randn(shape, generator=g) * 3, 1).to(DEV).requires_grad_(True)
        return x, t
    y = torch.randint(0, max(K - 1, 1), (N,) + tuple(shape[2:]), generator=g)
    y[torch.rand(y.shape, generator=g) < 0.1] = -100
    return x, y.to(DEV)


def _weights(K):
    w = [0.5 + 0.25 * (k % 5) for k in range(K)]
    if K >= 3:
        w[1] = 0.0
    return w


SHAPES = [(2, 3, 5, 7),            # V = 35: scalar loads, odd K
          (3, 4, 36, 57),          # V = 2052: three workgroups per entry, a 4-voxel tail
          (2, 5, 6, 10, 70),       # 3D
          (2, 20, 33, 31),         # run-time K over a chunk of classes, odd V
          (1, 70, 8, 8),           # more classes than lanes in a wave
          (2, 1, 8, 8)]            # one class


@pytest.mark.parametrize("soft", [False, True], ids=["labels", "soft"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_against_float64_forms(shape, soft):
    K = shape[1]
    x, tgt = _case(shape, soft, seed=K)
    others = (tgt,) if soft else ()
    for batch_dice in (False, True):
        for ign in ((False,) if K == 1 else (False, True)):
            for w in (None, _weights(K)):
                opt = dict(weight=w, ignore_background=ign, batch_dice=batch_dice)
                what = "%s soft=%s batch=%s ign=%s w=%s" % (shape, soft, batch_dice, ign, w is not None)
                _against_closed(lambda: _L().dice_loss(x, tgt, **opt),
                                lambda a, *b: dice_closed(a, b[0] if soft else tgt, **opt), x, others, "dice " + what)
                fused = dict(opt, dice_weight=0.7, ce_weight=1.3, smooth=0.05)
                _against_closed(lambda: _L().dice_ce_loss(x, tgt, **fused),
                                lambda a, *b: dice_ce_closed(a, b[0] if soft else tgt, **fused), x, others, "dice_ce " + what)


@pytest.mark.parametrize("soft", [False, True], ids=["labels", "soft"])
def test_cross_entropy_3d_against_float64_form(soft):
    x, tgt = _case((2, 5, 6, 10, 70), soft, seed=3)
    others = (tgt,) if soft else ()
    for w, avg in ((None, True), (_weights(5), True), (torch.tensor(_weights(5), device=DEV), False)):
        _against_closed(lambda: _L().cross_entropy_3D(x, tgt, weight=w, size_average=avg),
                        lambda a, *b: ce_closed_nd(a, b[0] if soft else tgt, w, avg), x, others, "ce3d soft=%s" % soft,
                        relative=not avg)
    with pytest.raises(ValueError):
        _L().cross_entropy_3D(x[:, :, 0], tgt[:, 0] if not soft else tgt[:, :, 0])
    with pytest.raises(ValueError):
        _L().cross_entropy_2D(x, tgt)


def test_ignored_voxels_and_empty_classes():
    shape = (3, 4, 36, 57)
    x, y = _case(shape, False, seed=7)           # 10 % ignored, class 3 absent
    y[1] = -100                                  # one entry without a counted voxel
    for fn, closed in ((_L().dice_loss, dice_closed), (_L().dice_ce_loss, dice_ce_closed)):
        for batch_dice in (False, True):
            v, (g,) = _grads_of(lambda: fn(x, y, batch_dice=batch_dice), x)
            assert bool(torch.isfinite(v)) and bool(torch.isfinite(g).all())
            assert float(g[1].abs().max()) == 0.0
            _against_closed(lambda: fn(x, y, batch_dice=batch_dice), lambda a: closed(a, y, batch_dice=batch_dice), x, (),
                            "ignored entry batch=%s" % batch_dice)
    # nothing counted at all: every dice term is smooth / smooth = 1
    v, (g,) = _grads_of(lambda: _L().dice_loss(x[1:2], y[1:2]), x)
    assert float(v) == 0.0 and float(g.abs().max()) == 0.0
    v, (g,) = _grads_of(lambda: _L().dice_ce_loss(x[1:2], y[1:2]), x)
    assert float(v) == 0.0 and float(g.abs().max()) == 0.0
    # a label outside [0, K) that is not -100: NaN, never an address
    for bad in (4, -1, 2 ** 40):
        yb = y.clone()
        yb[0, 2, 3] = bad
        for fn in (_L().dice_loss, _L().dice_ce_loss):
            v, (g,) = _grads_of(lambda: fn(x, yb), x)
            torch.cuda.synchronize()
            assert bool(torch.isnan(v)), (bad, float(v))


def test_refused_inputs():
    from advchain_amd import _lib
    x = torch.randn(2, 4, 8, 8, device=DEV)
    y = torch.randint(0, 4, (2, 8, 8), device=DEV)
    for fn in (_L().dice_loss, _L().dice_ce_loss):
        with pytest.raises(_lib.AdvchainHipError, match="float16"):
            fn(x.half(), y)
        with pytest.raises(_lib.AdvchainHipError):
            fn(x, y.cpu())
        with pytest.raises(RuntimeError):
            fn(x, y.int())
        with pytest.raises(ValueError):
            fn(x, y[:, :4])
        with pytest.raises(ValueError):
            fn(x[:, :1], y, ignore_background=True)


@pytest.mark.parametrize("soft", [False, True], ids=["labels", "soft"])
@pytest.mark.parametrize("shape", [(3, 4, 36, 57), (2, 5, 6, 10, 70)], ids=["2d", "3d"])
def test_dice_ce_is_the_weighted_sum_of_its_parts(shape, soft):
    L = _L()
    K = shape[1]
    x, tgt = _case(shape, soft, seed=11)
    leaves = (x, tgt) if soft else (x,)
    ce = L.cross_entropy_2D if len(shape) == 4 else L.cross_entropy_3D
    for opt in (dict(), dict(weight=_weights(K), ignore_background=True), dict(batch_dice=True, smooth=0.5)):
        v, gs = _grads_of(lambda: 3 * L.dice_ce_loss(x, tgt, dice_weight=0.7, ce_weight=1.3, **opt), *leaves)
        w, gw = _grads_of(lambda: 3 * (1.3 * ce(x, tgt, weight=opt.get("weight")) + 0.7 * L.dice_loss(x, tgt, **opt)), *leaves)
        print("fused %.9g, parts %.9g" % (float(v) / 3, float(w) / 3))
        assert abs(float(v) / 3 - float(w) / 3) <= TOL_V, (opt, float(v) / 3, float(w) / 3)
        for a, b in zip(gs, gw):
            _grad_close(a, b, "fused vs parts %s" % (opt,))


@pytest.mark.parametrize("shape", [(3, 4, 36, 57), (2, 20, 33, 31)], ids=["vector", "scalar"])
def test_bf16_logits_are_the_fp32_call_on_the_upcast(shape):
    L = _L()
    x, y = _case(shape, False, seed=13)
    xb = x.detach().to(torch.bfloat16).requires_grad_(True)
    x32 = xb.detach().float().requires_grad_(True)
    t = torch.softmax(torch.randn(shape, device=DEV), 1)
    for fn in (L.dice_loss, L.dice_ce_loss):
        for tgt in (y, t):
            vb, (gb,) = _grads_of(lambda: fn(xb, tgt, weight=_weights(shape[1])), xb)
            v32, (g32,) = _grads_of(lambda: fn(x32, tgt, weight=_weights(shape[1])), x32)
            assert vb.dtype == torch.float32 and gb.dtype == torch.bfloat16
            assert torch.equal(vb, v32), (float(vb), float(v32))
            assert torch.equal(gb, g32.bfloat16())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_value_does_not_depend_on_alignment(dtype):
    """The same logits at a 16-byte aligned address and one element later (scalar loads of the same four voxels per lane)."""
    L = _L()
    shape = (3, 4, 36, 57)                       # V % 4 == 0
    x, y = _case(shape, False, seed=17)
    n = x.numel()
    a = torch.empty(n + 1, device=DEV, dtype=dtype)
    b = torch.empty(n + 1, device=DEV, dtype=dtype)
    a[:n] = x.detach().reshape(-1).to(dtype)
    b[1:] = a[:n]
    xa = a[:n].view(shape).detach().requires_grad_(True)
    xo = b[1:].view(shape).detach().requires_grad_(True)
    assert xa.data_ptr() % 16 == 0 and xo.data_ptr() % 16 != 0 and xo.is_contiguous()
    ts = torch.softmax(torch.randn(shape, device=DEV), 1)
    fa = torch.empty(n + 1, device=DEV)
    fa[1:] = ts.reshape(-1)
    to = fa[1:].view(shape)
    for fn in (L.dice_loss, L.dice_ce_loss):
        va, (ga,) = _grads_of(lambda: fn(xa, y), xa)
        vo, (go,) = _grads_of(lambda: fn(xo, y), xo)
        assert torch.equal(va, vo) and torch.equal(ga, go)
        va, (ga,) = _grads_of(lambda: fn(xa, ts), xa)
        vo, (go,) = _grads_of(lambda: fn(xa, to), xa)
        assert torch.equal(va, vo) and torch.equal(ga, go)


def test_runs_are_bitwise_identical_and_a_captured_graph_replays_them():
    L = _L()
    x, y = _case((3, 4, 36, 57), False, seed=19)
    w = torch.rand(4, device=DEV) + 0.5

    def step():
        return _grads_of(lambda: L.dice_ce_loss(x, y, weight=w, ignore_background=True), x)

    v_eager, (g_eager,) = step()
    v_again, (g_again,) = step()
    assert torch.equal(v_eager, v_again) and torch.equal(g_eager, g_again)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        v_static, (g_static,) = step()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(v_static, v_eager) and torch.equal(g_static, g_eager)
    with torch.no_grad():
        x.mul_(0.5)
    g.replay()
    v2, (g2,) = step()
    torch.cuda.synchronize()
    assert torch.equal(v_static, v2) and torch.equal(g_static, g2)


def _kernels(prof):
    evs = [e for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
    return [e.name for e in evs if not any(w in e.name.lower() for w in ("memcpy", "memset", "hipmemcpy", "hipmemset"))]


@pytest.mark.parametrize("soft", [False, True], ids=["labels", "soft"])
def test_launch_counts(soft):
    """Kernel records of the device activity (what bench.py counts as launches): at most three forward, exactly one backward."""
    from torch.profiler import ProfilerActivity, profile
    L = _L()
    x, tgt = _case((3, 4, 36, 57), soft, seed=23)
    leaves = (x, tgt) if soft else (x,)
    one = torch.ones((), device=DEV)
    for _ in range(2):
        torch.autograd.grad(L.dice_ce_loss(x, tgt), leaves, grad_outputs=one)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        v = L.dice_ce_loss(x, tgt)
        torch.cuda.synchronize()
    fwd = _kernels(prof)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.autograd.grad(v, leaves, grad_outputs=one)
        torch.cuda.synchronize()
    bwd = _kernels(prof)
    print(fwd, bwd)
    assert 1 <= len(fwd) <= 3 and all("k_dice" in k for k in fwd), fwd
    assert len(bwd) == 1 and "k_dice_bwd" in bwd[0], bwd


def test_tensors_on_another_device_than_the_current_one():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    L = _L()
    x, y = _case((3, 4, 36, 57), False, seed=29)
    v0, (g0,) = _grads_of(lambda: L.dice_ce_loss(x, y), x)
    x1 = x.detach().to("cuda:1").requires_grad_(True)
    y1 = y.to("cuda:1")
    assert torch.cuda.current_device() == 0
    v1, (g1,) = _grads_of(lambda: L.dice_ce_loss(x1, y1), x1)
    c1, (h1,) = _grads_of(lambda: L.cross_entropy_3D(x1[:, :, None], y1[:, None]), x1)
    torch.cuda.synchronize("cuda:1")
    assert v1.device == x1.device and g1.device == x1.device
    assert torch.equal(v1.cpu(), v0.cpu()) and torch.equal(g1.cpu(), g0.cpu())
    c0, (h0,) = _grads_of(lambda: L.cross_entropy_3D(x[:, :, None], y[:, None]), x)
    assert torch.equal(c1.cpu(), c0.cpu()) and torch.equal(h1.cpu(), h0.cpu())
