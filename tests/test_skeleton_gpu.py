"""soft_skeletonize / cldice_loss on the HIP kernels (csrc/seg_skeleton.hip) against the forms of tests/skeleton_forms.py.

Skeleton values are compared bit for bit with the fp32 stacked form on the CPU (min, max and relu are exact and every other
operation is rounded once); gradients with float64 autograd of the same form, which has the kernels' tie rule, to 1e-5 of
the largest |expected| (TOL_G of tests/test_dice_gpu.py).  The loss is held to the bounds of tests/test_dice_gpu.py -- value
within 2e-5 absolute, gradient within 1e-5 of the largest |expected| -- on logits whose softmax keeps every selection at least
1e-5 from flipping (skeleton_forms.margin_logits; asserted per case), about 30 times what the fp32 softmax perturbs."""
import pytest
import torch

from tests.skeleton_forms import cldice_closed, margin_logits, selection_margin, soft_skeleton_stacked

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TOL_V, TOL_G = 2e-5, 1e-5


def _L():
    import advchain.common.loss as L
    return L


def _ops():
    from advchain_amd import ops
    return ops


def _grads_of(fn, *leaves):
    v = fn()
    return v.detach(), torch.autograd.grad(v, leaves)


def _grad_close(got, want, what):
    want = want.detach().double().cpu()
    err = float((got.detach().double().cpu() - want).abs().max())
    scale = max(float(want.abs().max()), 1e-30)
    print("%s: gradient |diff| %.3g of max %.3g" % (what, err, scale))
    assert err <= TOL_G * scale, (what, err, scale)


# ---- skeleton values and gradients -----------------------------------------------------------------------------------------
SKEL_SHAPES = [(1, 1, 1, 1),
               (1, 1, 1, 40),
               (2, 3, 5, 7),
               (2, 2, 70, 75),          # several tiles each way, ragged edges, halos across the tile seams
               (1, 2, 3, 4, 5),
               (1, 2, 20, 24, 40),
               (1, 1, 2, 3, 2),         # smaller than the halo in every axis
               (1, 1, 3, 3)]


def _past_fused():
    return _ops().SKELETON_FUSED_MAX_ITERATIONS + 1


def _check_skeleton(x_cpu, iterations, what, route=None):
    x = x_cpu.to(DEV).requires_grad_(True)
    cot = torch.randn(x_cpu.shape, generator=torch.Generator().manual_seed(1))
    if route is None:
        out = _L().soft_skeletonize(x, iterations=iterations)
    else:
        out = _ops().soft_skeletonize(x, iterations=iterations, route=route)
    assert out.dtype == torch.float32 and out.shape == x.shape
    want = soft_skeleton_stacked(x_cpu, iterations)
    assert torch.equal(out.detach().cpu(), want), (what, float((out.detach().cpu() - want).abs().max()))
    g, = torch.autograd.grad(out, x, cot.to(DEV))
    assert g.dtype == torch.float32 and g.shape == x.shape
    x64 = x_cpu.double().requires_grad_(True)
    gw, = torch.autograd.grad(soft_skeleton_stacked(x64, iterations), x64, cot.double())
    _grad_close(g, gw, what)
    return out.detach()


@pytest.mark.parametrize("shape", SKEL_SHAPES, ids=["x".join(map(str, s)) for s in SKEL_SHAPES])
def test_skeleton_bits_and_gradient(shape):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(len(shape) + shape[-1]))
    for iterations in (0, 1, 3, 10, _past_fused()):
        _check_skeleton(x, iterations, "%s iterations=%d" % (shape, iterations))


@pytest.mark.parametrize("shape", [(2, 2, 70, 75), (1, 2, 20, 24, 40), (1, 1, 2, 3, 2)], ids=["2d", "3d", "tiny3d"])
def test_fused_and_level_routes_have_the_same_bits(shape):
    ops = _ops()
    x = torch.rand(shape, generator=torch.Generator().manual_seed(3))
    for iterations in (0, 3, ops.SKELETON_FUSED_MAX_ITERATIONS):
        a = _check_skeleton(x, iterations, "fused %s %d" % (shape, iterations), route="fused")
        b = _check_skeleton(x, iterations, "levels %s %d" % (shape, iterations), route="levels")
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.soft_skeletonize(x.to(DEV), iterations=_past_fused(), route="fused")
    with pytest.raises(ValueError):
        ops.soft_skeletonize(x.to(DEV), iterations=1, route="tiles")


def test_every_iteration_count_up_to_the_limit_runs():
    x = torch.rand((1, 2, 9, 11), generator=torch.Generator().manual_seed(4))
    for iterations in (2, 4, 11, 32):
        _check_skeleton(x, iterations, "iterations=%d" % iterations)
    x3 = torch.rand((1, 1, 5, 6, 7), generator=torch.Generator().manual_seed(5))
    _check_skeleton(x3, 32, "3d iterations=32")


def _cross_and_plateau(nd):
    shape = (1, 2) + (13,) * nd if nd == 2 else (1, 2, 9, 11, 13)
    x = torch.zeros(shape)
    c = [s // 2 for s in shape[2:]]
    if nd == 2:
        x[0, 0, c[0], 1:-1] = 1
        x[0, 0, 1:-1, c[1]] = 1                  # a hard cross: its soft skeleton loses the centre
        x[0, 1, 3:9, 2:11] = 1                   # a plateau
        x[0, 1, 5, 5] = 0.5
    else:
        x[0, 0, c[0], c[1], 1:-1] = 1
        x[0, 0, c[0], 1:-1, c[2]] = 1
        x[0, 0, 1:-1, c[1], c[2]] = 1
        x[0, 1, 2:7, 3:9, 2:11] = 1
        x[0, 1, 4, 5, 6] = 0.25
    return x


@pytest.mark.parametrize("nd", [2, 3], ids=["2d", "3d"])
def test_ties_on_hard_masks_follow_the_stated_rule(nd):
    x = _cross_and_plateau(nd)
    for iterations in (0, 1, 3, _past_fused()):
        _check_skeleton(x, iterations, "hard mask %dd iterations=%d" % (nd, iterations))
    # the known artefact: the skeleton of a hard cross breaks at the junction -- without iterations it loses the
    # centre, with them the centre comes back and the arm voxels next to it stay lost
    c = tuple(s // 2 for s in x.shape[2:])
    beside = c[:-1] + (c[-1] + 1,)
    skel = _L().soft_skeletonize(x.to(DEV), iterations=0).cpu()
    assert float(skel[(0, 0) + c]) == 0.0 and float(skel[(0, 0) + beside]) == 0.0
    skel = _L().soft_skeletonize(x.to(DEV), iterations=3).cpu()
    assert float(skel[(0, 0) + c]) == 1.0 and float(skel[(0, 0) + beside]) == 0.0


# ---- cldice_loss against the float64 form ---------------------------------------------------------------------------------
def _labels(shape, seed, ignored=0.0, top=None):
    g = torch.Generator().manual_seed(1000 + seed)
    N, K = shape[:2]
    y = torch.randint(0, K if top is None else top, (N,) + tuple(shape[2:]), generator=g)
    if ignored:
        y[torch.rand(y.shape, generator=g) < ignored] = -100
    return y


def _against_closed(x_cpu, tgt_cpu, opt, counted_first, what, scale=1.0):
    iterations = opt.get("iterations", 3)
    p64 = torch.softmax(x_cpu.double(), 1)
    margin = selection_margin(p64[:, counted_first:], iterations)
    print("%s: selection margin %.3g" % (what, margin))
    assert margin >= 1e-5, (what, margin)
    x = x_cpu.to(DEV).requires_grad_(True)
    tgt = tgt_cpu.to(DEV)
    v, (g,) = _grads_of(lambda: scale * _L().cldice_loss(x, tgt, **opt), x)
    assert v.dtype == torch.float32 and v.dim() == 0 and g.dtype == x.dtype and g.shape == x.shape
    x64 = x_cpu.double().requires_grad_(True)
    w, (gw,) = _grads_of(lambda: scale * cldice_closed(x64, tgt_cpu, **opt), x64)
    print("%s: value %.9g, float64 %.9g, |diff| %.3g" % (what, float(v), float(w), abs(float(v) - float(w))))
    assert abs(float(v) - float(w)) <= TOL_V * abs(scale), (what, float(v), float(w))
    _grad_close(g, gw, what)


CASES = [((2, 2, 17, 23), 3, False),
         ((1, 2, 9, 11, 13), 3, False),
         ((1, 2, 9, 11, 13), 10, False),
         ((2, 3, 17, 23), 3, True),
         ((2, 4, 40, 70), 3, True),
         ((1, 3, 20, 24, 40), 3, True)]


@pytest.mark.parametrize("shape,iterations,ign", CASES, ids=["%s-it%d" % ("x".join(map(str, c[0])), c[1]) for c in CASES])
def test_loss_against_the_float64_form(shape, iterations, ign):
    x = margin_logits(shape, seed=iterations + shape[1]).float()
    first = 1 if ign else 0
    K = shape[1]
    y = _labels(shape, 1)
    what = "%s iterations=%d" % (shape, iterations)
    _against_closed(x, y, dict(iterations=iterations, ignore_background=ign), first, what + " labels")
    _against_closed(x, _labels(shape, 2, ignored=0.1), dict(iterations=iterations, ignore_background=ign, batch=True, smooth=0.3),
                    first, what + " ignored voxels, batch")
    t = torch.softmax(torch.randn(shape, generator=torch.Generator().manual_seed(7)) * 3, 1)
    _against_closed(x, t, dict(iterations=iterations, ignore_background=ign), first, what + " soft target", scale=-2.5)
    if K >= 3:
        w = [0.5, 0.0, 1.5, 0.75][:K]
        xw = x.clone()
        _against_closed(xw, y, dict(iterations=iterations, ignore_background=True, weight=w), 2, what + " weights")


def test_two_class_pooled_case_is_the_published_loss():
    from tests.skeleton_forms import one_hot_no_class, soft_cldice_published
    shape = (2, 2, 17, 23)
    x = margin_logits(shape, seed=9).float()
    y = _labels(shape, 3)
    v = _L().cldice_loss(x.to(DEV), y.to(DEV), iterations=3, ignore_background=True, batch=True, smooth=1.0)
    w = soft_cldice_published(one_hot_no_class(y, 2, torch.float64), torch.softmax(x.double(), 1), 3, 1.0)
    assert abs(float(v) - float(w)) <= TOL_V


def test_smooth_zero_and_an_empty_class_give_nan():
    shape = (2, 3, 17, 23)
    x = margin_logits(shape, seed=11).float().to(DEV)
    y = _labels(shape, 4, top=2).to(DEV)                   # class 2 absent: its target skeleton is empty
    assert torch.isnan(_L().cldice_loss(x, y, smooth=0.0, ignore_background=True))
    assert torch.isfinite(_L().cldice_loss(x, y, smooth=1e-3, ignore_background=True))


def test_labels_outside_the_classes_are_in_no_class():
    shape = (1, 3, 9, 12)
    x = margin_logits(shape, seed=12).float()
    y = _labels(shape, 5)
    y[0, :2] = 7
    y[0, 2] = -3
    _against_closed(x, y, dict(iterations=2), 1, "labels outside [0, K)")


def test_misaligned_storage_gives_the_same_bits():
    L = _L()
    shape = (2, 3, 17, 24)
    x = margin_logits(shape, seed=13).float()
    y = _labels(shape, 6, ignored=0.1).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        n = x.numel()
        a = torch.empty(n + 1, device=DEV, dtype=dtype)
        b = torch.empty(n + 1, device=DEV, dtype=dtype)
        a[:n] = x.reshape(-1).to(DEV).to(dtype)
        b[1:] = a[:n]
        xa = a[:n].view(shape).detach().requires_grad_(True)
        xo = b[1:].view(shape).detach().requires_grad_(True)
        assert xa.data_ptr() % 16 == 0 and xo.data_ptr() % 16 != 0 and xo.is_contiguous()
        va, (ga,) = _grads_of(lambda: L.cldice_loss(xa, y), xa)
        vo, (go,) = _grads_of(lambda: L.cldice_loss(xo, y), xo)
        assert torch.equal(va, vo) and torch.equal(ga, go)


# ---- bf16, reproducibility, capture, device guard ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 33, 47), (1, 2, 6, 10, 21)], ids=["2d", "3d"])
def test_bf16_logits_are_the_fp32_call_on_the_upcast(shape):
    L = _L()
    g = torch.Generator().manual_seed(21)
    xb = (torch.randn(shape, generator=g) * 2).to(DEV).to(torch.bfloat16).requires_grad_(True)
    x32 = xb.detach().float().requires_grad_(True)
    y = _labels(shape, 8, ignored=0.1).to(DEV)
    t = torch.softmax(torch.randn(shape, generator=g) * 3, 1).to(DEV)
    for tgt in (y, t):
        for iterations in (3, _past_fused()):
            vb, (gb,) = _grads_of(lambda: L.cldice_loss(xb, tgt, iterations=iterations), xb)
            v32, (g32,) = _grads_of(lambda: L.cldice_loss(x32, tgt, iterations=iterations), x32)
            assert vb.dtype == torch.float32 and gb.dtype == torch.bfloat16
            assert torch.equal(vb, v32), (float(vb), float(v32))
            assert torch.equal(gb, g32.bfloat16())


def test_loss_routes_have_the_same_bits():
    ops = _ops()
    for shape in ((2, 3, 70, 75), (1, 2, 10, 12, 40)):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(22)).to(DEV).requires_grad_(True)
        y = _labels(shape, 9).to(DEV)
        va, (ga,) = _grads_of(lambda: ops.cldice_loss(x, y, route="fused"), x)
        vb, (gb,) = _grads_of(lambda: ops.cldice_loss(x, y, route="levels"), x)
        assert torch.equal(va, vb) and torch.equal(ga, gb)


def test_runs_are_bitwise_identical_and_a_captured_graph_replays_them():
    L = _L()
    shape = (2, 3, 36, 57)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(23)).to(DEV).requires_grad_(True)
    y = _labels(shape, 10, ignored=0.1).to(DEV)
    w = torch.rand(3, device=DEV) + 0.5

    def step():
        return _grads_of(lambda: L.cldice_loss(x, y, weight=w), x)

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


def test_no_memset_and_no_copy_in_the_device_activity():
    from torch.profiler import ProfilerActivity, profile
    L = _L()
    shape = (2, 3, 36, 57)
    x = torch.randn(shape, device=DEV, requires_grad=True)
    y = _labels(shape, 11).to(DEV)
    one = torch.ones((), device=DEV)
    torch.autograd.grad(L.cldice_loss(x, y), x, grad_outputs=one)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.autograd.grad(L.cldice_loss(x, y), x, grad_outputs=one)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
    print(names)
    assert names and not any(w in n.lower() for n in names for w in ("memset", "memcpy")), names
    assert any("k_skel_tile" in n for n in names) and any("k_skel_bwd" in n for n in names), names


def test_cpu_tensors_are_refused():
    from advchain_amd._lib import AdvchainHipError
    L = _L()
    with pytest.raises(AdvchainHipError):
        L.soft_skeletonize(torch.rand(1, 1, 4, 4))
    with pytest.raises(AdvchainHipError):
        L.cldice_loss(torch.randn(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(AdvchainHipError):
        L.cldice_loss(torch.randn(1, 2, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64))
