"""dice_loss / dice_ce_loss / cross_entropy_3D of common.loss without a GPU: the public names and signatures, the float64 closed
forms of tests/dice_forms.py against plain loops and against autograd (the formula the kernels implement), host-side argument
checks of the C entries, and no CPU path."""
import ctypes
import inspect
import itertools

import pytest
import torch

from tests.dice_forms import (ce_closed_nd, dice_ce_closed, dice_closed, dice_coefficients, dice_from_maps, dice_loop,
                              targets_and_mask)


@pytest.mark.parametrize("pkg", ["advchain.common.loss", "advchain_amd.common.loss"])
def test_public_names_and_signatures(pkg):
    import importlib
    mod = importlib.import_module(pkg)
    sig = inspect.signature(mod.dice_loss)
    assert [(k, p.default) for k, p in sig.parameters.items()] == [
        ("input", inspect.Parameter.empty), ("target", inspect.Parameter.empty), ("weight", None),
        ("ignore_background", False), ("batch_dice", False), ("smooth", 1e-5)]
    sig = inspect.signature(mod.dice_ce_loss)
    assert [(k, p.default) for k, p in sig.parameters.items()] == [
        ("input", inspect.Parameter.empty), ("target", inspect.Parameter.empty), ("weight", None),
        ("ignore_background", False), ("batch_dice", False), ("smooth", 1e-5), ("dice_weight", 1.0), ("ce_weight", 1.0)]
    sig = inspect.signature(mod.cross_entropy_3D)
    assert [(k, p.default) for k, p in sig.parameters.items()] == [
        ("input", inspect.Parameter.empty), ("target", inspect.Parameter.empty), ("weight", None), ("size_average", True)]


def _inputs(shape, soft, seed=0):
    g = torch.Generator().manual_seed(seed)
    N, K = shape[:2]
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 2
    if soft:
        return x, torch.softmax(torch.randn(shape, generator=g, dtype=torch.float64) * 3, 1)
    y = torch.randint(0, max(K - 1, 1), (N,) + tuple(shape[2:]), generator=g)            # class K - 1 is absent
    y[torch.rand(y.shape, generator=g) < 0.1] = -100
    return x, y


OPTIONS = [dict(), dict(batch_dice=True), dict(ignore_background=True, weight=[0.5, 2.0, 0.0, 1.5]),
           dict(batch_dice=True, ignore_background=True, smooth=0.3), dict(weight=[1.0, 0.0, 3.0, 0.25], smooth=0.0)]


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (2, 4, 3, 4, 5)])
def test_closed_form_agrees_with_plain_loops(shape, soft):
    x, tgt = _inputs(shape, soft)
    for opt in OPTIONS:
        a, b = float(dice_closed(x, tgt, **opt)), dice_loop(x, tgt, **opt)
        assert abs(a - b) <= 1e-12, (opt, a, b)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (2, 4, 3, 4, 5)])
def test_gradient_coefficients_agree_with_autograd(shape, soft):
    """dL/dp = A t + B at counted voxels (0 elsewhere) and dL/dt = A p + B: the table the backward kernel reads."""
    x, tgt = _inputs(shape, soft, seed=1)
    t, m = targets_and_mask(x, tgt)
    for opt in OPTIONS:
        p = torch.softmax(x, 1).requires_grad_(True)
        tt = t.clone().requires_grad_(True)
        gp, gt = torch.autograd.grad(dice_from_maps(p, tt, m, **opt), (p, tt))
        A, B = dice_coefficients(p.detach(), t, m, **opt)
        bshape = A.shape + (1,) * (x.dim() - 2)
        A, B = A.reshape(bshape), B.reshape(bshape)
        assert float((gp - (A * t + B) * m).abs().max()) <= 1e-10, opt
        assert float((gt - (A * p.detach() + B) * m).abs().max()) <= 1e-10, opt


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (2, 4, 3, 4, 5)])
def test_fused_form_is_the_sum_of_its_parts(shape, soft):
    x, tgt = _inputs(shape, soft, seed=2)
    for opt in OPTIONS:
        w = opt.get("weight")
        fused = dice_ce_closed(x, tgt, dice_weight=0.7, ce_weight=1.3, **opt)
        parts = 1.3 * ce_closed_nd(x, tgt, w) + 0.7 * dice_closed(x, tgt, **opt)
        assert abs(float(fused) - float(parts)) <= 1e-12, opt


def test_c_entries_reject_bad_arguments_on_the_host():
    from advchain_amd import _lib
    lib = _lib.load()
    d2, d3 = _lib.dims_array((8, 8)), _lib.dims_array((4, 8, 8))
    bad = _lib.dims_array((0, 8))
    p = ctypes.c_void_p(16)            # never dereferenced: every call below fails validation before any launch
    assert lib.advchain_dice_workspace(2, 4, 4, d2) < 0
    assert lib.advchain_dice_workspace(2, 4, 2, bad) < 0
    assert lib.advchain_dice_workspace(2, 0, 2, d2) < 0
    assert lib.advchain_dice_workspace(0, 4, 2, d2) < 0
    assert lib.advchain_dice_workspace(2, 65536, 2, d2) < 0
    huge = _lib.dims_array((1 << 24, 1 << 16, 1))                 # 2^40 voxels: with N = K = 65535 the sizes leave int64
    assert lib.advchain_dice_workspace(65535, 65535, 3, huge) < 0
    assert lib.advchain_dice_workspace(1, 1, 3, huge) > 0
    assert lib.advchain_dice_workspace(2, 4, 2, d2) > 0
    assert lib.advchain_dice_workspace(2, 4, 3, d3) > 0

    def fwd(x=p, bf16=0, lab=p, soft=None, ws=p, value=p, N=2, K=4, ndim=2, dims=d2, flags=0, smooth=1e-5):
        return lib.advchain_dice_fwd(x, bf16, lab, soft, None, p, p, ws, value, N, K, ndim, dims, flags, smooth, 1.0, 1.0, None)

    def bwd(x=p, bf16=0, lab=p, soft=None, lse=p, coef=p, gx=p, gt=None, N=2, K=4, ndim=2, dims=d2):
        return lib.advchain_dice_bwd(x, bf16, lab, soft, None, lse, coef, None, gx, gt, N, K, ndim, dims, 1.0, 1.0, None)

    cases = [
        (lambda: fwd(x=None), b"null"), (lambda: fwd(ws=None), b"null"), (lambda: fwd(value=None), b"null"),
        (lambda: fwd(soft=p), b"exactly one"), (lambda: fwd(lab=None), b"exactly one"),
        (lambda: fwd(K=0), b"K"), (lambda: fwd(K=65536), b"K"),
        (lambda: fwd(dims=bad), b"dims"), (lambda: fwd(ndim=4), b"dims"), (lambda: fwd(ndim=1), b"dims"),
        (lambda: fwd(N=0), b"dims"), (lambda: fwd(ndim=3, dims=None), b"dims"),
        (lambda: fwd(bf16=2), b"bf16"), (lambda: fwd(bf16=-1), b"bf16"),
        (lambda: fwd(smooth=-1.0), b"smooth"), (lambda: fwd(smooth=float("nan")), b"smooth"),
        (lambda: fwd(smooth=float("inf")), b"smooth"),
        (lambda: fwd(flags=4), b"flags"), (lambda: fwd(K=1, flags=1), b"ignore_background"),
        (lambda: bwd(x=None), b"null"), (lambda: bwd(lse=None), b"null"), (lambda: bwd(coef=None), b"null"),
        (lambda: bwd(gx=None), b"null"),
        (lambda: bwd(soft=p), b"exactly one"), (lambda: bwd(lab=None), b"exactly one"),
        (lambda: bwd(gt=p), b"label"),
        (lambda: bwd(K=0), b"K"), (lambda: bwd(dims=bad), b"dims"), (lambda: bwd(ndim=5), b"dims"),
        (lambda: bwd(bf16=3), b"bf16"),
    ]
    for i, (call, word) in enumerate(cases):
        rc = call()
        assert rc < 0, (i, word)
        assert word in lib.advchain_last_error(), (i, word, lib.advchain_last_error())


def test_cpu_tensors_raise():
    from advchain.common.loss import cross_entropy_3D, dice_ce_loss, dice_loss
    from advchain_amd import _lib
    for shape in ((2, 4, 8, 8), (2, 4, 4, 8, 8)):
        x = torch.rand(shape)
        y = torch.randint(0, 4, (2,) + shape[2:])
        for fn in (dice_loss, dice_ce_loss):
            with pytest.raises(_lib.AdvchainHipError):
                fn(x, y)
            with pytest.raises(_lib.AdvchainHipError):
                fn(x, torch.softmax(x, 1), weight=[1.0, 2.0, 1.0, 1.0], batch_dice=True)
    with pytest.raises(_lib.AdvchainHipError):
        cross_entropy_3D(x, y)
    with pytest.raises(_lib.AdvchainHipError):
        cross_entropy_3D(x, torch.softmax(x, 1))


def test_argument_errors_come_before_any_device_work():
    from advchain.common.loss import cross_entropy_3D, dice_ce_loss, dice_loss
    x = torch.rand(2, 4, 8, 8)
    y = torch.randint(0, 4, (2, 8, 8))
    for fn, smooth in itertools.product((dice_loss, dice_ce_loss), (-1e-3, float("nan"), float("inf"))):
        with pytest.raises(ValueError, match="smooth"):
            fn(x, y, smooth=smooth)
    for fn in (dice_loss, dice_ce_loss):
        with pytest.raises(ValueError, match="ignore_background"):
            fn(x[:, :1], y, ignore_background=True)
        with pytest.raises(ValueError, match="weight"):
            fn(x, y, weight=[1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="weight"):
            fn(x, y, weight=torch.ones(5))
        with pytest.raises(ValueError, match="weight"):
            fn(x, y, weight=2.0)
        with pytest.raises(ValueError):
            fn(x[0], y[0])
    with pytest.raises(ValueError):
        cross_entropy_3D(x, y)                                   # 4-D: that is cross_entropy_2D
