"""The forms of tests/skeleton_forms.py against each other on the CPU, and the host-side argument checks of
common.loss.soft_skeletonize / cldice_loss (they run before any device work, so a CPU caller sees them).

The stacked form (shifted copies, first extremum) has the values of the published max_pool composition bit for bit in fp32;
on continuous random maps, where no window holds equal values from different voxels, their float64 gradients agree to 1e-12."""
import pytest
import torch

from tests.skeleton_forms import (cldice_closed, margin_logits, one_hot_no_class, selection_margin, soft_cldice_published,
                                  soft_skel, soft_skeleton_stacked)

SHAPES = [(2, 3, 17, 23), (1, 2, 9, 11, 13)]
ITERATIONS = [0, 1, 3, 10]


def _L():
    import advchain.common.loss as L
    return L


@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=["2d", "3d"])
def test_stacked_form_has_the_bits_of_the_published_composition(shape, iterations):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(iterations))
    assert torch.equal(soft_skeleton_stacked(x, iterations), soft_skel(x, iterations))
    hard = (x > 0.6).float()                     # plateaus, lines and isolated voxels: ties everywhere
    assert torch.equal(soft_skeleton_stacked(hard, iterations), soft_skel(hard, iterations))


@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=["2d", "3d"])
def test_gradients_of_the_two_forms_agree_on_continuous_maps(shape, iterations):
    g = torch.Generator().manual_seed(100 + iterations)
    x = torch.rand(shape, generator=g, dtype=torch.float64).requires_grad_(True)
    cot = torch.randn(shape, generator=g, dtype=torch.float64)
    ga, = torch.autograd.grad(soft_skeleton_stacked(x, iterations), x, cot)
    gb, = torch.autograd.grad(soft_skel(x, iterations), x, cot)
    assert float((ga - gb).abs().max()) <= 1e-12


def test_first_extremum_wins_in_the_stacked_form():
    """What the tie rule rests on: min / max over dim 0 return the first index among equal values, and autograd routes there."""
    s = torch.tensor([[1.0], [1.0], [1.0]], dtype=torch.float64, requires_grad=True)
    for fn in (torch.min, torch.max):
        r = fn(s, dim=0)
        assert int(r.indices) == 0
        g, = torch.autograd.grad(r.values.sum(), s)
        assert g.reshape(-1).tolist() == [1.0, 0.0, 0.0]


@pytest.mark.parametrize("shape", [(2, 2, 17, 23), (1, 2, 9, 11, 13)], ids=["2d", "3d"])
def test_pooled_two_class_case_is_the_published_soft_cldice(shape):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g, dtype=torch.float64) * 2
    y = torch.randint(0, 2, (shape[0],) + shape[2:], generator=g)
    for iterations in (0, 3):
        mine = cldice_closed(x, y, iterations=iterations, ignore_background=True, batch=True, smooth=1.0)
        theirs = soft_cldice_published(one_hot_no_class(y, 2, x.dtype), torch.softmax(x, 1), iterations, 1.0)
        assert abs(float(mine) - float(theirs)) <= 1e-12


def test_margin_construction_keeps_its_distance():
    x = margin_logits((2, 3, 17, 23), seed=0).float()
    p = torch.softmax(x.double(), 1)
    assert selection_margin(p[:, 1:], 3) >= 1e-5
    assert selection_margin(torch.softmax(torch.randn(2, 3, 17, 23, dtype=torch.float64), 1), 3) < 1e-4


def test_soft_skeletonize_argument_checks():
    L = _L()
    from advchain_amd._lib import AdvchainHipError
    x = torch.rand(1, 2, 5, 6)
    for bad in ([[1.0]], torch.rand(5, 6), torch.rand(1, 5, 6), torch.rand(1, 1, 2, 2, 2, 2)):
        with pytest.raises(ValueError):
            L.soft_skeletonize(bad)
    for it in (-1, 33, 1.5, True, None, "3"):
        with pytest.raises(ValueError):
            L.soft_skeletonize(x, iterations=it)
    for dt in (torch.float64, torch.float16, torch.bfloat16, torch.int64):
        with pytest.raises(ValueError):
            L.soft_skeletonize(x.to(dt))
    with pytest.raises(NotImplementedError):
        L.soft_skeletonize(torch.empty(1, L.MAX_CLASSES + 1, 1, 1))
    with pytest.raises(AdvchainHipError):
        L.soft_skeletonize(x)
    with pytest.raises(AdvchainHipError):
        L.soft_skeletonize(x, iterations=0)


def test_cldice_loss_argument_checks():
    L = _L()
    from advchain_amd._lib import AdvchainHipError
    x = torch.randn(2, 3, 5, 6)
    y = torch.randint(0, 3, (2, 5, 6))
    t = torch.softmax(torch.randn(2, 3, 5, 6), 1)
    for bad in ([[1.0]], torch.rand(5, 6), torch.rand(2, 5, 6)):
        with pytest.raises(ValueError):
            L.cldice_loss(bad, y)
    for it in (-1, 33, 2.0, False, None):
        with pytest.raises(ValueError):
            L.cldice_loss(x, y, iterations=it)
    with pytest.raises(ValueError):
        L.cldice_loss(x.half(), y)
    with pytest.raises(ValueError):
        L.cldice_loss(x, t.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        L.cldice_loss(x, y[:, :4])
    with pytest.raises(ValueError):
        L.cldice_loss(x, t[:, :2])
    with pytest.raises(NotImplementedError):
        L.cldice_loss(x, y[0])
    for smooth in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            L.cldice_loss(x, y, smooth=smooth)
    with pytest.raises(ValueError):
        L.cldice_loss(x[:, :1], y, ignore_background=True)
    with pytest.raises(ValueError):
        L.cldice_loss(x, y, weight=[1.0, 2.0])
    with pytest.raises(ValueError):
        L.cldice_loss(x, y, weight=torch.ones(4))
    with pytest.raises(ValueError):
        L.cldice_loss(x, y, weight=1.0)
    with pytest.raises(NotImplementedError):
        L.cldice_loss(torch.empty(1, L.MAX_CLASSES + 1, 1, 1), torch.zeros(1, 1, 1, dtype=torch.int64))
    for tgt in (y, t):
        with pytest.raises(AdvchainHipError):
            L.cldice_loss(x, tgt)
    with pytest.raises(AdvchainHipError):
        L.cldice_loss(x.bfloat16(), y, iterations=0, weight=[1.0, 0.0, 2.0], ignore_background=False, batch=True, smooth=0.0)


def test_switch_point_is_exported():
    from advchain_amd import ops
    assert 0 <= ops.SKELETON_FUSED_MAX_ITERATIONS < ops.SKELETON_MAX_ITERATIONS == 32
