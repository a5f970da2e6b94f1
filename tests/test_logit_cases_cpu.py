"""What the regimes of tests/logit_cases.py promise, checked on their own -- conditions on the inputs, no kernel involved -- and
the float64 consistency form of tests/consistency_forms.py against the CPU oracle where the oracle can run (fp32)."""
import math

import pytest
import torch

from tests import logit_cases as C
from tests.consistency_forms import consistency_closed
from tests.dice_forms import ce_closed_nd, dice_closed

SHAPES = tuple(sorted(set(C.SUPERVISED + C.CONSISTENCY)))
IDS = ["%s-K%d" % ("x".join(map(str, d)), K) for d, K in SHAPES]


def _voxels(dims):
    return math.prod(dims)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dims,K", SHAPES, ids=IDS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_generators_are_deterministic_and_typed(regime, dims, K, bf16):
    x, y = C.logits(regime, C.N, K, dims, seed=1, bf16=bf16)
    x2, y2 = C.logits(regime, C.N, K, dims, seed=1, bf16=bf16)
    assert x.dtype == torch.float32 and y.dtype == torch.int64
    assert tuple(x.shape) == (C.N, K) + dims and tuple(y.shape) == (C.N,) + dims
    assert torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(x2, nan=12345.0)) and torch.equal(y, y2)
    assert int(y.min()) >= 0 and int(y.max()) < K
    other, _ = C.logits(regime, C.N, K, dims, seed=2, bf16=bf16)
    assert not torch.equal(torch.nan_to_num(other, nan=12345.0), torch.nan_to_num(x, nan=12345.0))
    if bf16:
        assert torch.equal(torch.nan_to_num(x.bfloat16().float(), nan=12345.0), torch.nan_to_num(x, nan=12345.0))
    if regime in C.FINITE:
        assert bool(torch.isfinite(x).all())


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dims,K", SHAPES, ids=IDS)
@pytest.mark.parametrize("regime", [r for r in C.REGIMES if r != "poison"])
def test_float64_cross_entropy_and_dice_are_finite(regime, dims, K, bf16):
    """Every regime but `poison` has a finite float64 cross entropy (labels) and Dice loss with finite gradients: what the
    kernels are held to exists."""
    x, y = C.logits(regime, C.N, K, dims, seed=1, bf16=bf16)
    for closed in (ce_closed_nd, dice_closed):
        x64 = x.double().requires_grad_(True)
        v = closed(x64, y)
        (g,) = torch.autograd.grad(v, x64)
        assert bool(torch.isfinite(v)) and bool(torch.isfinite(g).all()), (regime, closed.__name__)
        if regime == "masked":
            assert float(g[torch.isinf(x)].abs().max()) == 0.0


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dims,K", SHAPES, ids=IDS)
def test_saturated_holds_exact_ones_and_zeros_and_wrong_labels(dims, K, bf16):
    x, y = C.logits("saturated", C.N, K, dims, seed=1, bf16=bf16)
    p = torch.softmax(x, 1)
    assert p.dtype == torch.float32
    assert bool((p == 1.0).any()) and bool((p == 0.0).any())
    wrong = float((y != x.argmax(1)).float().mean())
    assert wrong >= 0.1, wrong


@pytest.mark.parametrize("dims,K", SHAPES, ids=IDS)
def test_masked_holds_every_pattern_and_no_empty_voxel(dims, K):
    """Each pattern on at least 16 voxels of every entry; where an entry has fewer than 96 voxels, on at least V // 8 of them and
    on one at least (the 7-voxel rows of the run-time-K cases hold each pattern once or twice)."""
    x, y = C.logits("masked", C.N, K, dims, seed=1)
    V = _voxels(dims)
    inf = torch.isinf(x.reshape(C.N, K, V))
    assert bool((x[torch.isinf(x)] < 0).all())
    assert int(inf.all(1).sum()) == 0                                   # no voxel with every class masked
    pat = C.masked_pattern(V)
    need = 16 if V >= 96 else max(V // 8, 1)
    for p in range(4):
        want = torch.zeros(K, dtype=torch.bool)
        want[C.masked_classes(p, K)] = True
        hit = (inf == want[None, :, None]).all(1) & (pat == p)[None]
        assert int(hit.sum(1).min()) >= need, (p, hit.sum(1).tolist(), need)
        assert bool(hit[:, pat == p].all())
    assert not bool(inf[:, :, pat == -1].any()) and int((pat == -1).sum()) >= (4 if V >= 16 else 0)
    assert bool(torch.isfinite(x.gather(1, y[:, None])).all())          # no label on a masked class


@pytest.mark.parametrize("dims,K", SHAPES, ids=IDS)
def test_mixed_holds_equal_and_vanishing_probabilities(dims, K):
    x, _ = C.logits("mixed", C.N, K, dims, seed=1)
    p = torch.softmax(x, 1)
    spread = (p.max(1).values - p.min(1).values) / p.max(1).values
    assert bool((spread <= 2.0 ** -23).any())                           # all classes equal to one fp32 ulp
    assert bool((p.min(1).values < 1e-30).any())


@pytest.mark.parametrize("dims,K", SHAPES, ids=IDS)
def test_huge_and_poison_sit_where_the_table_says(dims, K):
    V = _voxels(dims)
    x, y = C.logits("huge", C.N, K, dims, seed=1)
    x, y = x.reshape(C.N, K, V), y.reshape(C.N, V)
    vox = C.huge_voxels(V)
    assert len(set(vox)) == min(8, V)
    big = float(torch.tensor(C.HUGE, dtype=torch.float32))
    for v in vox:
        assert float(x[0, :, v].max()) == big and float(x[0, y[0, v], v]) == big
        assert K == 1 or float(x[0, :, v].min()) == -big
    assert float(x[1].abs().max()) < 100
    x, _ = C.logits("poison", C.N, K, dims, seed=1)
    x = x.reshape(C.N, K, V)
    nan_v, inf_v = C.poison_voxels(V)
    assert nan_v != inf_v
    bad = ~torch.isfinite(x)
    assert int(bad.sum()) == 2 and bool(torch.isnan(x[1, 0, nan_v])) and float(x[1, K - 1, inf_v]) == float("inf")


def test_offsets_shift_the_same_draw():
    for sign, regime in ((1.0, "offset+"), (-1.0, "offset-")):
        x, _ = C.logits(regime, C.N, 4, (11, 20), seed=3)
        assert abs(float(x.mean()) - sign * 1000.0) < 1.0 and 2.0 < float(x.std()) < 4.0


# ---- the float64 consistency form is the oracle's expression -----------------------------------------------------------------

MIXES = ((["kl"], [1.0]), (["kl", "contour"], [1.0, 0.5]), (["mse", "kl", "contour"], [0.7, 1.3, 0.5]), (["mse", "contour"], [1.0, 0.5]))


@pytest.mark.parametrize("dims,K", [((11, 20), 5), ((3, 5, 7), 2), ((1, 7), 17)])
def test_consistency_form_is_the_oracle_in_fp32(dims, K):
    """Value and both gradients in fp32 against the oracle (and, with class weights, against the weighted expression of
    tests/test_class_weights_cpu.py), within the fp32 contract of tests/test_ref_grad_gpu.py: 1e-7 + 2e-5 |v|, 2e-5 max|g| + 1e-10."""
    import torch.nn.functional as F
    from oracle import advchain_oracle as O
    from tests.test_class_weights_cpu import cycle_weights, weighted_loss
    pred, _ = C.logits("base", C.N, K, dims, seed=1)
    ref, _ = C.logits("base", C.N, K, dims, seed=2)
    mk = C.binary_mask(C.N, K, dims)
    onehot = F.one_hot(ref.argmax(1), K).movedim(-1, 1).float().contiguous()
    for types, weights in MIXES:
        for r, mask, is_gt in ((ref, None, False), (ref, mk[:, :1].contiguous(), False), (ref, mk, False),
                               (onehot, mk[:, :1].contiguous(), True)):
            for cw in (None, cycle_weights(K)):
                a, b = pred.clone().requires_grad_(True), r.clone().requires_grad_(True)
                got = consistency_closed(a, b, types, weights, mask, is_gt, cw)
                ga, gb = torch.autograd.grad(got, (a, b), allow_unused=True)
                c, d = pred.clone().requires_grad_(True), r.clone().requires_grad_(True)
                want = O.consistency_loss(c, d, types, weights, mask=mask, is_gt=is_gt) if cw is None else \
                    weighted_loss(c, d, types, weights, cw, mask=mask, is_gt=is_gt)
                gc, gd = torch.autograd.grad(want, (c, d), allow_unused=True)
                tag = (dims, K, tuple(types), mask is not None and mask.shape[1], is_gt, cw is not None)
                got, want = float(got.detach()), float(want.detach())
                assert abs(got - want) < 1e-7 + 2e-5 * abs(want), tag
                for g, w in ((ga, gc), (gb, gd)):
                    g = torch.zeros_like(pred) if g is None else g
                    w = torch.zeros_like(pred) if w is None else w
                    assert float((g - w).abs().max()) < 2e-5 * float(w.abs().max()) + 1e-10, tag
