"""The gradient of the consistency loss with respect to the REFERENCE (csrc/loss_ref.hip: advchain_consistency_ref_bwd, one
launch whichever forward family ran) against the CPU oracle's autograd with both operands requiring grad.

Operands and mask modes are those of tests/test_wide_loss_gpu.py plus `soft_gt` (a soft is_gt=True target that requires grad).
Tolerance, as there: gradient 2e-5 of its maximum + 1e-10, value 1e-7 + 2e-5 |v|, against the oracle in fp32 (whose own
fp32-against-float64 spread of the reference-side gradient is 6.5e-7 of its maximum: a factor of 30 is left to the kernels).
An oracle gradient of None (is_gt with 'kl' alone: the reference's where() cuts the graph) counts as zeros."""
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

MIXES = ((["kl"], [1.0]), (["kl", "contour"], [1.0, 0.5]), (["mse", "kl", "contour"], [0.7, 1.3, 0.5]),
         (["mse", "contour"], [1.0, 0.5]))
FULL = MIXES[2]
MODES = ("none", "one", "perclass", "one_gt", "soft_gt")

# fused and declined rows, whole and partial tiles, single-row volumes; every forward family (fused K = 2..4, three-kernel
# K = 5..16 and what the fused form declines, run-time K from 17 on)
PARITY = ([(d, K) for K in (2, 3, 4) for d in ((12, 64), (37, 52), (1, 7), (64, 256), (5, 6, 64), (3, 5, 7), (1, 1, 5))]
          + [((37, 52), 5), ((7, 9, 80), 5)]
          + [(d, K) for K in (8, 16) for d in ((11, 20), (3, 5, 7))]
          + [(d, K) for K in (17, 20, 33, 105) for d in ((11, 20), (1, 7), (2, 3, 8))]
          + [((19, 40, 128), 20)])


@functools.lru_cache(maxsize=4)
def _operands(K, dims, N=2):
    pred = rand((N, K) + dims, 311) * 3
    ref = rand((N, K) + dims, 312) * 3
    mk = (rand((N, K) + dims, 313) > -0.6).float()
    onehot = F.one_hot(ref.argmax(1), K).movedim(-1, 1).float().contiguous()
    soft = torch.softmax(rand((N, K) + dims, 314) * 2, 1)
    return pred, ref, mk, onehot, soft


def _case(mode, K, dims):
    """(prediction, reference, mask, is_gt) of one mask mode."""
    pred, ref, mk, onehot, soft = _operands(K, dims)
    one = mk[:, :1].contiguous()
    return {"none": (pred, ref, None, False), "one": (pred, ref, one, False), "perclass": (pred, ref, mk, False),
            "one_gt": (pred, onehot, one, True), "soft_gt": (pred, soft, one, True)}[mode]


def _zeros_if_none(g, like):
    return torch.zeros_like(like) if g is None else g


def _oracle(pred, r, types, weights, mask, is_gt):
    """(value, prediction.grad, reference.grad) of the oracle in fp32 with BOTH operands requiring grad."""
    from oracle import advchain_oracle as O
    a, b = pred.clone().requires_grad_(True), r.clone().requires_grad_(True)
    v = O.consistency_loss(a, b, types, weights, mask=mask, is_gt=is_gt)
    v.backward()
    return float(v.detach()), a.grad, _zeros_if_none(b.grad, b)


def _product(pred, r, types, weights, mask, is_gt, scale=1.0, pred_grad=True, ref_grad=True, raw=False):
    from advchain_amd.common.loss import calc_segmentation_consistency
    a = pred.to(DEV).requires_grad_(pred_grad)
    b = r.to(DEV).requires_grad_(ref_grad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")            # no UserWarning for a reference that requires grad
        v = calc_segmentation_consistency(a, b, types, weights, scales=[0], mask=None if mask is None else mask.to(DEV),
                                          is_gt=is_gt)
    (scale * v).backward()
    if raw:
        return v.detach(), a.grad, b.grad
    return (float(v.detach()), None if a.grad is None else a.grad.cpu(), _zeros_if_none(b.grad, b).cpu())


def _close(got, want, tag):
    err, top = maxdiff(got, want), float(want.abs().max())
    print("%s: err %.3e (max %.3e, bound %.3e)" % (tag, err, top, 2e-5 * top + 1e-10))
    assert err < 2e-5 * top + 1e-10, tag


def _check(got, want, tag):
    assert abs(got[0] - want[0]) < 1e-7 + 2e-5 * abs(want[0]), tag + ("value",)
    _close(got[1], want[1], tag + ("prediction.grad",))
    _close(got[2], want[2], tag + ("reference.grad",))


@pytest.mark.parametrize("mix", range(len(MIXES)))
@pytest.mark.parametrize("dims,K", PARITY)
def test_reference_grad_matches_the_oracle(dims, K, mix):
    types, weights = MIXES[mix]
    for mode in MODES:
        pred, r, mask, is_gt = _case(mode, K, dims)
        _check(_product(pred, r, types, weights, mask, is_gt), _oracle(pred, r, types, weights, mask, is_gt),
               (dims, K, tuple(types), mode))


@pytest.mark.parametrize("mix", range(len(MIXES)))
@pytest.mark.parametrize("dims", [(12, 64), (37, 52), (5, 6, 64), (3, 5, 7)])
@pytest.mark.parametrize("K", [2, 4])
def test_register_and_run_time_forms_agree(K, dims, mix):
    """ops.REF_GRAD_REG_MAX_K = 0 routes K <= 4 through the run-time-K form: against the oracle and the register form."""
    from advchain_amd import ops
    types, weights = MIXES[mix]
    for mode in MODES:
        pred, r, mask, is_gt = _case(mode, K, dims)
        want = _oracle(pred, r, types, weights, mask, is_gt)
        reg = _product(pred, r, types, weights, mask, is_gt)
        assert ops.REF_GRAD_REG_MAX_K == 4
        ops.REF_GRAD_REG_MAX_K = 0
        try:
            run = _product(pred, r, types, weights, mask, is_gt)
        finally:
            ops.REF_GRAD_REG_MAX_K = 4
        tag = (dims, K, tuple(types), mode)
        _check(reg, want, tag + ("register",))
        _check(run, want, tag + ("run-time",))
        _close(run[2], reg[2], tag + ("run-time vs register",))
        assert torch.equal(run[1], reg[1])          # (the prediction side does not know the knob)


@pytest.mark.parametrize("dims", [(37, 52), (5, 6, 64)])
@pytest.mark.parametrize("K", [4, 8, 20])
def test_value_and_prediction_grad_do_not_move(K, dims):
    """A reference that requires grad changes neither the value nor prediction.grad by a bit (same kernels, same launches).
    (The value's partial sums meet in 64 float-atomic slots, slot = (workgroup + 7 n) mod 64: at these sizes -- fewer than 64
    workgroups per batch entry, N = 2 -- a slot receives at most two, and a sum of two does not depend on their order.)"""
    for mode in ("one", "perclass", "soft_gt"):
        pred, r, mask, is_gt = _case(mode, K, dims)
        both = _product(pred, r, *FULL, mask, is_gt, raw=True)
        only = _product(pred, r, *FULL, mask, is_gt, ref_grad=False, raw=True)
        assert only[2] is None and both[2] is not None
        assert torch.equal(both[1], only[1]), (K, dims, mode)
        assert torch.equal(both[0], only[0]), (K, dims, mode)


_PRED_SIDE = ("k_consistency_bwd", "k_loss_fused_bwd", "k_lp_bwd")


@pytest.mark.parametrize("dims", [(37, 52), (5, 6, 64)])
@pytest.mark.parametrize("K", [4, 8, 20])
def test_reference_only(K, dims):
    """With a detached prediction: the same bits in reference.grad, and no prediction-side backward kernel is launched."""
    from torch.profiler import ProfilerActivity, profile
    from advchain_amd import _lib
    pred, r, mask, is_gt = _case("one", K, dims)
    both = _product(pred, r, *FULL, mask, is_gt, raw=True)
    lib = _lib.load()
    torch.cuda.synchronize()
    with lib.timed() as timed:
        del timed.records[:]
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            only = _product(pred, r, *FULL, mask, is_gt, pred_grad=False, raw=True)
            torch.cuda.synchronize()
        entries = [rec[0] for rec in timed.records]
        del timed.records[:]
    assert only[1] is None
    assert torch.equal(only[2], both[2])
    assert "advchain_consistency_ref_bwd" in entries, entries
    assert not [e for e in entries if e.endswith("_bwd") and e != "advchain_consistency_ref_bwd"], entries
    kernels = [e.name for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower()]
    print(sorted(set(kernels)))
    assert any("k_loss_ref_grad" in k for k in kernels), kernels
    assert not [k for k in kernels if any(p in k for p in _PRED_SIDE)], kernels


@pytest.mark.parametrize("dims", [(37, 52), (5, 6, 64)])
@pytest.mark.parametrize("K", [4, 20])
def test_mse_is_antisymmetric_in_its_operands(K, dims):
    """'mse' alone, no mask: (P - T)^2 is symmetric, so grad_ref(pred=a, ref=b) is grad_pred(pred=b, ref=a) of the proven
    prediction-side kernels."""
    a, b, _, _, _ = _operands(K, dims)
    types, weights = ["mse"], [1.0]
    ref_side = _product(a, b, types, weights, None, False)[2]
    pred_side = _product(b, a, types, weights, None, False, ref_grad=False)[1]
    _close(ref_side, pred_side, (K, dims, "mse symmetry"))


@pytest.mark.parametrize("K", [4, 8, 20])
def test_bit_reproducible_and_grad_scale(K):
    dims = (37, 52)
    for mode in ("perclass", "soft_gt"):
        pred, r, mask, is_gt = _case(mode, K, dims)
        one = _product(pred, r, *FULL, mask, is_gt)
        two = _product(pred, r, *FULL, mask, is_gt)
        assert torch.equal(one[2], two[2]) and torch.equal(one[1], two[1])
        scaled = _product(pred, r, *FULL, mask, is_gt, scale=0.37)
        want = _oracle(pred, r, *FULL, mask, is_gt)
        _close(scaled[2] / 0.37, want[2], (K, mode, "0.37 * v"))
        _close(scaled[1] / 0.37, want[1], (K, mode, "0.37 * v, prediction"))


@pytest.mark.parametrize("K", [4, 8, 20])
def test_kl_with_a_ground_truth_reference_has_no_gradient(K):
    pred, r, mask, is_gt = _case("soft_gt", K, (11, 20))
    v, gp, gr = _product(pred, r, ["kl"], [1.0], mask, is_gt, raw=True)
    assert gr is None and gp is not None
    want = _oracle(pred, r, ["kl"], [1.0], mask, is_gt)
    _close(gp.cpu(), want[1], (K, "kl is_gt"))
    assert float(want[2].abs().max()) == 0.0


@pytest.mark.parametrize("K", [4, 8, 20])
def test_non_contiguous_reference(K):
    """A permuted view as the reference: its gradient has the view's shape and the values of the contiguous case."""
    from advchain_amd.common.loss import calc_segmentation_consistency
    dims = (11, 20)
    pred, r, mask, is_gt = _case("one", K, dims)
    want = _oracle(pred, r, *FULL, mask, is_gt)
    base = r.permute(0, 1, 3, 2).contiguous().to(DEV).requires_grad_(True)       # (N, K, W, H) leaf
    view = base.permute(0, 1, 3, 2)
    assert not view.is_contiguous() and view.shape == r.shape
    a = pred.to(DEV).requires_grad_(True)
    calc_segmentation_consistency(a, view, *FULL, scales=[0], mask=mask.to(DEV), is_gt=is_gt).backward()
    assert base.grad.shape == base.shape
    _close(base.grad.permute(0, 1, 3, 2).cpu(), want[2], (K, "permuted reference"))
    _close(a.grad.cpu(), want[1], (K, "permuted reference, prediction"))


@pytest.mark.parametrize("K", [4, 20])
def test_kl_divergence_fills_both_gradients(K):
    from oracle import advchain_oracle as O
    from advchain_amd.common.loss import kl_divergence
    pred, r, mask, _ = _case("one", K, (11, 20))
    a, b = pred.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v = kl_divergence(b, a, mask=mask.to(DEV))
    v.backward()
    oa, ob = pred.clone().requires_grad_(True), r.clone().requires_grad_(True)
    ov = O.consistency_loss(oa, ob, ["kl"], [1.0], mask=mask)
    ov.backward()
    _check((float(v.detach()), a.grad.cpu(), b.grad.cpu()), (float(ov.detach()), oa.grad, ob.grad), (K, "kl_divergence"))


@pytest.mark.parametrize("dims,K", [((12, 64), 4), ((6, 8, 64), 4), ((12, 20), 20)])
def test_two_scales(dims, K):
    """scales=[0, 1]: the pooling is torch autograd around the operator; against the oracle evaluated per scale on
    torch-pooled operands, sum_s 2^s loss_s / 2."""
    from oracle import advchain_oracle as O
    from advchain_amd.common.loss import calc_segmentation_consistency
    pred, r, _, _, _ = _operands(K, dims)
    types, weights = FULL
    a, b = pred.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    v = calc_segmentation_consistency(a, b, types, weights, scales=[0, 1])
    v.backward()
    oa, ob = pred.clone().requires_grad_(True), r.clone().requires_grad_(True)
    pool = torch.nn.AvgPool2d(2) if len(dims) == 2 else torch.nn.AvgPool3d(2)
    ov = (O.consistency_loss(oa, ob, types, weights) + 2.0 * O.consistency_loss(pool(oa), pool(ob), types, weights)) / 2.0
    ov.backward()
    _check((float(v.detach()), a.grad.cpu(), b.grad.cpu()), (float(ov.detach()), oa.grad, ob.grad), (dims, K, "scales 0, 1"))
