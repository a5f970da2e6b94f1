"""Class weights in the consistency loss, as far as a machine without a GPU can check them.

The reference documents `class_weights` and raises (advchain/common/loss.py:18,27-28), so this file DEFINES what the weighted
loss is -- `weighted_loss`, a torch expression written from the reference's formulas (loss.py:55-79,102-220,223-249) with w_k
inserted -- and proves that expression against the oracle: with w = 1 it is the oracle's loss in value and in both gradients,
and it is linear in w.  tests/test_class_weights_gpu.py holds the kernels to it.

    'mse'      sum_{n,k,v} w_k (m_k P_k - m_k T_k)^2 / (N K V) / (numel(mask) / K)
    'kl'       mean over (n, v) of  sum_k w_k m_k T'_k (log T'_k - log P_k)
    'contour'  sum_{i >= 1} w_i contour_term(P_i, T_i, mask) / (K - 1)          (w_0 does not enter)

Then the argument checks: a wrong length, a negative entry, a NaN and an infinite entry are ValueErrors with CPU tensors --
raised before anything asks for a device -- and valid weights reach the kernels' gate (AdvchainHipError: no CPU path)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_ref_grad_gpu import MIXES, MODES, _operands

CYCLE = (0.25, 2.0, 0.0, 1.5, 0.5)     # a background weight != 1, a class that must contribute nothing, a spread of 8


def cycle_weights(K):
    return tuple(CYCLE[k % len(CYCLE)] for k in range(K))


def weighted_loss(output, reference, types, weights, class_weights, mask=None, is_gt=False):
    """oracle.advchain_oracle.consistency_loss with the class weights inserted (scales = [0])."""
    from oracle import advchain_oracle as O
    K = reference.size(1)
    if mask is None:
        mask = torch.ones_like(output).float()
    w = torch.as_tensor(class_weights, dtype=torch.float32).reshape((1, K) + (1,) * (output.dim() - 2))
    dist = 0.
    for kind, weight in zip(types, weights):
        if kind == "kl":
            if not is_gt:
                p = F.softmax(reference, dim=1)
                log_p = F.log_softmax(reference, dim=1)
            else:
                p = torch.where(reference == 0, 1e-8, 1 - 1e-8)
                log_p = torch.log(p)
            plogp = torch.sum(w * (mask * (p * log_p)), dim=1)
            plogq = torch.sum(w * (mask * (p * F.log_softmax(output, dim=1))), dim=1)
            loss = torch.mean(plogp - plogq)
        elif kind == "mse":
            tgt = reference if is_gt else torch.softmax(reference, dim=1)
            inp = torch.softmax(output, dim=1)
            loss = torch.mean(w * (inp * mask - tgt * mask) ** 2) / (torch.numel(mask) / K)
        elif kind == "contour":
            tgt = reference if is_gt else torch.softmax(reference, dim=1)
            inp = torch.softmax(output, dim=1)
            loss = 0.
            for i in range(1, K):
                loss = loss + float(class_weights[i]) * O._contour_term(inp[:, [i]], tgt[:, [i]], mask)
            if K > 1:
                loss = loss / (K - 1)
        else:
            raise NotImplementedError(kind)
        dist = dist + weight * loss
    return dist / 1.0


def want(pred, r, types, weights, class_weights, mask, is_gt):
    """(value, prediction.grad, reference.grad or None) of `weighted_loss` in fp32 on the CPU, on the upcast operands."""
    a, b = pred.detach().float().clone().requires_grad_(True), r.detach().float().clone().requires_grad_(True)
    v = weighted_loss(a, b, types, weights, class_weights, mask=mask, is_gt=is_gt)
    v.backward()
    return float(v.detach()), a.grad, b.grad


def case(mode, K, dims):
    """(prediction, reference, mask, is_gt) of one mask mode of tests/test_ref_grad_gpu.py, N = 2, fp32 on the CPU."""
    pred, ref, mk, onehot, soft = _operands(K, dims)
    one = mk[:, :1].contiguous()
    return {"none": (pred, ref, None, False), "one": (pred, ref, one, False), "perclass": (pred, ref, mk, False),
            "one_gt": (pred, onehot, one, True), "soft_gt": (pred, soft, one, True)}[mode]


def _fp32_close(got, ref, tag):
    """The project's fp32 contract: elementwise 2e-5 max|g| + 1e-10; None counts as zeros."""
    if got is None or ref is None:
        assert (got is None or float(got.abs().max()) == 0.0) and (ref is None or float(ref.abs().max()) == 0.0), tag
        return
    assert float((got - ref).abs().max()) < 2e-5 * float(ref.abs().max()) + 1e-10, tag


# ---- the expression itself -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mix", range(len(MIXES)))
@pytest.mark.parametrize("dims", [(11, 20), (3, 5, 7)])
@pytest.mark.parametrize("K", [1, 4, 20])
def test_weight_one_is_the_oracle(K, dims, mix):
    from oracle import advchain_oracle as O
    types, weights = MIXES[mix]
    for mode in MODES:
        pred, r, mask, is_gt = case(mode, K, dims)
        v, gp, gr = want(pred, r, types, weights, (1.0,) * K, mask, is_gt)
        a, b = pred.clone().requires_grad_(True), r.clone().requires_grad_(True)
        ov = O.consistency_loss(a, b, types, weights, mask=mask, is_gt=is_gt)
        ov.backward()
        tag = (K, dims, tuple(types), mode)
        ov = float(ov.detach())
        assert abs(v - ov) < 1e-7 + 2e-5 * abs(ov), tag
        _fp32_close(gp, a.grad, tag + ("prediction.grad",))
        _fp32_close(gr, b.grad, tag + ("reference.grad",))


@pytest.mark.parametrize("dims", [(11, 20), (3, 5, 7)])
@pytest.mark.parametrize("K", [4, 20])
def test_linear_in_the_weights(K, dims):
    """L(a w1 + b w2) = a L(w1) + b L(w2), value and both gradients (a, b powers of two: the combination itself is exact)."""
    types, weights = MIXES[2]
    w1 = cycle_weights(K)
    w2 = tuple(float(x) for x in torch.rand(K, generator=torch.Generator().manual_seed(5)).mul(4).round().div(4))
    a, b = 0.5, 2.0
    for mode in MODES:
        pred, r, mask, is_gt = case(mode, K, dims)
        l1 = want(pred, r, types, weights, w1, mask, is_gt)
        l2 = want(pred, r, types, weights, w2, mask, is_gt)
        l12 = want(pred, r, types, weights, tuple(a * x + b * y for x, y in zip(w1, w2)), mask, is_gt)
        comb = a * l1[0] + b * l2[0]
        assert abs(l12[0] - comb) < 1e-7 + 2e-5 * abs(comb), (K, dims, mode)
        for i in (1, 2):
            _fp32_close(l12[i], a * l1[i] + b * l2[i], (K, dims, mode, i))


def test_a_zero_weight_class_contributes_nothing_and_contour_ignores_the_background():
    K, dims = 5, (11, 20)
    pred, r, mask, is_gt = case("perclass", K, dims)
    w = cycle_weights(K)                                   # w_2 = 0
    m2 = mask.clone()
    m2[:, 2] = 1 - m2[:, 2]                                # (the mask of class 2 may change freely: 'mse' and 'kl' read it per class)
    assert want(pred, r, ["mse", "kl"], [0.7, 1.3], w, m2, is_gt)[0] == want(pred, r, ["mse", "kl"], [0.7, 1.3], w, mask, is_gt)[0]
    for w0 in (0.0, 3.0):
        assert want(pred, r, ["contour"], [1.0], (w0,) + w[1:], mask, is_gt)[0] == want(pred, r, ["contour"], [1.0], w, mask, is_gt)[0]


# ---- the argument checks ---------------------------------------------------------------------------------------------------

BAD = {"a wrong length": ([1.0, 2.0, 1.0], "length"), "a negative entry": ([1.0, -0.5, 1.0, 1.0], "negative"),
       "a NaN": ([1.0, float("nan"), 1.0, 1.0], "NaN"), "an infinite entry": ([1.0, 1.0, float("inf"), 1.0], "infinite")}


@pytest.mark.parametrize("what", sorted(BAD))
@pytest.mark.parametrize("kind", ["list", "tuple", "ndarray", "tensor"])
def test_bad_weights_are_value_errors_on_cpu_tensors(what, kind):
    from advchain_amd.common.loss import calc_segmentation_consistency, kl_divergence
    vals, word = BAD[what]
    w = {"list": list, "tuple": tuple, "ndarray": np.array, "tensor": torch.tensor}[kind](vals)
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError, match=word):
        calc_segmentation_consistency(x, x, ["mse", "contour"], [1.0, 0.5], class_weights=w)
    with pytest.raises(ValueError, match=word):
        kl_divergence(x, x, class_weights=w)
    with pytest.raises(ValueError, match=word):
        calc_segmentation_consistency(x.bfloat16(), x, ["kl"], [1.0], class_weights=w, scales=[0, 1])


@pytest.mark.parametrize("kind", ["list", "tuple", "ndarray", "tensor"])
def test_valid_weights_on_cpu_tensors_reach_the_gate(kind):
    """Not NotImplementedError any more: the operator's own refusal of CPU tensors."""
    from advchain_amd import _lib
    from advchain_amd.common.loss import calc_segmentation_consistency, kl_divergence
    w = {"list": list, "tuple": tuple, "ndarray": np.array, "tensor": torch.tensor}[kind]([0.25, 2.0, 0.0, 1.5])
    x = torch.zeros(1, 4, 8, 8)
    for a, b in ((x, x), (x.bfloat16(), x)):
        with pytest.raises(_lib.AdvchainHipError, match="no CPU path"):
            calc_segmentation_consistency(a, b, ["mse", "contour"], [1.0, 0.5], class_weights=w)
        with pytest.raises(_lib.AdvchainHipError, match="no CPU path"):
            kl_divergence(b, a, class_weights=w)


def test_the_solver_keeps_the_weights_as_a_plain_tuple_in_its_graph_key():
    from advchain_amd.augmentor import ComposeAdversarialTransformSolver
    solver = ComposeAdversarialTransformSolver(chain_of_transforms=[], class_weights=np.array([0.25, 2.0, 0.0, 1.5]))
    assert solver.class_weights == (0.25, 2.0, 0.0, 1.5)
    assert ("_class_weights", (0.25, 2.0, 0.0, 1.5)) in solver._plain_attrs(solver)
    solver.class_weights = torch.tensor([1.0, 1.0, 3.0, 1.0])
    assert ("_class_weights", (1.0, 1.0, 3.0, 1.0)) in solver._plain_attrs(solver)
    solver.class_weights = None
    assert solver.class_weights is None and ComposeAdversarialTransformSolver(chain_of_transforms=[]).class_weights is None
    with pytest.raises(ValueError, match="negative"):
        solver.class_weights = [1.0, -1.0]


def test_cw_entries_check_their_arguments_on_the_host():
    """The lp entries' checks plus class_w: a negative code and a message that names the entry; nothing is launched."""
    from advchain_amd import _lib
    lib = _lib.load()
    dims = _lib.dims_array((4, 8))
    buf = (ctypes.c_float * 4096)()          # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(pred=p, ref=p, stats=p, out=p, K=20, pb=0, rb=0, mask=None, mch=1, nd=2, N=1, w=p):
        return lib.advchain_consistency_cw_fwd(pred, pb, ref, rb, mask, stats, None, out, N, K, nd, dims, mch, 0, 1, 0, w, None)

    def bwd(pred=p, ref=p, stats=p, out=p, K=20, pb=0, rb=0, mask=None, mch=1, nd=2, N=1, w=p):
        return lib.advchain_consistency_cw_bwd(pred, pb, ref, rb, stats, None, mask, None, out, 1.0, 0.0, 0.0, 0.0, 0, N, K, nd,
                                               dims, mch, w, None)

    def ref_bwd(pred=p, ref=p, stats=p, out=p, K=20, pb=0, rb=0, mask=None, mch=1, nd=2, N=1, w=p):
        return lib.advchain_consistency_cw_ref_bwd(pred, pb, ref, rb, stats, None, mask, None, out, 1.0, 0.0, 0.0, 0.0, 0, N, K,
                                                   nd, dims, mch, w, None)
    for call, name in ((fwd, b"consistency_cw_fwd"), (bwd, b"consistency_cw_bwd"), (ref_bwd, b"consistency_cw_ref_bwd")):
        for kw in (dict(w=None), dict(pred=None), dict(ref=None), dict(stats=None), dict(out=None), dict(K=0), dict(K=65536),
                   dict(pb=2), dict(rb=-1), dict(mask=p, mch=3), dict(nd=4), dict(N=65536)):
            assert call(**kw) < 0, (name, kw)
            assert name in lib.advchain_last_error(), (name, kw, lib.advchain_last_error())
        for pb in (0, 1):
            for rb in (0, 1):
                assert call(N=0, pb=pb, rb=rb) == 0, (name, pb, rb)       # an empty batch is fine and launches nothing
