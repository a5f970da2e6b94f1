"""Class weights in the consistency loss, kl_divergence and the solver (the cw entries of csrc/loss_lp.hip:
advchain_consistency_cw_fwd / cw_bwd / cw_ref_bwd) against `weighted_loss` of tests/test_class_weights_cpu.py -- the
reference's formulas with w_k inserted, proved there against the oracle -- evaluated in fp32 on the CPU.

Operands and mask modes are those of tests/test_ref_grad_gpu.py at N = 2, built as tests/test_bf16_loss_gpu.py builds them: a
bf16 operand is rounded first and the want is computed on its exact upcast.  Weights cycle through (0.25, 2.0, 0.0, 1.5, 0.5)
over the classes: a background weight != 1 (which 'contour' must ignore), a class of weight 0, a spread of 8.

Tolerances, the project's own (tests/test_ref_grad_gpu.py, tests/test_bf16_loss_gpu.py): value 1e-7 + 2e-5 |v|; gradient of
an fp32 operand, elementwise, 2e-5 max|g| + 1e-10; gradient of a bf16 operand the same plus 2^-8 |g| (one rounding to 8
significant bits).  Nothing is added for the weights: they are exact binary fractions and enter as one more fp32 factor."""
import contextlib
import functools
import io
import warnings

import pytest
import torch

from tests.helpers import make_model, maxdiff, notebook_configs, seeded_init_param, smooth_data
from tests.test_class_weights_cpu import cycle_weights, want, weighted_loss
from tests.test_ref_grad_gpu import FULL, MIXES, MODES, _operands

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF16, FP32 = torch.bfloat16, torch.float32
PAIRS = {"bf16-bf16": (BF16, BF16), "fp32-bf16": (FP32, BF16), "bf16-fp32": (BF16, FP32), "fp32-fp32": (FP32, FP32)}

# (9, 70) crosses the 64-wide 2D tile, (5, 6, 40) the 32-wide 3D one; every shape meets at least two K, every K a 2D and a 3D shape
PARITY = [((1, 7), 1), ((1, 7), 4), ((1, 7), 17), ((11, 20), 2), ((11, 20), 5), ((11, 20), 20), ((9, 70), 4), ((9, 70), 16),
          ((1, 1, 5), 2), ((1, 1, 5), 16), ((3, 5, 7), 1), ((3, 5, 7), 5), ((3, 5, 7), 20), ((5, 6, 40), 4), ((5, 6, 40), 17)]


@functools.lru_cache(maxsize=8)
def _case(mode, K, dims, pair):
    """(prediction, reference, mask, is_gt) of one mask mode, each operand in the storage type of `pair` (CPU tensors)."""
    pred, ref, mk, onehot, soft = _operands(K, dims)
    one = mk[:, :1].contiguous()
    pt, rt = PAIRS[pair]
    p, r, m, is_gt = {"none": (pred, ref, None, False), "one": (pred, ref, one, False), "perclass": (pred, ref, mk, False),
                      "one_gt": (pred, onehot, one, True), "soft_gt": (pred, soft, one, True)}[mode]
    return p.to(pt), r.to(rt), m, is_gt


def _product(pred, r, types, weights, mask, is_gt, class_weights, pred_grad=True, ref_grad=True, scales=(0,)):
    """(value tensor, prediction.grad, reference.grad) of the product, device tensors as autograd left them."""
    from advchain_amd.common.loss import calc_segmentation_consistency
    a = pred.to(DEV).requires_grad_(pred_grad)
    b = r.to(DEV).requires_grad_(ref_grad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v = calc_segmentation_consistency(a, b, types, weights, class_weights=class_weights, scales=list(scales),
                                          mask=None if mask is None else mask.to(DEV), is_gt=is_gt)
    v.backward()
    return v.detach(), a.grad, b.grad


def _excess(got, ref, lowp):
    """max over the elements of |got - ref| / bound (<= 1 passes; the fp32 contract is strict)."""
    ref = ref.double()
    tol = (2.0 ** -8 * ref.abs() if lowp else 0.0) + 2e-5 * float(ref.abs().max()) + 1e-10
    return float(((got.double() - ref).abs() / tol).max())


def _close(got, ref, dtype, tag):
    assert got.dtype == dtype, tag
    lowp = dtype == BF16
    ex = _excess(got.float().cpu(), ref, lowp)
    print("%s: %.3f of the %s bound" % (tag, ex, "bf16" if lowp else "fp32"))
    assert (ex <= 1.0) if lowp else (ex < 1.0), tag


def _check(got, ref, pred, r, tag):
    v, gp, gr = got
    assert v.dtype == FP32 and v.dim() == 0, tag
    print("%s: value %.9g want %.9g: %.3f of the bound" % (tag, float(v), ref[0], abs(float(v) - ref[0]) / (1e-7 + 2e-5 * abs(ref[0]))))
    assert abs(float(v) - ref[0]) < 1e-7 + 2e-5 * abs(ref[0]), tag + ("value", float(v), ref[0])
    _close(gp, ref[1], pred.dtype, tag + ("prediction.grad",))
    if gr is None:
        assert ref[2] is None or float(ref[2].abs().max()) == 0.0, tag
    else:
        _close(gr, torch.zeros_like(r, dtype=FP32) if ref[2] is None else ref[2], r.dtype, tag + ("reference.grad",))


# ---- parity ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mix", range(len(MIXES)))
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims,K", PARITY)
def test_matches_the_weighted_expression(dims, K, pair, mix):
    types, weights = MIXES[mix]
    w = cycle_weights(K)
    for mode in MODES:
        pred, r, mask, is_gt = _case(mode, K, dims, pair)
        got = _product(pred, r, types, weights, mask, is_gt, w)
        # no reference gradient exactly where the unweighted path has none: is_gt with 'kl' alone (K = 1 has no contour term)
        cut = is_gt and "mse" not in types and not ("contour" in types and K > 1)
        assert (got[2] is None) == cut, (dims, K, pair, mode)
        _check(got, want(pred, r, types, weights, w, mask, is_gt), pred, r, (dims, K, pair, tuple(types), mode))


@pytest.mark.parametrize("kind", ["list", "ndarray", "cpu tensor", "device tensor"])
def test_every_kind_of_weights_gives_the_same_bits(kind):
    import numpy as np
    pred, r, mask, is_gt = _case("perclass", 5, (11, 20), "fp32-bf16")
    w = cycle_weights(5)
    given = {"list": list(w), "ndarray": np.array(w), "cpu tensor": torch.tensor(w), "device tensor": torch.tensor(w, device=DEV)}[kind]
    one, two = _product(pred, r, *FULL, mask, is_gt, w), _product(pred, r, *FULL, mask, is_gt, given)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])


# ---- weight one ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["bf16-bf16", "fp32-fp32"])
@pytest.mark.parametrize("dims", [(11, 20), (3, 5, 7)])
@pytest.mark.parametrize("K", [4, 20])
def test_weight_one_is_the_unweighted_loss(K, dims, pair):
    """Within the contract, not bitwise: at K <= 16 the unweighted fp32 side runs the register kernels of csrc/loss.hip."""
    for mode in MODES:
        pred, r, mask, is_gt = _case(mode, K, dims, pair)
        plain = _product(pred, r, *FULL, mask, is_gt, None)
        ones = _product(pred, r, *FULL, mask, is_gt, [1.0] * K)
        ref = (float(plain[0]), plain[1].float().cpu(), None if plain[2] is None else plain[2].float().cpu())
        assert (ones[2] is None) == (plain[2] is None)
        _check(ones, ref, pred, r, (dims, K, pair, mode, "w = 1"))


# ---- dispatch --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["bf16-bf16", "fp32-fp32"])
@pytest.mark.parametrize("dims,K", [((11, 20), 4), ((3, 5, 7), 20)])
def test_only_the_weighted_entries_that_are_needed_are_launched(dims, K, pair):
    from advchain_amd import _lib
    pred, r, mask, is_gt = _case("one", K, dims, pair)
    w = cycle_weights(K)
    lib = _lib.load()

    def entries(class_weights, **kw):
        with lib.timed() as timed:
            del timed.records[:]
            out = _product(pred, r, *FULL, mask, is_gt, class_weights, **kw)
            torch.cuda.synchronize()
            names = [rec[0] for rec in timed.records]
            del timed.records[:]
        return names, out

    both = _product(pred, r, *FULL, mask, is_gt, w)
    for kw, absent, present in ((dict(), None, "advchain_consistency_cw_ref_bwd"),
                                (dict(ref_grad=False), "advchain_consistency_cw_ref_bwd", "advchain_consistency_cw_bwd"),
                                (dict(pred_grad=False), "advchain_consistency_cw_bwd", "advchain_consistency_cw_ref_bwd")):
        names, only = entries(w, **kw)
        assert "advchain_consistency_cw_fwd" in names and present in names and absent not in names, names
        assert not [e for e in names if e.startswith("advchain_consistency") and "_cw_" not in e
                    and e != "advchain_consistency_finish"], names
        assert torch.equal(only[0], both[0])
        for i in (1, 2):
            assert only[i] is None or torch.equal(only[i], both[i])
    names, _ = entries(None)
    assert [e for e in names if e.startswith("advchain_consistency")] and not [e for e in names if "_cw_" in e], names


# ---- bit-reproducibility, layout independence ------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["bf16-bf16", "fp32-fp32"])
@pytest.mark.parametrize("dims", [(37, 52), (7, 9, 80)])
@pytest.mark.parametrize("K", [4, 20])
def test_bit_reproducible(K, dims, pair):
    """(As in tests/test_bf16_loss_gpu.py: at these sizes a slot of the value's 64 float-atomic slots receives at most two
    partial sums, and a sum of two does not depend on their order.)"""
    w = cycle_weights(K)
    for mode in ("perclass", "soft_gt"):
        pred, r, mask, is_gt = _case(mode, K, dims, pair)
        one = _product(pred, r, *FULL, mask, is_gt, w)
        two = _product(pred, r, *FULL, mask, is_gt, w)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(one[2], two[2]), (K, dims, pair, mode)


def _layouts(t):
    """A device tensor as a non-contiguous view x[..., 1:], as its contiguous copy and -- bf16 -- as a contiguous tensor that
    starts one element (2 bytes) into a flat buffer."""
    base = torch.zeros(t.shape[:-1] + (t.shape[-1] + 1,), dtype=t.dtype, device=DEV)
    base[..., 1:] = t.to(DEV)
    view = base[..., 1:]
    assert not view.is_contiguous()
    out = {"view": view, "copy": view.contiguous()}
    if t.dtype == BF16:
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        off = flat[1:].view(t.shape)
        off.copy_(view)
        assert off.is_contiguous() and off.data_ptr() % 8 == 2
        out["offset"] = off
    return out


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims,K", [((12, 64), 20), ((4, 6, 16), 5)])
def test_layout_independence(dims, K, pair):
    from advchain_amd.common.loss import calc_segmentation_consistency
    pred, r, mask, is_gt = _case("perclass", K, dims, pair)
    w = cycle_weights(K)
    lp, lr = _layouts(pred), _layouts(r)
    results = {}
    for name in ("view", "copy", "offset"):
        a = lp.get(name, lp["copy"]).detach().requires_grad_(True)
        b = lr.get(name, lr["copy"]).detach().requires_grad_(True)
        v = calc_segmentation_consistency(a, b, *FULL, class_weights=w, scales=[0], mask=mask.to(DEV), is_gt=is_gt)
        v.backward()
        results[name] = (v.detach(), a.grad.contiguous(), b.grad.contiguous())
    for name in ("view", "offset"):
        for i in range(3):
            assert torch.equal(results[name][i], results["copy"][i]), (name, i)
    _check(results["copy"], want(pred, r, *FULL, w, mask, is_gt), pred, r, (dims, K, pair, "layouts"))


# ---- kl_divergence, two scales ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims,K", [((11, 20), 4), ((3, 5, 7), 20)])
def test_kl_divergence(dims, K, pair):
    from advchain_amd.common.loss import kl_divergence
    pred, r, mask, _ = _case("one", K, dims, pair)
    w = cycle_weights(K)
    a, b = pred.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    v = kl_divergence(b, a, mask=mask.to(DEV), class_weights=w)
    v.backward()
    _check((v.detach(), a.grad, b.grad), want(pred, r, ["kl"], [1.0], w, mask, False), pred, r, (dims, K, pair, "kl_divergence"))


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_two_scales(pair):
    """scales=[0, 1] at (12, 64), K = 4: every scale runs the weighted kernels (a bf16 operand upcast once in front of the pool,
    as without weights).  Against the want evaluated per scale on the torch-pooled upcast operands, sum_s 2^s loss_s / 2."""
    from advchain_amd import _lib
    K, dims = 4, (12, 64)
    pred, r, _, _ = _case("none", K, dims, pair)
    w = cycle_weights(K)
    types, weights = FULL
    lib = _lib.load()
    with lib.timed() as timed:
        del timed.records[:]
        got = _product(pred, r, types, weights, None, False, w, scales=(0, 1))
        torch.cuda.synchronize()
        names = [rec[0] for rec in timed.records]
        del timed.records[:]
    assert names.count("advchain_consistency_cw_fwd") == 2 and not [e for e in names if e.startswith("advchain_consistency")
                                                                    and "_cw_" not in e and e != "advchain_consistency_finish"], names
    oa, ob = pred.detach().float().clone().requires_grad_(True), r.detach().float().clone().requires_grad_(True)
    pool = torch.nn.AvgPool2d(2)
    ov = (weighted_loss(oa, ob, types, weights, w) + 2.0 * weighted_loss(pool(oa), pool(ob), types, weights, w)) / 2.0
    ov.backward()
    _check(got, (float(ov.detach()), oa.grad, ob.grad), pred, r, (dims, K, pair, "scales 0, 1"))


# ---- the solver ------------------------------------------------------------------------------------------------------------

W4 = (0.25, 2.0, 0.0, 1.5)


def _solver(class_weights, hip_graph=False):
    """A noise + bias chain on 2 x 1 x 32 x 32 (no geometric transform: the validity mask is all ones)."""
    from advchain_amd.augmentor import AdvBias, AdvNoise, ComposeAdversarialTransformSolver
    specs = notebook_configs((32, 32), 2, ("noise", "bias"))
    gcls = {"noise": AdvNoise, "bias": AdvBias}
    chain = [gcls[nm](spatial_dims=2, config_dict=cfg, device=DEV) for nm, cfg in specs]
    return ComposeAdversarialTransformSolver(chain_of_transforms=chain, hip_graph=hip_graph, class_weights=class_weights), specs


def _one_step(class_weights):
    solver, specs = _solver(class_weights)
    for i, ((nm, cfg), t) in enumerate(zip(specs, solver.chain_of_transforms)):
        t.init_parameters()
        t.set_parameters(seeded_init_param(nm, tuple(t.param.shape), 300 + i).to(DEV))
    model = make_model(2, k=4, device=DEV)
    with contextlib.redirect_stdout(io.StringIO()):
        loss = solver.adversarial_training(data=smooth_data(2, 1, (32, 32), 17).to(DEV), model=model, n_iter=1, lazy_load=True,
                                           step_sizes=1)
    return solver, loss, [t.param.detach().cpu().clone() for t in solver.chain_of_transforms]


def _loss_of(solver, class_weights):
    from advchain_amd.common.loss import calc_segmentation_consistency
    return float(calc_segmentation_consistency(solver.warped_back_adv_output.detach(), solver.init_output.detach(),
                                               solver.divergence_types, solver.divergence_weights, class_weights=class_weights))


def test_solver_returns_the_weighted_loss():
    solver, loss, _ = _one_step(W4)
    weighted, plain = _loss_of(solver, W4), _loss_of(solver, None)
    tol = 1e-7 + 2e-5 * abs(weighted)
    print("solver loss %.9g weighted %.9g unweighted %.9g" % (float(loss), weighted, plain))
    assert loss.dtype == FP32 and loss.dim() == 0
    assert abs(float(loss) - weighted) < tol
    assert abs(float(loss) - plain) > 10 * tol


def test_solver_with_weight_one_takes_the_unweighted_step():
    """The parameters after one ascent step, w = 1 against None: the 1e-4 parameter contract of the fixtures."""
    _, l1, p1 = _one_step([1.0] * 4)
    _, l0, p0 = _one_step(None)
    assert abs(float(l1) - float(l0)) < 1e-6 + 1e-4 * abs(float(l0))
    for a, b in zip(p1, p0):
        print("w = 1 against None: %.3e" % maxdiff(a, b))
        assert maxdiff(a, b) < 1e-4


def test_new_weights_record_a_new_graph():
    """hip_graph=True: after the capture, assigning other weights is a new signature -- that call runs (and is recorded) the
    ordinary way instead of replaying an ascent against the old weights.  Its loss and its parameters are those of a solver
    without graphs given the same weights, data and seed."""
    model = make_model(2, k=4, device=DEV)
    w2 = (2.0, 0.25, 1.5, 0.0)

    def call(solver, k):
        torch.manual_seed(900 + k)
        with contextlib.redirect_stdout(io.StringIO()):
            loss = solver.adversarial_training(data=smooth_data(2, 1, (32, 32), 40 + k).to(DEV), model=model, n_iter=1,
                                               lazy_load=False, step_sizes=1)
        return float(loss), [t.param.detach().cpu().clone() for t in solver.chain_of_transforms]

    graph, _ = _solver(W4, hip_graph=True)
    for k in range(5):
        call(graph, k)
    st = dict(graph.graph_stats)
    assert st["recorded"] == 3 and st["captures"] == 1 and st["replays"] >= 1 and st["refused"] == 0 and st["violations"] == 0, st
    graph.class_weights = w2
    loss, params = call(graph, 5)
    after = graph.graph_stats
    assert after["recorded"] == 4 and after["replays"] == st["replays"] and after["captures"] == 1, after
    weighted, stale = _loss_of(graph, w2), _loss_of(graph, W4)
    tol = 1e-7 + 2e-5 * abs(weighted)
    print("after the change: loss %.9g, with the new weights %.9g, with the old %.9g" % (loss, weighted, stale))
    assert abs(loss - weighted) < tol and abs(loss - stale) > 10 * tol
    eager, _ = _solver(w2)
    eloss, eparams = call(eager, 5)
    assert abs(loss - eloss) < 1e-6 + 1e-4 * abs(eloss)
    for a, b in zip(params, eparams):
        assert maxdiff(a, b) < 1e-4
    graph.class_weights = W4                       # back to the captured signature: a replay again
    call(graph, 6)
    assert graph.graph_stats["replays"] == st["replays"] + 1 and graph.graph_stats["recorded"] == 4, graph.graph_stats
