"""bf16 logits in the consistency loss and the solver (csrc/loss_lp.hip: advchain_consistency_lp_fwd / lp_bwd / lp_ref_bwd)
against the CPU oracle in fp32.

Operands are those of tests/test_ref_grad_gpu.py at N = 2 with the low-precision ones rounded to bf16; the oracle gets the
upcast of exactly those bf16 tensors, so the want does not depend on the code under test.

Tolerances.  Value: 1e-7 + 2e-5 |v| -- the fp32 contract of tests/test_wide_loss_gpu.py and tests/test_ref_grad_gpu.py; the
forward is fp32 arithmetic on exact upcasts, nothing is added.  Gradient of a bf16 operand, elementwise:
    |g.float() - g_oracle| <= 2^-8 |g_oracle| + 2e-5 max|g_oracle| + 1e-10.
The last two terms are the fp32 contract.  Rounding a value x to bf16 (8 significant bits, to nearest) moves it by at most
2^-8 2^floor(log2 |x|) <= 2^-8 |x|: the first term, with the fp32 allowance left for the distance between x and the oracle's
value (measured on the CPU: the oracle's own gradient rounded to bf16 uses 0.975 of the bound).  The gradient of an fp32
operand of a mixed pair keeps the plain fp32 contract."""
import contextlib
import functools
import io
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import make_model, maxdiff, notebook_configs, seeded_init_param, smooth_data
from tests.test_ref_grad_gpu import FULL, MIXES, MODES, _operands

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BF16, FP32 = torch.bfloat16, torch.float32
PAIRS = {"bf16-bf16": (BF16, BF16), "fp32-bf16": (FP32, BF16), "bf16-fp32": (BF16, FP32)}     # (prediction, reference)

# every shape meets at least two K, every K at least two shapes of each rank
_KS = ((2, 5), (4, 16, 20), (2, 20), (4, 5), (16, 4))
SHAPES_2D = ((1, 7), (11, 20), (37, 52), (6, 252), (64, 256))
SHAPES_3D = ((1, 1, 5), (3, 5, 7), (2, 3, 8), (5, 6, 64), (7, 9, 80))
PARITY = [(d, K) for shapes in (SHAPES_2D, SHAPES_3D) for d, ks in zip(shapes, _KS) for K in ks] + [((9, 20), 1), ((4, 6, 10), 1)]


@functools.lru_cache(maxsize=8)
def _case(mode, K, dims, pair, scale=1.0):
    """(prediction, reference, mask, is_gt) of one mask mode, each operand in the storage type of `pair` (CPU tensors)."""
    pred, ref, mk, onehot, soft = _operands(K, dims)
    one = mk[:, :1].contiguous()
    pt, rt = PAIRS[pair]
    p, r, m, is_gt = {"none": (pred * scale, ref * scale, None, False), "one": (pred * scale, ref * scale, one, False),
                      "perclass": (pred * scale, ref * scale, mk, False), "one_gt": (pred * scale, onehot, one, True),
                      "soft_gt": (pred * scale, soft, one, True)}[mode]
    return p.to(pt), r.to(rt), m, is_gt


def _oracle(pred, r, types, weights, mask, is_gt):
    """(value, prediction.grad, reference.grad or None) of the oracle in fp32 on the upcast operands."""
    from oracle import advchain_oracle as O
    a, b = pred.detach().float().clone().requires_grad_(True), r.detach().float().clone().requires_grad_(True)
    v = O.consistency_loss(a, b, types, weights, mask=mask, is_gt=is_gt)
    v.backward()
    return float(v.detach()), a.grad, b.grad


def _product(pred, r, types, weights, mask, is_gt, pred_grad=True, ref_grad=True, scales=(0,)):
    """(value tensor, prediction.grad, reference.grad) of the product, device tensors as autograd left them."""
    from advchain_amd.common.loss import calc_segmentation_consistency
    a = pred.to(DEV).requires_grad_(pred_grad)
    b = r.to(DEV).requires_grad_(ref_grad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v = calc_segmentation_consistency(a, b, types, weights, scales=list(scales), mask=None if mask is None else mask.to(DEV),
                                          is_gt=is_gt)
    v.backward()
    return v.detach(), a.grad, b.grad


def _excess(got, want, lowp):
    """max over the elements of |got - want| / bound (<= 1 passes; the fp32 contract is strict)."""
    want = want.double()
    tol = (2.0 ** -8 * want.abs() if lowp else 0.0) + 2e-5 * float(want.abs().max()) + 1e-10
    return float(((got.double() - want).abs() / tol).max())


def _close(got, want, dtype, tag):
    assert got.dtype == dtype, tag
    lowp = dtype == BF16
    ex = _excess(got.float().cpu(), want, lowp)
    print("%s: %.3f of the %s bound" % (tag, ex, "bf16" if lowp else "fp32"))
    assert (ex <= 1.0) if lowp else (ex < 1.0), tag


def _check(got, want, pred, r, tag):
    v, gp, gr = got
    assert v.dtype == FP32 and v.dim() == 0, tag
    assert abs(float(v) - want[0]) < 1e-7 + 2e-5 * abs(want[0]), tag + ("value", float(v), want[0])
    _close(gp, want[1], pred.dtype, tag + ("prediction.grad",))
    if gr is None:
        assert want[2] is None or float(want[2].abs().max()) == 0.0, tag
    else:
        _close(gr, torch.zeros_like(r, dtype=FP32) if want[2] is None else want[2], r.dtype, tag + ("reference.grad",))


# ---- 1. parity, 2. dtypes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mix", range(len(MIXES)))
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims,K", PARITY)
def test_matches_the_oracle(dims, K, pair, mix):
    types, weights = MIXES[mix]
    for mode in MODES:
        pred, r, mask, is_gt = _case(mode, K, dims, pair)
        got = _product(pred, r, types, weights, mask, is_gt)
        # no reference gradient exactly where the fp32 path has none: is_gt with 'kl' alone (K = 1 has no contour term)
        cut = is_gt and "mse" not in types and not ("contour" in types and K > 1)
        assert (got[2] is None) == cut, (dims, K, pair, mode)
        _check(got, _oracle(pred, r, types, weights, mask, is_gt), pred, r, (dims, K, pair, tuple(types), mode))


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_gradients_have_their_operands_dtype(pair):
    pred, r, mask, is_gt = _case("one", 4, (11, 20), pair)
    v, gp, gr = _product(pred, r, *FULL, mask, is_gt)
    assert gp.dtype == pred.dtype == PAIRS[pair][0] and gr.dtype == r.dtype == PAIRS[pair][1]
    assert gp.shape == pred.shape and gr.shape == r.shape
    assert v.dtype == FP32 and v.dim() == 0


# ---- 3. the intermediate is not bf16 ---------------------------------------------------------------------------------------

def _parked_in_bf16(pred, r, types, weights):
    """The prediction's gradient as a kernel would give it that rounds the probability-space gradient g_k of 'mse' + 'contour'
    to bf16 between its sweeps (dot = sum_k g_k P_k from the unrounded values, as k_wide_bwd keeps it in registers), from the
    oracle's probabilities; and the same expression without the rounding (a check of the emulation itself)."""
    from oracle import advchain_oracle as O
    w = dict(zip(types, weights))
    K = pred.shape[1]
    P = torch.softmax(pred, 1).detach().requires_grad_(True)
    T = torch.softmax(r, 1)
    ones = torch.ones_like(pred)
    edge = sum(O._contour_term(P[:, [i]], T[:, [i]], ones) for i in range(1, K)) / (K - 1)
    (w["mse"] * F.mse_loss(P, T) / (ones.numel() / K) + w["contour"] * edge).backward()
    g, Pd = P.grad, P.detach()
    dot = (g * Pd).sum(1, keepdim=True)
    b = pred.clone().requires_grad_(True)
    O.consistency_loss(b, r, ["kl"], [w["kl"]]).backward()
    return Pd * (g.bfloat16().float() - dot) + b.grad, Pd * (g - dot) + b.grad


def test_the_backward_intermediate_does_not_pass_through_bf16():
    """(37, 52), K = 20, 'mse' + 'kl' + 'contour', logits scaled by 8 (the scale asked for: no enlargement was needed): softmax
    rows are peaked and P_k (g_k - dot) cancels.  On the CPU first: with g_k rounded to bf16 between the sweeps the bound FAILS
    for this input (7.6 times the bound; 2.9 times already at scale 1), while the same expression without that rounding meets the
    fp32 contract -- so the bound below tells the two schemes apart.  Then the kernels must meet it."""
    pair = "bf16-bf16"
    pred, r, mask, is_gt = _case("none", 20, (37, 52), pair, 8.0)
    want = _oracle(pred, r, *FULL, mask, is_gt)
    parked, exact = _parked_in_bf16(pred.float(), r.float(), *FULL)
    assert _excess(exact, want[1], False) < 1.0
    assert _excess(parked.bfloat16().float(), want[1], True) > 2.0 and _excess(parked, want[1], True) > 2.0
    _check(_product(pred, r, *FULL, mask, is_gt), want, pred, r, (pair, "scale 8"))
    for other in ("fp32-bf16", "bf16-fp32"):
        pred, r, mask, is_gt = _case("none", 20, (37, 52), other, 8.0)
        _check(_product(pred, r, *FULL, mask, is_gt), _oracle(pred, r, *FULL, mask, is_gt), pred, r, (other, "scale 8"))


# ---- 4. only the needed backward is launched -------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims,K", [((37, 52), 4), ((5, 6, 64), 20)])
def test_only_the_needed_backward_is_launched(dims, K, pair):
    from advchain_amd import _lib
    pred, r, mask, is_gt = _case("one", K, dims, pair)
    both = _product(pred, r, *FULL, mask, is_gt)
    lib = _lib.load()
    for kw, absent, present in ((dict(ref_grad=False), "advchain_consistency_lp_ref_bwd", "advchain_consistency_lp_bwd"),
                                (dict(pred_grad=False), "advchain_consistency_lp_bwd", "advchain_consistency_lp_ref_bwd")):
        with lib.timed() as timed:
            del timed.records[:]
            only = _product(pred, r, *FULL, mask, is_gt, **kw)
            torch.cuda.synchronize()
            entries = [rec[0] for rec in timed.records]
            del timed.records[:]
        assert present in entries and absent not in entries, entries
        assert "advchain_consistency_lp_fwd" in entries, entries
        assert not [e for e in entries if e.startswith("advchain_consistency") and "_lp_" not in e
                    and e != "advchain_consistency_finish"], entries
        if "ref_grad" in kw:
            assert only[2] is None and torch.equal(only[1], both[1])
        else:
            assert only[1] is None and torch.equal(only[2], both[2])
        assert torch.equal(only[0], both[0])


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_kl_with_a_ground_truth_reference_has_no_gradient(pair):
    pred, r, mask, is_gt = _case("soft_gt", 4, (11, 20), pair)
    v, gp, gr = _product(pred, r, ["kl"], [1.0], mask, is_gt)
    assert gr is None and gp is not None and gp.dtype == pred.dtype


# ---- 5. layout independence ------------------------------------------------------------------------------------------------

def _layouts(t):
    """A device tensor as a non-contiguous view x[..., 1:], as its contiguous copy and -- bf16 -- as a contiguous tensor that
    starts one element (2 bytes) into a flat buffer."""
    base = torch.zeros(t.shape[:-1] + (t.shape[-1] + 1,), dtype=t.dtype, device=DEV)
    base[..., 1:] = t.to(DEV)
    view = base[..., 1:]
    assert not view.is_contiguous()
    out = {"view": view, "copy": view.contiguous()}
    assert out["copy"].data_ptr() % 16 == 0
    if t.dtype == BF16:
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        off = flat[1:].view(t.shape)
        off.copy_(view)
        assert off.is_contiguous() and off.data_ptr() % 8 == 2
        out["offset"] = off
    return out


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims,K", [((12, 64), 4), ((12, 64), 20), ((4, 6, 16), 5)])
def test_layout_independence(dims, K, pair):
    from advchain_amd.common.loss import calc_segmentation_consistency
    pred, r, mask, is_gt = _case("perclass", K, dims, pair)
    lp, lr = _layouts(pred), _layouts(r)
    results = {}
    for name in ("view", "copy", "offset"):
        a = lp.get(name, lp["copy"]).detach().requires_grad_(True)
        b = lr.get(name, lr["copy"]).detach().requires_grad_(True)
        if name == "view":
            assert not a.is_contiguous() and not b.is_contiguous()
        v = calc_segmentation_consistency(a, b, *FULL, scales=[0], mask=mask.to(DEV), is_gt=is_gt)
        v.backward()
        assert a.grad.shape == pred.shape and b.grad.shape == r.shape
        results[name] = (v.detach(), a.grad.contiguous(), b.grad.contiguous())
    for name in ("view", "offset"):
        assert torch.equal(results[name][0], results["copy"][0]), (name, float(results[name][0]), float(results["copy"][0]))
        assert torch.equal(results[name][1], results["copy"][1]), name
        assert torch.equal(results[name][2], results["copy"][2]), name
    _check(results["copy"], _oracle(pred, r, *FULL, mask, is_gt), pred, r, (dims, K, pair, "layouts"))


# ---- 6. bit-reproducibility ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims", [(37, 52), (7, 9, 80)])
@pytest.mark.parametrize("K", [4, 20])
def test_bit_reproducible(K, dims, pair):
    """(The value's partial sums meet in 64 float-atomic slots, slot = (workgroup + 7 n) mod 64: at these sizes a slot receives
    at most two, and a sum of two does not depend on their order.)"""
    for mode in ("perclass", "soft_gt"):
        pred, r, mask, is_gt = _case(mode, K, dims, pair)
        one = _product(pred, r, *FULL, mask, is_gt)
        two = _product(pred, r, *FULL, mask, is_gt)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(one[2], two[2]), (K, dims, pair, mode)


# ---- 7. kl_divergence, 8. two scales ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims,K", [((11, 20), 4), ((3, 5, 7), 20)])
def test_kl_divergence(dims, K, pair):
    from advchain_amd.common.loss import kl_divergence
    pred, r, mask, _ = _case("one", K, dims, pair)
    a, b = pred.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    v = kl_divergence(b, a, mask=mask.to(DEV))
    v.backward()
    _check((v.detach(), a.grad, b.grad), _oracle(pred, r, ["kl"], [1.0], mask, False), pred, r, (dims, K, pair, "kl_divergence"))


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("dims", [(12, 64), (4, 6, 16)])
def test_two_scales(dims, pair):
    """scales=[0, 1]: a call with a scale > 0 upcasts a bf16 operand ONCE, in front of the pool, and every scale -- scale 0
    too -- then runs the fp32 kernels on that copy, so that the scales' gradients add up in fp32 and the cast rounds their sum
    once (two bf16 gradients added in bf16 would be rounded three times and miss the bound).  This test therefore exercises the
    upcast and the fp32 kernels, not csrc/loss_lp.hip.  Against the oracle evaluated per scale on the torch-pooled upcast
    operands, sum_s 2^s loss_s / 2."""
    from oracle import advchain_oracle as O
    K = 4
    pred, r, _, _ = _case("none", K, dims, pair)
    types, weights = FULL
    got = _product(pred, r, types, weights, None, False, scales=(0, 1))
    oa, ob = pred.detach().float().clone().requires_grad_(True), r.detach().float().clone().requires_grad_(True)
    pool = torch.nn.AvgPool2d(2) if len(dims) == 2 else torch.nn.AvgPool3d(2)
    ov = (O.consistency_loss(oa, ob, types, weights) + 2.0 * O.consistency_loss(pool(oa), pool(ob), types, weights)) / 2.0
    ov.backward()
    _check(got, (float(ov.detach()), oa.grad, ob.grad), pred, r, (dims, K, pair, "scales 0, 1"))


# ---- 9. the solver ---------------------------------------------------------------------------------------------------------

class _Bf16Out(torch.nn.Module):
    """A model whose output is bf16 (what autocast leaves), or -- `back` -- that output upcast again: the fp32 view of the
    same numbers."""

    def __init__(self, inner, back):
        super(_Bf16Out, self).__init__()
        self.inner, self.back = inner, back

    def forward(self, x):
        y = self.inner(x).bfloat16()
        return y.float() if self.back else y


CHAINS = {"a": ["noise", "bias"], "b": ["noise", "bias", "morph", "affine"]}


def _solver_run(which, names, n_iter):
    """One adversarial_training call on 2 x 1 x 32 x 32 with a 4-class model: which = 'oracle' (CPU, `.bfloat16().float()`
    model), 'fp32' (this package, the same model: the fp32 path) or 'bf16' (this package, bf16 model output)."""
    from oracle import advchain_oracle as O
    from advchain_amd.augmentor import AdvAffine, AdvBias, AdvMorph, AdvNoise, ComposeAdversarialTransformSolver
    dims, N = (32, 32), 2
    specs = notebook_configs(dims, N, names)
    data = smooth_data(N, 1, dims, 17)
    ocls = {"noise": O.OracleNoise, "bias": O.OracleBias, "morph": O.OracleMorph, "affine": O.OracleAffine}
    gcls = {"noise": AdvNoise, "bias": AdvBias, "morph": AdvMorph, "affine": AdvAffine}
    if which == "oracle":
        chain = [ocls[nm](2, cfg) for nm, cfg in specs]
    else:
        chain = [gcls[nm](spatial_dims=2, config_dict=cfg, device=DEV) for nm, cfg in specs]
    for i, ((nm, cfg), t) in enumerate(zip(specs, chain)):
        t.init_parameters()
        p = seeded_init_param(nm, tuple(t.param.shape), 300 + i)
        if which == "oracle":
            t.param = p.clone()
        else:
            t.set_parameters(p.to(DEV))
    if which == "oracle":
        solver, model = O.OracleSolver(chain), _Bf16Out(make_model(2, k=4), True)
    else:
        solver = ComposeAdversarialTransformSolver(chain_of_transforms=chain)
        model = _Bf16Out(make_model(2, k=4, device=DEV), which == "fp32")
        data = data.to(DEV)
    with contextlib.redirect_stdout(io.StringIO()):
        loss = solver.adversarial_training(data=data, model=model, n_iter=n_iter, lazy_load=True, step_sizes=1)
    return solver, model, loss, [t.param.detach().cpu().clone() for t in chain]


@functools.lru_cache(maxsize=None)
def _solver_want(chain, n_iter):
    _, _, loss, params = _solver_run("oracle", tuple(CHAINS[chain]), n_iter)
    return float(loss), params


@pytest.mark.parametrize("n_iter", [0, 1])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_solver_with_a_bf16_model(chain, n_iter):
    """A model whose output is bf16 needs no wrapper.  Loss: |d| < 1e-6 + 1e-4 |loss| against the oracle run with the
    `.bfloat16().float()` model (the solver contract of the fixtures).  Transform parameters after one ascent step: with d0 the
    distance between the oracle and this package's fp32 path on that same model (per transform), the bf16 path must be within
    max(1e-4, 2 d0) of the oracle -- the gradient the model receives is rounded to bf16 in both runs, and a rounding that flips
    may move a normalised update."""
    names = tuple(CHAINS[chain])
    oloss, oparams = _solver_want(chain, n_iter)
    solver, model, loss, params = _solver_run("bf16", names, n_iter)
    assert solver.init_output.dtype == BF16
    assert loss.dtype == FP32 and loss.dim() == 0 and bool(torch.isfinite(loss))
    model.zero_grad()
    loss.backward()
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    print("chain %s n_iter %d: loss %.9g oracle %.9g" % (chain, n_iter, float(loss), oloss))
    assert abs(float(loss) - oloss) < 1e-6 + 1e-4 * abs(oloss), (float(loss), oloss)
    if n_iter:
        _, _, floss, fparams = _solver_run("fp32", names, n_iter)
        assert abs(float(floss) - oloss) < 1e-6 + 1e-4 * abs(oloss), (float(floss), oloss)
        for nm, o, f, b in zip(names, oparams, fparams, params):
            d0, db = maxdiff(f, o), maxdiff(b, o)
            print("chain %s %s: d0 %.3e bf16 %.3e bound %.3e" % (chain, nm, d0, db, max(1e-4, 2 * d0)))
            assert db <= max(1e-4, 2 * d0), (chain, nm, d0, db)


# ---- 10. the gate ----------------------------------------------------------------------------------------------------------

def test_float16_is_refused_by_name():
    from advchain_amd import _lib
    from advchain_amd.common.loss import calc_segmentation_consistency, kl_divergence
    x = torch.zeros(1, 4, 8, 8, device=DEV)
    for a, b in ((x.half(), x), (x, x.half()), (x.half(), x.bfloat16())):
        with pytest.raises(_lib.AdvchainHipError, match=r"got torch\.float16"):
            calc_segmentation_consistency(a, b, ["mse", "contour"], [1.0, 0.5])
        with pytest.raises(_lib.AdvchainHipError, match=r"got torch\.float16"):
            kl_divergence(b, a)
