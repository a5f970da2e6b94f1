"""Every kernel that takes a softmax -- the supervised losses of csrc/seg_loss.hip, seg_dice.hip, seg_boundary.hip and the
consistency loss of csrc/loss.hip, loss_lp.hip, loss_ref.hip -- on the logit regimes of tests/logit_cases.py: shifted by +-1000,
saturated, mixed scales, +-1e30, classes masked with -inf, NaN / +inf, and the usual randn * 3 as the control.  Each result is held
to a float64 evaluation of the same expression (tests/seg_loss_forms.py, dice_forms.py, edt_forms.py, consistency_forms.py) that
starts from exactly the values the kernel reads (bf16 logits: rounded first).

Tolerances.  Consistency loss: the bounds of tests/test_wide_loss_gpu.py::_check -- value 1e-7 + 2e-5 |v|, gradient 2e-5 of its
maximum + 1e-10 -- in every finite regime, and for bf16 operands the elementwise 2^-8 |g| + 2e-5 max|g| + 1e-10 of
tests/test_bf16_loss_gpu.py: these kernels normalise exp(x - max), so the magnitude of the logits must not matter.

Supervised losses: the bounds of their own tests -- cross entropy 2e-5 |v| (tests/test_seg_loss_gpu.py), Dice and Dice + CE 2e-5
absolute (tests/test_dice_gpu.py), boundary 2e-5 max(|v|, S) (tests/test_boundary_gpu.py), gradients 1e-5 of the largest expected
one (bf16 logits: 1e-2, the rounding of the stored gradient, tests/test_seg_loss_gpu.py::test_cross_entropy_bf16_logits) -- PLUS a
term for the rounding of lse.  These kernels keep lse = max + log(sum) per voxel in fp32 and form p = exp(x - lse) from it in the
backward (and in Dice's second sweep).  With e = 2^-24 the fp32 unit roundoff, the stored lse is off by at most e |lse| and the
difference x - lse is rounded once more, by at most e |x - lse|, which is no more than e |lse| wherever p matters (|x - lse| > |lse|
needs x and lse of opposite sign or |x| > 2 |lse|, a class whose p is below exp(-|lse|)); so the argument of the exponential is off by
at most 2 e L = 2^-23 L, L = max |lse| over the voxels (taken from the float64 reference of the case), and p by the same RELATIVE
amount.  Hence, with E = 2^-23 L:
  * every gradient is linear in the p of its voxel: E relative, added to the 1e-5;
  * cross entropy: a voxel's loss w_y (lse - x_y) is off by at most w_y E, so the value by E times the largest normalised class
    weight times (counted voxels / normaliser): 1 with size_average, N V without;
  * Dice: I and P are sums of p, so dI <= E I, dP <= E P and d dice <= 2 E I / D + dice E P / D <= 2 E dice <= 2 E; the class
    weights omega sum to one: 2 E absolute (Dice + CE: dice_weight 2 E + ce_weight E w_max);
  * boundary: the forward divides exp(x - max) sums and does not read lse; the bound still carries E S (S the size of the summands,
    tests/edt_forms.py::boundary_scale), what a relative error E of every p would do.
At `base` L is about 10 and E about 1e-6, a twentieth of the 2e-5: the control stays at the existing bounds.  At `huge` L = 1e30
makes the bounds mean nothing; there the test asks for finite results and for the exact zeros of the cross-entropy gradient at
the +-1e30 voxels (p is exactly 1 on the label and 0 elsewhere).

Non-finite contracts.  `masked`: with labels, with a soft target in Dice, and in 'mse' / 'contour', values and gradients are finite
and within the bounds, and the gradient at a masked logit is exactly 0; 'kl' and a soft-target cross entropy are NaN or +inf in
float64 themselves (0 * -inf, t * -inf): the kernel's value is NaN exactly where the reference's is and +inf exactly where it is
+inf, nothing more.  `poison`: the value is NaN where the reference's is; the cross entropy's gradient is NaN in exactly the
columns of the two poisoned voxels and within bounds everywhere else.

Every check prints the observed error beside its bound."""
import functools
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import logit_cases as C
from tests.consistency_forms import consistency_closed
from tests.dice_forms import ce_closed_nd, dice_ce_closed, dice_closed
from tests.edt_forms import boundary_closed, boundary_scale, signed_maps_brute
from tests.test_boundary_gpu import _offset_copy
from tests.test_class_weights_cpu import cycle_weights
from tests.test_wide_loss_gpu import MASKS, MIXES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
E23 = 2.0 ** -23
TOL_V, TOL_G, TOL_G_BF16 = 2e-5, 1e-5, 1e-2
ALL_MIXES = MIXES + ((["mse", "contour"], [1.0, 0.5]),)      # (the one mix without 'kl': finite at `masked`)
SUP_IDS = ["%s-K%d" % ("x".join(map(str, d)), K) for d, K in C.SUPERVISED]
CON_IDS = ["%s-K%d" % ("x".join(map(str, d)), K) for d, K in C.CONSISTENCY]


def _L():
    import advchain.common.loss as L
    return L


@functools.lru_cache(maxsize=None)
def _inputs(regime, dims, K, bf16, seed=1):
    return C.logits(regime, C.N, K, dims, seed=seed, bf16=bf16)


@functools.lru_cache(maxsize=None)
def _brute_maps(regime, dims, K, bf16):
    return signed_maps_brute(_inputs(regime, dims, K, bf16)[1], K)


def _weights(K):
    return [0.5 + 0.25 * (k % 5) for k in range(K)]


def _on_device(x, bf16=False, misaligned=False):
    t = x.to(DEV)
    if bf16:
        t = t.bfloat16()
    if misaligned:
        t = _offset_copy(t)
        assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t.requires_grad_(True)


def _same_nonfinite(got, want, what):
    """NaN exactly where the reference is NaN, +inf exactly where it is +inf."""
    got, want = float(got), float(want)
    print("%s: value %r, float64 %r" % (what, got, want))
    assert math.isnan(got) == math.isnan(want), (what, got, want)
    assert (got == math.inf) == (want == math.inf), (what, got, want)


def _lse_max(x64):
    lse = torch.logsumexp(x64.detach(), 1)
    return float(lse[torch.isfinite(lse)].abs().max())


def _supervised(regime, fn, closed, x, others, bf16, what, base_tol, lse_factor, parity_only=False, nan_columns=False,
                misaligned=False, zero_at_huge=False):
    """One supervised loss `fn(logits, *others)` against `closed` in float64.  base_tol(want) is the loss's existing absolute
    value bound, lse_factor what multiplies 2^-23 L in the value bound (module docstring).  parity_only: the reference is NaN
    or +inf itself; nan_columns: `poison`, the gradient's NaN mask is compared too; zero_at_huge: the logits' gradient is exactly
    0 at the +-1e30 voxels."""
    xd = _on_device(x, bf16, misaligned)
    od = [_on_device(o, False, misaligned) for o in others]
    v = fn(xd, *od)
    gs = torch.autograd.grad(v, [xd] + od)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and v.dim() == 0 and gs[0].dtype == xd.dtype
    x64 = x.double().requires_grad_(True)
    o64 = [o.double().requires_grad_(True) for o in others]
    w = closed(x64, *o64)
    gw = torch.autograd.grad(w, [x64] + o64)
    w = w.detach()
    if regime == "poison" or parity_only:
        _same_nonfinite(v, w, what)
        if regime == "poison":
            assert math.isnan(float(w)), what               # (the regime poisons every softmax-family value)
        if not nan_columns:
            return
    L = _lse_max(x64)
    E = E23 * L
    if not nan_columns:
        bound = base_tol(float(w)) + E * lse_factor
        err = abs(float(v) - float(w))
        print("%s: L %.4g; value %.9g, float64 %.9g, |diff| %.3g (bound %.3g)" % (what, L, float(v), float(w), err, bound))
        assert math.isfinite(float(v)), what
        assert err <= bound, (what, float(v), float(w), err, bound)
    for i, (g, gref) in enumerate(zip(gs, gw)):
        g = g.detach().double().cpu()
        if nan_columns:
            assert torch.equal(torch.isnan(g), torch.isnan(gref)), what
            assert int(torch.isnan(gref).sum()) == 2 * x.shape[1], what      # the columns of the two poisoned voxels
            keep = ~torch.isnan(gref)
            g, gref = g[keep], gref[keep]
        assert bool(torch.isfinite(g).all()), what
        gmax = max(float(gref.abs().max()), 1e-30)
        tol = ((TOL_G_BF16 if (bf16 and i == 0) else TOL_G) + (0.0 if (bf16 and i == 0) else E)) * gmax
        gerr = float((g - gref).abs().max())
        print("%s: gradient %d |diff| %.3g of max %.3g (bound %.3g)" % (what, i, gerr, gmax, tol))
        assert gerr <= tol, (what, i, gerr, tol)
        if regime == "masked" and i == 0:
            assert float(g[torch.isinf(x)].abs().max()) == 0.0, what
    if regime == "huge" and zero_at_huge:
        V = math.prod(x.shape[2:])
        g0 = gs[0].detach().float().cpu().reshape(x.shape[0], x.shape[1], V)
        assert float(g0[0][:, C.huge_voxels(V)].abs().max()) == 0.0, what


def _ce_form(y, w, avg):
    """ce_closed_nd of the logits and the labels y, or of the logits and a soft target handed in as a second leaf (y None)."""
    return lambda a, *t: ce_closed_nd(a, t[0] if t else y, w, avg)


def _w_max(w, K):
    return 1.0 if w is None else max(w) / sum(w) * K


# ---- supervised losses ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dims,K", C.SUPERVISED, ids=SUP_IDS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_cross_entropy(regime, dims, K, bf16):
    """cross_entropy_2D / cross_entropy_3D with labels and with a soft target, with and without weights, size_average both ways;
    fp32 also from tensors that start one element off (the scalar instantiations)."""
    L = _L()
    x, y = _inputs(regime, dims, K, bf16)
    soft = C.soft_target(C.N, K, dims)
    fn = L.cross_entropy_2D if len(dims) == 2 else L.cross_entropy_3D
    NV = C.N * math.prod(dims)
    yd = y.to(DEV)
    for w, avg in ((None, True), (_weights(K), True), (_weights(K), False)):
        what = "ce %s %s K=%d %s w=%s avg=%s" % (regime, dims, K, "bf16" if bf16 else "fp32", w is not None, avg)
        factor = _w_max(w, K) * (1.0 if avg else NV)
        for mis in ((False, True) if (not bf16 and w is None) else (False,)):
            _supervised(regime, lambda a: fn(a, yd if not mis else _offset_copy(yd), weight=w, size_average=avg), _ce_form(y, w, avg),
                        x, (), bf16, what + (" misaligned" if mis else "") + " labels", lambda v: TOL_V * abs(v), factor,
                        nan_columns=regime == "poison", misaligned=mis, zero_at_huge=True)
            _supervised(regime, lambda a, t: fn(a, t, weight=w, size_average=avg), _ce_form(None, w, avg), x, (soft,), bf16,
                        what + (" misaligned" if mis else "") + " soft", lambda v: TOL_V * abs(v), factor,
                        parity_only=regime == "masked", misaligned=mis)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dims,K", C.SUPERVISED, ids=SUP_IDS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_dice_and_dice_ce(regime, dims, K, bf16):
    """dice_loss alone and fused with the cross entropy, labels and soft target; batch_dice and ignore_background once each."""
    L = _L()
    x, y = _inputs(regime, dims, K, bf16)
    soft = C.soft_target(C.N, K, dims)
    yd = y.to(DEV)
    w = _weights(K)
    fused = dict(weight=w, dice_weight=0.7, ce_weight=1.3, smooth=0.05)
    fused_factor = 0.7 * 2.0 + 1.3 * _w_max(w, K)

    def label_form(opt):
        # Dice + CE from labels at `masked`: the closed form multiplies the one-hot target into log p, 0 * -inf; its two terms
        # from their own closed forms (the cross entropy gathers the label's log p) are the same number and finite
        if regime != "masked":
            return lambda a: dice_ce_closed(a, y, **opt)
        dopt = {k: v for k, v in opt.items() if k not in ("dice_weight", "ce_weight")}
        return lambda a: opt["ce_weight"] * ce_closed_nd(a, y, opt["weight"], True) + opt["dice_weight"] * dice_closed(a, y, **dopt)
    tag = "%s %s K=%d %s" % (regime, dims, K, "bf16" if bf16 else "fp32")
    for opt in (dict(), dict(batch_dice=True), dict(ignore_background=True)):
        for mis in ((False, True) if (not bf16 and not opt) else (False,)):
            what = "dice %s %s%s" % (tag, opt, " misaligned" if mis else "")
            _supervised(regime, lambda a: L.dice_loss(a, yd if not mis else _offset_copy(yd), **opt), lambda a: dice_closed(a, y, **opt),
                        x, (), bf16, what + " labels", lambda v: TOL_V, 2.0, misaligned=mis)
            _supervised(regime, lambda a, t: L.dice_loss(a, t, **opt), lambda a, t: dice_closed(a, t, **opt), x, (soft,), bf16,
                        what + " soft", lambda v: TOL_V, 2.0, misaligned=mis)
    _supervised(regime, lambda a: L.dice_ce_loss(a, yd, **fused), label_form(fused), x, (), bf16, "dice_ce %s labels" % tag,
                lambda v: TOL_V, fused_factor)
    _supervised(regime, lambda a, t: L.dice_ce_loss(a, t, **fused), lambda a, t: dice_ce_closed(a, t, **fused), x, (soft,), bf16,
                "dice_ce %s soft" % tag, lambda v: TOL_V, fused_factor, parity_only=regime == "masked")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dims,K", C.SUPERVISED, ids=SUP_IDS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_boundary(regime, dims, K, bf16):
    """boundary_loss from labels (maps computed on the device, held to the brute-force float64 maps) and from given maps."""
    L = _L()
    x, y = _inputs(regime, dims, K, bf16)
    yd = y.to(DEV)
    maps64 = _brute_maps(regime, dims, K, bf16)
    given = L.signed_distance_maps(yd, K)
    given64 = given.cpu().double()
    tag = "%s %s K=%d %s" % (regime, dims, K, "bf16" if bf16 else "fp32")

    def bounds(kw):
        """(the loss's own value bound 2e-5 max(|v|, S), S) -- S from the logits with the two poisoned entries set to 0."""
        S = boundary_scale(torch.nan_to_num(x.double(), nan=0.0, posinf=0.0), **kw)
        return (lambda v: TOL_V * max(abs(v), S)), S
    for ign in (True, False):
        for mis in ((False, True) if (not bf16 and ign) else (False,)):
            what = "boundary %s ign=%s%s" % (tag, ign, " misaligned" if mis else "")
            kw = dict(target=y, ignore_background=ign, dist_maps=maps64)
            tol, S = bounds(kw)
            _supervised(regime, lambda a: L.boundary_loss(a, yd if not mis else _offset_copy(yd), ignore_background=ign),
                        lambda a: boundary_closed(a, **kw), x, (), bf16, what + " labels", tol, S, misaligned=mis)
            kw = dict(ignore_background=ign, dist_maps=given64)
            tol, S = bounds(kw)
            _supervised(regime, lambda a: L.boundary_loss(a, dist_maps=given if not mis else _offset_copy(given), ignore_background=ign),
                        lambda a: boundary_closed(a, **kw), x, (), bf16, what + " maps", tol, S, misaligned=mis)


# ---- consistency loss ----------------------------------------------------------------------------------------------------------

def _mask_case(mode, ref, mk):
    """(reference, mask, is_gt) of one mask mode of tests/test_wide_loss_gpu.py."""
    if mode == "none":
        return ref, None, False
    if mode == "one":
        return ref, mk[:, :1].contiguous(), False
    if mode == "perclass":
        return ref, mk, False
    K = ref.shape[1]
    onehot = F.one_hot(torch.nan_to_num(ref, nan=0.0).argmax(1), K).movedim(-1, 1).float().contiguous()
    return onehot, mk[:, :1].contiguous(), True


def _consistency(pred, r, types, weights, mask, is_gt, bf16=False, class_weights=None, ref_grad=False):
    """((value, prediction.grad, reference.grad or None) of the kernels, the same of the float64 form)."""
    from advchain_amd.common.loss import calc_segmentation_consistency
    a = _on_device(pred, bf16)
    b = _on_device(r, bf16 and not is_gt).requires_grad_(ref_grad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v = calc_segmentation_consistency(a, b, types, weights, class_weights=class_weights, scales=[0],
                                          mask=None if mask is None else mask.to(DEV), is_gt=is_gt)
    v.backward()
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and a.grad.dtype == a.dtype
    a64, b64 = pred.double().requires_grad_(True), r.double().requires_grad_(True)
    w = consistency_closed(a64, b64, types, weights, mask, is_gt, class_weights)
    ga, gb = torch.autograd.grad(w, (a64, b64), allow_unused=True)
    gb = torch.zeros_like(b64) if gb is None else gb
    got_b = None if not ref_grad else (torch.zeros_like(b) if b.grad is None else b.grad).detach().double().cpu()
    return (float(v.detach()), a.grad.detach().double().cpu(), got_b), (float(w.detach()), ga, gb)


def _check_grad(g, gref, lowp, what):
    top = float(gref.abs().max())
    tol = (2.0 ** -8 * gref.abs() if lowp else 0.0) + 2e-5 * top + 1e-10
    worst = float(((g - gref).abs() / tol).max())
    print("%s: gradient err %.3e (max %.3e): %.3f of the %s bound" % (what, float((g - gref).abs().max()), top, worst, "bf16" if lowp else "fp32"))
    assert bool(torch.isfinite(g).all()), what
    assert worst <= 1.0 if lowp else worst < 1.0, what


def _check_consistency(regime, got, want, types, what, pred, r, bf16=False, is_gt=False):
    (v, gp, gr), (w, wp, wr) = got, want
    if regime == "poison" or (regime == "masked" and "kl" in types):
        _same_nonfinite(v, w, what)
        return
    err = abs(v - w)
    print("%s: value err %.3e (|v| %.3e, bound %.3e)" % (what, err, abs(w), 1e-7 + 2e-5 * abs(w)))
    assert math.isfinite(v) and err < 1e-7 + 2e-5 * abs(w), what
    _check_grad(gp, wp, bf16, what + " prediction")
    if gr is not None:
        _check_grad(gr, wr, bf16 and not is_gt, what + " reference")
    if regime == "masked":
        assert float(gp[torch.isinf(pred)].abs().max()) == 0.0, what
        if gr is not None and not is_gt:
            assert float(gr[torch.isinf(r)].abs().max()) == 0.0, what


@pytest.mark.parametrize("dims,K", C.CONSISTENCY, ids=CON_IDS)
@pytest.mark.parametrize("regime", C.REGIMES)
def test_consistency_loss(regime, dims, K):
    """calc_segmentation_consistency, every term mix x mask mode of tests/test_wide_loss_gpu.py, one shape per kernel variant; both
    operands of the regime.  The mix without 'kl' (['mse', 'contour']) joins at `masked`, where it is the one mix with a finite
    reference, and at the control.  It is NOT run at the other regimes: measured on the MI355X at `saturated`, (1, 7), K = 17 and
    20, no mask, its gradient misses the bound -- error 1.2e-9 and 1.1e-9 against 2e-5 max|g| + 1e-10 = 1.2e-10 and 1.4e-10
    (max|g| 7.9e-7 and 2.2e-6, value 0.2 within 4e-9) -- and so does the same expression evaluated by torch in fp32 on the CPU.
    With all 14 voxels saturated and no 'kl' term the whole gradient is p_j (h_j - sum_k h_k p_k) with p_j within 1e-7 of 1: a
    difference of fp32 numbers that agree to 7 digits.  Every mix with 'kl' passes there (its gradient is of order 1 / (N V)).
    INTEGRATION.md "Known deviations" states it."""
    pred, _ = _inputs(regime, dims, K, False, 1)
    ref, _ = _inputs(regime, dims, K, False, 2)
    mk = C.binary_mask(C.N, K, dims)
    for types, weights in (ALL_MIXES if regime in ("base", "masked") else MIXES):
        for mode in MASKS:
            r, mask, is_gt = _mask_case(mode, ref, mk)
            got, want = _consistency(pred, r, types, weights, mask, is_gt)
            _check_consistency(regime, got, want, types, "%s %s K=%d %s %s" % (regime, dims, K, types, mode), pred, r)
    from advchain_amd.common.loss import kl_divergence
    v = float(kl_divergence(ref.to(DEV), pred.to(DEV)))
    w = float(consistency_closed(pred.double(), ref.double(), ["kl"], [1.0]))
    what = "kl_divergence %s %s K=%d" % (regime, dims, K)
    if regime in ("poison", "masked"):
        _same_nonfinite(v, w, what)
    else:
        print("%s: value err %.3e (|v| %.3e)" % (what, abs(v - w), abs(w)))
        assert abs(v - w) < 1e-7 + 2e-5 * abs(w), what


@pytest.mark.parametrize("dims,K", [((11, 20), 5), ((1, 7), 20)], ids=["11x20-K5", "1x7-K20"])
@pytest.mark.parametrize("regime", C.REGIMES)
def test_consistency_reference_grad_bf16_and_class_weights(regime, dims, K):
    """A reference that requires grad (csrc/loss_ref.hip, run-time-K form), bf16 operands and class weights, once per regime:
    the full mix with a one-channel mask -- at `masked` the mix without 'kl', whose value and gradients are finite."""
    types, weights = ALL_MIXES[3] if regime == "masked" else ALL_MIXES[2]
    for bf16, cw in ((False, None), (True, None), (False, cycle_weights(K))):
        pred, _ = _inputs(regime, dims, K, bf16, 1)
        ref, _ = _inputs(regime, dims, K, bf16, 2)
        mask = C.binary_mask(C.N, K, dims)[:, :1].contiguous()
        got, want = _consistency(pred, ref, types, weights, mask, False, bf16=bf16, class_weights=cw, ref_grad=True)
        what = "%s %s K=%d %s cw=%s both grads" % (regime, dims, K, "bf16" if bf16 else "fp32", cw is not None)
        _check_consistency(regime, got, want, types, what, pred, ref, bf16=bf16)
