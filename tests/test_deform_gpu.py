"""The deformation helpers of advchain.augmentor on the MI355X: parity with the reference's recorded values and gradients
(g13), float64 closed forms at user sizes, the exponentiation against the squarings issued one by one, reproducibility,
graph capture, solver state and non-current devices.

Tolerances, relative to the largest magnitude of the expected tensor: the finite differences and the Jacobian forward are
bitwise (one rounding per ATen op, in the reference's order); their backwards differ from autograd's summation order only
(5e-7, 4 ulps).  Composition and the Gaussian: 1e-5 against the fp32 reference (5e-5 against float64 at 128 x 128 x 64,
where the rounding of a normalised position is ~1e-5 px times the field's slope).  Exponentiation: 1e-4 for values and
gradients -- each squaring samples the previous field at rounded positions, and the chain amplifies that rounding up to 2^n
(test_ops_gpu.py holds ONE squaring's gradient to 5e-5).  The dense Gaussian weight is built on the host CPU: 1e-6, since the
vectorised exp of another CPU may differ in the last bit."""
import numpy as np
import pytest
import torch

from advchain_amd import ops
from tests.helpers import Fixture

pytestmark = pytest.mark.gpu
G = Fixture("g13_deform")
META = G.json()
DEV = torch.device("cuda:0")


def _close(got, want, tol, what=""):
    got = got.detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max())
    assert err <= tol * scale, (what, err, scale)


def _t(k, grad=False):
    return G.t(k, DEV).float().contiguous().requires_grad_(grad)


@pytest.mark.parametrize("case", META["diff"], ids=[c["name"] for c in META["diff"]])
def test_image_diff_matches_reference(case):
    from advchain.augmentor import calculate_image_diff
    n = case["name"]
    x = _t(n + "__x", True)
    dx, dy = calculate_image_diff(x)
    assert torch.equal(dx.detach().cpu(), G.t(n + "__dx")) and torch.equal(dy.detach().cpu(), G.t(n + "__dy"))
    torch.autograd.backward([dx, dy], [_t(n + "__gdx"), _t(n + "__gdy")])
    _close(x.grad, G.t(n + "__grad"), 5e-7, n)
    # one of the two gradients alone
    x2 = _t(n + "__x", True)
    calculate_image_diff(x2)[1].backward(_t(n + "__gdy"))
    x3 = _t(n + "__x").double().requires_grad_(True)
    dd = x3.new_zeros(x3.shape)
    dd[..., 0, :] = x3[..., 1, :] - x3[..., 0, :]
    dd[..., -1, :] = x3[..., -1, :] - x3[..., -2, :]
    dd[..., 1:-1, :] = 0.5 * (x3[..., 2:, :] - x3[..., :-2, :])
    dd.backward(_t(n + "__gdy").double())
    _close(x2.grad, x3.grad, 5e-7, n)


@pytest.mark.parametrize("case", META["jac"], ids=[c["name"] for c in META["jac"]])
def test_jacobian_matches_reference(case):
    from advchain.augmentor import calculate_jacobian_determinant
    n = case["name"]
    x = _t(n + "__x", True)
    det = calculate_jacobian_determinant(x)
    assert det.shape == (x.shape[0], 1) + tuple(x.shape[2:])
    assert torch.equal(det.detach().cpu(), G.t(n + "__det")), n
    assert int((det < 0).sum()) == case["negative"]
    det.backward(_t(n + "__g"))
    _close(x.grad, G.t(n + "__grad"), 5e-7, n)


def _diff64(x):
    dx, dy = torch.zeros_like(x), torch.zeros_like(x)
    dx[..., 0] = x[..., 1] - x[..., 0]
    dx[..., -1] = x[..., -1] - x[..., -2]
    dx[..., 1:-1] = 0.5 * (x[..., 2:] - x[..., :-2])
    dy[..., 0, :] = x[..., 1, :] - x[..., 0, :]
    dy[..., -1, :] = x[..., -1, :] - x[..., -2, :]
    dy[..., 1:-1, :] = 0.5 * (x[..., 2:, :] - x[..., :-2, :])
    return dx, dy


def test_float64_closed_forms_at_user_size():
    from advchain.augmentor import calculate_image_diff, calculate_jacobian_determinant
    g = torch.Generator(device=DEV).manual_seed(7)
    x = (torch.rand(32, 2, 256, 256, device=DEV, generator=g) * 2 - 1) * 0.05
    x.requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    det = calculate_jacobian_determinant(x)
    dxx, dxy = _diff64(x64[:, [0]])
    dyx, dyy = _diff64(x64[:, [1]])
    det64 = (1 + dxx) * (1 + dyy) - dxy * dyx
    _close(det, det64, 1e-6, "det")
    w = torch.rand(det.shape, device=DEV, generator=g)
    det.backward(w)
    det64.backward(w.double())
    _close(x.grad, x64.grad, 1e-6, "det grad")
    y = torch.rand(4, 3, 256, 200, device=DEV, generator=g).requires_grad_(True)
    y64 = y.detach().double().requires_grad_(True)
    dx, dy = calculate_image_diff(y)
    ex, ey = _diff64(y64)
    _close(dx, ex, 1e-6, "dx")
    _close(dy, ey, 1e-6, "dy")
    gx, gy = torch.rand_like(y), torch.rand_like(y)
    torch.autograd.backward([dx, dy], [gx, gy])
    torch.autograd.backward([ex, ey], [gx.double(), gy.double()])
    _close(y.grad, y64.grad, 1e-6, "diff grad")


@pytest.mark.parametrize("case", META["comp"], ids=[c["name"] for c in META["comp"]])
def test_composition_matches_reference(case):
    from advchain.augmentor import applyComposition2D, applyComposition3D
    n = case["name"]
    f1, f2 = _t(n + "__flow1", True), _t(n + "__flow2", True)
    fn = applyComposition2D if f1.dim() == 4 else applyComposition3D
    out = fn(f1, f2)
    assert out.shape == G.t(n + "__out").shape
    _close(out, G.t(n + "__out"), 1e-5, n)
    out.backward(_t(n + "__g"))
    _close(f1.grad, G.t(n + "__grad1"), 1e-5, n)
    _close(f2.grad, G.t(n + "__grad2"), 1e-5, n)


@pytest.mark.parametrize("case", META["exp2"], ids=[c["name"] for c in META["exp2"]])
def test_exponentiation_2d_matches_reference(case):
    from advchain.augmentor import vectorFieldExponentiation2D
    n = case["name"]
    v = _t(n + "__duv", True)
    out = vectorFieldExponentiation2D(v, nb_steps=case["nb_steps"], type=case["type"], device=DEV)
    assert out.device == v.device
    _close(out, G.t(n + "__out"), 1e-4, n)
    out.backward(_t(n + "__g"))
    if case["nb_steps"] <= 0:
        assert float(out.detach().abs().max()) == 0.0 and float(v.grad.abs().max()) == 0.0
    else:
        _close(v.grad, G.t(n + "__grad"), 1e-4, n)


@pytest.mark.parametrize("case", META["exp3"], ids=[c["name"] for c in META["exp3"]])
def test_exponentiation_3d_matches_reference(case):
    from advchain.augmentor import vectorFieldExponentiation3D
    n = case["name"]
    v = _t(n + "__duv")
    out = vectorFieldExponentiation3D(v, nb_steps=case["nb_steps"], device=DEV)
    _close(out, G.t(n + "__out"), 1e-5, n)
    # the step count: the value 2^-n of the start field is what the output scales with
    nrm = float(np.sqrt(np.float32(ops.sum_of_squares(v).item()), dtype=np.float32))
    k = case["nb_steps"]
    while nrm / 2.0 ** k > 0.5:
        k += 1
    assert k == case["n_final"]
    if case["n_final"] <= 0:
        assert float(out.abs().max()) == 0.0


def test_exponentiation_is_the_squarings_one_by_one():
    from advchain.augmentor import vectorFieldExponentiation2D
    g = torch.Generator(device=DEV).manual_seed(3)
    # a smooth velocity of up to ~6 px, as the solver integrates (on a rough random field the fp32 rounding of two different
    # sampler implementations crosses kinks and the chain amplifies it to O(1) differences)
    coarse = torch.rand(32, 2, 6, 6, device=DEV, generator=g) * 2 - 1
    v = torch.nn.functional.interpolate(coarse, size=(256, 256), mode="bilinear", align_corners=True).contiguous() * 0.05
    out = vectorFieldExponentiation2D(v, nb_steps=8, device=DEV)
    phi0 = ops.raw_expo_start(v, 2.0 ** -8)
    phi = phi0
    for _ in range(8):
        phi = ops.raw_compose_self_fwd(phi)
    assert torch.equal(out, phi - phi0)
    # ... and against the float32 ATen oracle of the reference's loop
    from oracle.advchain_oracle import field_exponentiation
    want, n = field_exponentiation(v, 8, "ss")
    assert n == 8
    # absolute: phi_n and phi_0 are positions of magnitude ~1 and the result is their difference; test_ops_gpu.py allows
    # 2e-5 between one HIP squaring and F.grid_sample, and there are 8 of them
    assert float((out - want).abs().max()) < 1e-4


def test_exponentiation_gradients_float64():
    from advchain.augmentor import vectorFieldExponentiation2D, vectorFieldExponentiation3D
    from oracle.advchain_oracle import field_exponentiation
    g = torch.Generator(device=DEV).manual_seed(11)
    for shape, n, fn in (((2, 2, 24, 20), 4, vectorFieldExponentiation2D), ((1, 3, 8, 9, 10), 3, vectorFieldExponentiation3D)):
        r = torch.rand(*shape, device=DEV, generator=g) * 2 - 1
        v = (torch.sign(r) * (0.4 + 0.6 * r.abs()) * (1.5 / shape[2])).requires_grad_(True)
        v64 = v.detach().double().requires_grad_(True)
        out = fn(v, nb_steps=n, device=DEV)
        ref, n_ref = field_exponentiation(v64, n, "ss")
        _close(out, ref, 1e-4, "value")
        w = torch.rand(out.shape, device=DEV, generator=g)
        out.backward(w)
        ref.backward(w.double())
        _close(v.grad, v64.grad, 1e-4, "grad")


def test_composition_3d_at_user_size():
    from advchain.augmentor import applyComposition3D
    g = torch.Generator(device=DEV).manual_seed(5)
    f1 = torch.rand(4, 3, 128, 128, 64, device=DEV, generator=g)
    from advchain.augmentor import get_base_grid
    pos = get_base_grid(4, 128, 128, 64, device=DEV) + (torch.rand(4, 3, 128, 128, 64, device=DEV, generator=g) - 0.5) * 0.05
    out = applyComposition3D(f1, pos)
    want = torch.nn.functional.grid_sample(f1.double(), pos.double().permute(0, 2, 3, 4, 1), padding_mode="border",
                                           align_corners=True)
    _close(out, want, 5e-5, "compose3d")


def test_backwards_are_reproducible_and_switch_restored():
    from advchain.augmentor import calculate_image_diff, calculate_jacobian_determinant, vectorFieldExponentiation2D
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.rand(8, 2, 96, 130, device=DEV, generator=g).requires_grad_(True)
    w = torch.rand(8, 1, 96, 130, device=DEV, generator=g)
    a = torch.autograd.grad(calculate_jacobian_determinant(x), x, w)[0]
    b = torch.autograd.grad(calculate_jacobian_determinant(x), x, w)[0]
    assert torch.equal(a, b)
    a = torch.autograd.grad(calculate_image_diff(x), x, (w.expand(8, 2, 96, 130), w.expand(8, 2, 96, 130) * 2))[0]
    b = torch.autograd.grad(calculate_image_diff(x), x, (w.expand(8, 2, 96, 130), w.expand(8, 2, 96, 130) * 2))[0]
    assert torch.equal(a, b)
    before = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        v = ((torch.rand(4, 2, 128, 128, device=DEV, generator=g) * 2 - 1) * 0.3).requires_grad_(True)
        gw = torch.rand(4, 2, 128, 128, device=DEV, generator=g)
        a = torch.autograd.grad(vectorFieldExponentiation2D(v, device=DEV), v, gw)[0]
        b = torch.autograd.grad(vectorFieldExponentiation2D(v, device=DEV), v, gw)[0]
        assert torch.equal(a, b)
        assert ops.is_deterministic()
    finally:
        ops.set_deterministic(before)
    assert ops.is_deterministic() == before


def test_graph_capture_equals_eager():
    from advchain.augmentor import applyComposition2D, calculate_image_diff, calculate_jacobian_determinant
    g = torch.Generator(device=DEV).manual_seed(13)
    x = torch.rand(4, 2, 64, 70, device=DEV, generator=g).requires_grad_(True)
    w = torch.rand(4, 1, 64, 70, device=DEV, generator=g)
    f1 = torch.rand(4, 3, 40, 50, device=DEV, generator=g)
    pos = torch.rand(4, 2, 64, 70, device=DEV, generator=g) * 2.2 - 1.1

    def step():
        det = calculate_jacobian_determinant(x)
        gdet = torch.autograd.grad(det, x, w)[0]
        dx, dy = calculate_image_diff(x)
        gdiff = torch.autograd.grad((dx, dy), x, (x.detach(), x.detach()))[0]
        with torch.no_grad():
            comp = applyComposition2D(f1, pos)
        return det.detach(), gdet, dx.detach(), dy.detach(), gdiff, comp

    eager = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def _solver_run(helpers):
    from advchain.augmentor import (AdvMorph, ComposeAdversarialTransformSolver, applyComposition2D,
                                    calculate_jacobian_determinant, vectorFieldExponentiation2D, vectorFieldExponentiation3D)
    torch.manual_seed(0)
    ds = [2, 1, 32, 32]
    morph = AdvMorph(2, dict(epsilon=1.5, data_size=ds, vector_size=[4, 4]), device=DEV)
    morph.init_parameters()
    morph.set_parameters((torch.rand(2, 2, 4, 4, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV))
    model = torch.nn.Conv2d(1, 4, 3, 1, 1).to(DEV).eval()
    torch.nn.init.constant_(model.bias, 0.1)
    with torch.no_grad():
        model.weight.copy_(torch.rand(model.weight.shape, generator=torch.Generator().manual_seed(2)).to(DEV) - 0.5)
    data = torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    solver = ComposeAdversarialTransformSolver(chain_of_transforms=[morph], deterministic=True)
    solver.adversarial_training(data=data, model=model, n_iter=1, lazy_load=True)
    if helpers:
        state = (ops.HINT_SLOT, ops.is_deterministic())
        hg = torch.Generator(device=DEV).manual_seed(4)     # (the global RNG stays where the solver left it)
        v = (torch.rand(2, 2, 32, 32, device=DEV, generator=hg) - 0.5).requires_grad_(True)
        out = vectorFieldExponentiation2D(v, device=DEV)
        out.sum().backward()
        calculate_jacobian_determinant(out.detach()).sum()
        applyComposition2D(data, out.detach().clamp(-1, 1))
        vectorFieldExponentiation3D(torch.rand(1, 3, 8, 8, 8, device=DEV, generator=hg), device=DEV)
        assert (ops.HINT_SLOT, ops.is_deterministic()) == state
    loss = solver.adversarial_training(data=data, model=model, n_iter=1, lazy_load=True)
    return float(loss.detach()), morph.param.detach().clone()


def test_helpers_between_solver_calls_change_nothing():
    l1, p1 = _solver_run(False)
    l2, p2 = _solver_run(True)
    assert l1 == l2 and torch.equal(p1, p2)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")
def test_non_current_device():
    from advchain.augmentor import calculate_jacobian_determinant, vectorFieldExponentiation2D
    d1 = torch.device("cuda:1")
    x = torch.rand(2, 2, 16, 20)
    a = calculate_jacobian_determinant(x.to(d1))
    assert a.device == d1 and torch.equal(a.cpu(), calculate_jacobian_determinant(x.to(DEV)).cpu())
    v = (x - 0.5) * 0.2
    e = vectorFieldExponentiation2D(v.to(d1), device=d1)
    assert e.device == d1 and torch.equal(e.cpu(), vectorFieldExponentiation2D(v.to(DEV), device=DEV).cpu())
    with pytest.raises(RuntimeError):
        vectorFieldExponentiation2D(v.to(d1))          # 'cuda' resolves to the current device, cuda:0


def test_gaussian_matches_reference():
    from advchain.augmentor import AdvMorph
    for case in META["gauss"]:
        n = case["name"]
        m = AdvMorph(case["nd"], dict(epsilon=1.5, data_size=[1, 1] + [8] * case["nd"], vector_size=[4] * case["nd"]),
                     device=DEV)
        x = _t(n + "__x")
        y = m.gaussian_smooth(x, iter=case["iter"], kernel_size=case["kernel_size"], sigma=case["sigma"])
        _close(y, G.t(n + "__y"), 1e-5, n)
        filt = m.get_gaussian_kernel(kernel_size=case["kernel_size"], sigma=case["sigma"], channels=x.shape[1])
        assert filt.weight.shape[-1] == case["taps"] and filt.weight.device.type == "cuda"
        if case["weight"]:
            _close(filt.weight, G.t(n + "__weight"), 1e-6, n)
        _close(filt(x), ops.gauss_smooth(x, case["sigma"], case["taps"]), 0.0, n)
