"""3D finite differences, the Jacobian determinant (displacement and positions mode, 2D and 3D) and the fused folding
statistics on the MI355X, against the float64 closed forms of tests/jacobian_forms.py.

Errors are relative to the largest magnitude of the expected tensor.  Values and gradients: 1e-6 against float64 -- the
figure test_deform_gpu.py::test_float64_closed_forms_at_user_size holds the 2D determinant to; torch's own fp32 evaluation of
the 3D closed form sits at 0.4-3.6e-7 of scale.  Only at the two user sizes the bound is max(1e-6, 4 * e32), e32 the error of
the fp32 twin of jacobian_forms on the same inputs, computed in the same test (never the kernel's own error).  The statistics
are compared with the package's own determinant map BITWISE (one device function evaluates both), and with float64 counts
exactly on fields whose float64 determinants keep 1e-4 away from zero.  AdvMorph's gradient through the whole chain: 1e-4, the
exponentiation tolerance of test_deform_gpu.py (the chain, not the determinant, sets that error)."""
import pytest
import torch

from advchain_amd import ops
from tests import jacobian_forms as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

C, R = ops.JACOBIAN_COLS, ops.JACOBIAN_ROWS_MIN
# the issue's shapes, then one on each side of every boundary of the decomposition: a wave owns C = 62 columns (61, 62, 63,
# 2C = 124, 125 are above) and a strip of R rows (R = 4 at these sizes: H = R - 1, R, R + 1 and 2R + 1; planes are not chunked)
SHAPES = [(1, 3, 2, 2, 2), (2, 3, 3, 2, 3), (3, 3, 3, 5, 61), (1, 3, 5, 3, 62), (2, 3, 4, 6, 63), (1, 3, 3, 4, 125),
          (1, 3, 2, R - 1, 2 * C), (1, 3, 2, 2 * R + 1, 2), (2, 3, 2, R, C + 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
AMPS = [0.05, 2.0, 0.3, 1.0, 0.5, 2.0, 0.05, 1.0, 0.3]


def _err(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _close(got, want, tol, what=""):
    e = _err(got, want)
    assert e <= tol, (what, e)


def _rand(shape, seed, amp=1.0):
    """uniform in [-amp, amp], drawn on the host (the same inputs on every machine)"""
    return ((torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * amp).to(DEV)


def _grid(shape, seed, amp):
    """identity sampling grid + a displacement: positions on both sides of the [-1, 1] border"""
    from advchain.augmentor import get_base_grid
    return get_base_grid(shape[0], *shape[2:], device=DEV) + _rand(shape, seed, amp)


def _smooth(shape, seed, amp):
    coarse = _rand((shape[0], shape[1]) + (6,) * (len(shape) - 2), seed, amp)
    mode = "trilinear" if len(shape) == 5 else "bilinear"
    return torch.nn.functional.interpolate(coarse, size=shape[2:], mode=mode, align_corners=True).contiguous()


def _value_and_grad(fn, x, w):
    x = x.detach().clone().requires_grad_(True)
    y = fn(x)
    g, = torch.autograd.grad(y, x, w.to(y.dtype))
    return y.detach(), g


@pytest.mark.parametrize("shape,amp", list(zip(SHAPES, AMPS)), ids=IDS)
def test_image_diff3d_smallest_shapes(shape, amp):
    from advchain.augmentor import calculate_image_diff3D
    n, _, *sp = shape
    x = _rand((n, 2, *sp), 11, amp)                       # C = 2: plane indexing
    ws = [_rand(x.shape, 12 + k) for k in range(3)]
    xg = x.clone().requires_grad_(True)
    got = calculate_image_diff3D(xg)
    x64 = x.double().requires_grad_(True)
    want = F.image_diff(x64)
    assert len(got) == 3
    for a, b in zip(got, want):
        assert a.shape == x.shape
        _close(a, b, 1e-6, "value")
    torch.autograd.backward(got, ws)
    torch.autograd.backward(want, [w.double() for w in ws])
    _close(xg.grad, x64.grad, 1e-6, "all three gradients")
    for k in range(3):                                    # one incoming gradient alone
        x1 = x.clone().requires_grad_(True)
        calculate_image_diff3D(x1)[k].backward(ws[k])
        x2 = x.double().requires_grad_(True)
        F.image_diff(x2)[k].backward(ws[k].double())
        _close(x1.grad, x2.grad, 1e-6, "gradient %d alone" % k)


@pytest.mark.parametrize("shape,amp", list(zip(SHAPES, AMPS)), ids=IDS)
def test_jacobian3d_smallest_shapes(shape, amp):
    from advchain.augmentor import calculate_jacobian_determinant3D
    w = _rand((shape[0], 1) + shape[2:], 21)
    f = _rand(shape, 22, amp)
    det, grad = _value_and_grad(calculate_jacobian_determinant3D, f, w)
    det64, grad64 = _value_and_grad(F.jacobian_det64, f.double(), w)
    assert det.shape == (shape[0], 1) + shape[2:]
    _close(det, det64, 1e-6, "displacement value")
    _close(grad, grad64, 1e-6, "displacement gradient")
    q = _grid(shape, 23, 0.3)
    assert bool((q.abs() > 1).any()) and bool((q.abs() < 1).any())
    det, grad = _value_and_grad(lambda t: calculate_jacobian_determinant3D(t, type='positions'), q, w)
    det64, grad64 = _value_and_grad(lambda t: F.jacobian_det64(t, True), q.double(), w)
    _close(det, det64, 1e-6, "positions value")
    _close(grad, grad64, 1e-6, "positions gradient")
    det, grad = _value_and_grad(lambda t: ops.jacobian_det(t, positions=True, clamp=True), q, w)
    det64, grad64 = _value_and_grad(lambda t: F.jacobian_det64(t, True, True), q.double(), w)
    _close(det, det64, 1e-6, "clamped value")
    _close(grad, grad64, 1e-6, "clamped gradient")
    assert bool((grad[q.abs() > 1] == 0).all())


def test_2d_displacement_mode_is_the_reference_helper():
    from advchain.augmentor import calculate_jacobian_determinant
    for shape in ((2, 2, 5, 63), (1, 2, 2, 2), (3, 2, 40, 130)):
        f, w = _rand(shape, 31), _rand((shape[0], 1) + shape[2:], 32)
        a, ga = _value_and_grad(ops.jacobian_det, f, w)
        b, gb = _value_and_grad(calculate_jacobian_determinant, f, w)
        assert torch.equal(a, b) and torch.equal(ga, gb), shape


@pytest.mark.parametrize("shape", [(2, 2, 5, 63), (1, 2, 2, 2)], ids=["2x2x5x63", "1x2x2x2"])
def test_2d_positions_mode_and_clamp(shape):
    w = _rand((shape[0], 1) + shape[2:], 41)
    q = _grid(shape, 42, 0.3)
    for clamp in (False, True):
        det, grad = _value_and_grad(lambda t: ops.jacobian_det(t, positions=True, clamp=clamp), q, w)
        det64, grad64 = _value_and_grad(lambda t: F.jacobian_det64(t, True, clamp), q.double(), w)
        _close(det, det64, 1e-6, "value, clamp=%s" % clamp)
        _close(grad, grad64, 1e-6, "gradient, clamp=%s" % clamp)


def _stats_equal_map(field, positions, clamp):
    with torch.no_grad():
        det = ops.jacobian_det(field, positions=positions, clamp=clamp)
    st = ops.jacobian_stats(field, positions=positions, clamp=clamp)
    flat = det.flatten(1)
    assert st.neg.dtype == torch.int64 and st.nonpos.dtype == torch.int64
    assert st.min.dtype == torch.float32 and st.max.dtype == torch.float32
    for t in st:
        assert t.shape == (field.shape[0],) and t.device == field.device
    assert torch.equal(st.neg, (flat < 0).sum(1))
    assert torch.equal(st.nonpos, (~(flat > 0)).sum(1))
    assert torch.equal(st.min, flat.amin(1))
    assert torch.equal(st.max, flat.amax(1))
    return st


@pytest.mark.parametrize("shape,amp", list(zip(SHAPES, AMPS)), ids=IDS)
def test_statistics_are_those_of_the_map_bitwise(shape, amp):
    _stats_equal_map(_rand(shape, 51, amp), False, False)
    q = _grid(shape, 52, 0.3)
    _stats_equal_map(q, True, False)
    _stats_equal_map(q, True, True)
    shape2 = (shape[0], 2) + shape[3:]                    # the 2D kernels: every mode
    _stats_equal_map(_rand(shape2, 53, amp), False, False)
    q2 = _grid(shape2, 54, 0.3)
    _stats_equal_map(q2, True, False)
    _stats_equal_map(q2, True, True)


@pytest.mark.parametrize("nd", [3, 2])
def test_statistics_against_float64_with_planted_folds(nd):
    from advchain.augmentor import jacobian_folding_stats
    shape = (4, 3, 9, 14, 70) if nd == 3 else (4, 2, 14, 70)
    f = _smooth(shape, 61, 0.1)
    x = torch.arange(shape[-1], device=DEV, dtype=torch.float32)
    blk = (slice(2, 6), slice(3, 9), slice(20, 50))[3 - nd:]
    for n in (0, 2):                                      # entries 1 and 3 stay fold-free
        f[(n, 0) + blk] += (-1.5 * x)[20:50]             # u = -1.5 x on a block: det ~ -0.5 inside
    det64 = F.jacobian_det64(f)
    assert float(det64.abs().min()) > 1e-4                # a condition on the INPUTS: no determinant near the decision
    neg64, nonpos64, mn64, mx64 = F.stats_of(det64)
    assert neg64.tolist()[1::2] == [0, 0] and min(neg64.tolist()[0::2]) >= blk[-1].stop - blk[-1].start
    st = jacobian_folding_stats(f)
    assert torch.equal(st.neg, neg64) and torch.equal(st.nonpos, nonpos64)
    _close(st.min, mn64, 1e-6, "min")
    _close(st.max, mx64, 1e-6, "max")
    # one NaN in a fold-free entry: exactly the voxels whose stencil reads it stop being positive
    fn = f.clone()
    fn[(1, 1) + (4, 7, 33)[3 - nd:]] = float("nan")
    touched = torch.isnan(F.jacobian_det64(fn)).flatten(1).sum(1)
    assert touched.tolist()[0::2] == [0, 0] and touched[3] == 0 and int(touched[1]) >= 2 * nd
    sn = jacobian_folding_stats(fn)
    assert torch.equal(sn.neg, st.neg)
    assert torch.equal(sn.nonpos, st.nonpos + touched)
    assert bool(torch.isfinite(sn.min).all()) and bool(torch.isfinite(sn.max).all())


def _user_size(shape, positions, clamp, seed):
    if positions:
        f = _grid(shape, seed, 0.0) + _smooth(shape, seed + 1, 0.08)
        assert bool((f.abs() > 1).any())
    else:
        f = _smooth(shape, seed + 1, 6.0)
    w = _rand((shape[0], 1) + shape[2:], seed + 2)
    det, grad = _value_and_grad(lambda t: ops.jacobian_det(t, positions=positions, clamp=clamp), f, w)
    det64, grad64 = _value_and_grad(lambda t: F.jacobian_det64(t, positions, clamp), f.double(), w)
    det32, grad32 = _value_and_grad(lambda t: F.jacobian_det32(t, positions, clamp), f, w)
    ev, eg = _err(det, det64), _err(grad, grad64)
    e32v, e32g = _err(det32, det64), _err(grad32, grad64)
    print("jacobian %s positions=%s clamp=%s: value %.3g (fp32 twin %.3g), gradient %.3g (fp32 twin %.3g)"
          % ("x".join(map(str, shape)), positions, clamp, ev, e32v, eg, e32g))
    assert ev <= max(1e-6, 4 * e32v), (ev, e32v)
    assert eg <= max(1e-6, 4 * e32g), (eg, e32g)
    st = ops.jacobian_stats(f, positions=positions, clamp=clamp)
    flat = det.flatten(1)
    assert torch.equal(st.neg, (flat < 0).sum(1)) and torch.equal(st.nonpos, (~(flat > 0)).sum(1))
    assert torch.equal(st.min, flat.amin(1)) and torch.equal(st.max, flat.amax(1))
    neg64, nonpos64, mn64, mx64 = F.stats_of(det64)
    near = (det64.abs() <= 1e-4 * float(det64.abs().max())).flatten(1).sum(1)       # voxels fp32 may decide the other way
    assert bool(((st.neg - neg64).abs() <= near).all()) and bool(((st.nonpos - nonpos64).abs() <= near).all())
    tol = max(1e-6, 4 * e32v) * float(det64.abs().max())
    assert float((st.min.double() - mn64).abs().max()) <= tol and float((st.max.double() - mx64).abs().max()) <= tol


def test_user_size_displacement():
    _user_size((4, 3, 128, 128, 64), False, False, 71)


def test_user_size_positions_clamped():
    _user_size((2, 3, 160, 160, 80), True, True, 75)


def test_reproducible_and_capturable():
    from advchain.augmentor import calculate_image_diff3D
    shape = (2, 3, 9, 37, 130)
    f = _rand(shape, 81, 0.5).requires_grad_(True)
    q = _grid(shape, 82, 0.3).requires_grad_(True)
    w = _rand((2, 1) + shape[2:], 83)
    x = _rand((2, 2) + shape[2:], 84).requires_grad_(True)

    def step():
        det = ops.jacobian_det(f)
        gdet = torch.autograd.grad(det, f, w)[0]
        detq = ops.jacobian_det(q, positions=True, clamp=True)
        gq = torch.autograd.grad(detq, q, w)[0]
        st = ops.jacobian_stats(f)
        sq = ops.jacobian_stats(q, positions=True, clamp=True)
        d3 = calculate_image_diff3D(x)
        gx = torch.autograd.grad(d3, x, (x.detach(), x.detach(), x.detach()))[0]
        return (det.detach(), gdet, detq.detach(), gq, gx) + tuple(st) + tuple(sq) + tuple(t.detach() for t in d3)

    eager, again = step(), step()
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
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


def _morph(nd, train=False):
    from advchain.augmentor import AdvMorph
    ds, vs = ([2, 1, 8, 10, 12], [2, 2, 3]) if nd == 3 else ([2, 1, 32, 32], [4, 4])
    m = AdvMorph(nd, dict(epsilon=1.5, data_size=ds, vector_size=vs), device=DEV)
    m.init_parameters()
    m.set_parameters((torch.rand(ds[0], nd, *vs, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV))
    if train:
        m.train()
    return m


@pytest.mark.parametrize("nd", [3, 2])
def test_advmorph_jacobian_and_folding_stats(nd):
    m = _morph(nd)
    for inverse, eps in ((False, 1.5), (True, -1.5)):
        with torch.no_grad():
            q = m.DemonsCompose(duv=eps * m.param)
            det = m.jacobian_determinant(inverse=inverse)
        assert det.shape == (2, 1) + tuple(q.shape[2:]) and not det.requires_grad
        det64 = F.jacobian_det64(q, True)
        _close(det, det64, 1e-6, "inverse=%s" % inverse)
        st = m.folding_stats(inverse=inverse)
        flat = det.flatten(1)
        assert torch.equal(st.neg, (flat < 0).sum(1)) and torch.equal(st.nonpos, (~(flat > 0)).sum(1))
        assert torch.equal(st.min, flat.amin(1)) and torch.equal(st.max, flat.amax(1))
        want = F.stats_of(det64)
        if float(det64.abs().min()) > 1e-4:
            assert torch.equal(st.neg, want[0]) and torch.equal(st.nonpos, want[1])
        _close(st.min, want[2], 1e-6, "min")
        _close(st.max, want[3], 1e-6, "max")


@pytest.mark.parametrize("nd", [3, 2])
def test_advmorph_jacobian_is_differentiable(nd):
    m = _morph(nd, train=True)
    assert m.param.requires_grad
    det = m.jacobian_determinant()
    assert det.requires_grad
    w = _rand(det.shape, 91)
    (det * w).sum().backward()
    g = m.param.grad.detach().clone()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    p2 = m.param.detach().clone().requires_grad_(True)
    (F.jacobian_det32(m.DemonsCompose(duv=1.5 * p2), True) * w).sum().backward()
    _close(g, p2.grad, 1e-4, "chain gradient")
    # the unweighted sum of the issue's example: finite and non-zero as well
    m.param.grad = None
    m.jacobian_determinant().sum().backward()
    assert bool(torch.isfinite(m.param.grad).all()) and float(m.param.grad.abs().max()) > 0
    assert not m.folding_stats().min.requires_grad


def _solver_run(helpers):
    from advchain.augmentor import AdvMorph, ComposeAdversarialTransformSolver
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
        from advchain.augmentor import calculate_image_diff3D, calculate_jacobian_determinant3D, jacobian_folding_stats
        state = (ops.HINT_SLOT, ops.is_deterministic())
        version = morph.param._version
        morph.jacobian_determinant()
        morph.jacobian_determinant(inverse=True)
        morph.folding_stats()
        morph.folding_stats(inverse=True)
        f = _rand((1, 3, 6, 7, 8), 95).requires_grad_(True)
        calculate_jacobian_determinant3D(f).sum().backward()
        jacobian_folding_stats(f.detach())
        calculate_image_diff3D(f.detach())
        assert (ops.HINT_SLOT, ops.is_deterministic()) == state and morph.param._version == version
    loss = solver.adversarial_training(data=data, model=model, n_iter=1, lazy_load=True)
    return float(loss.detach()), morph.param.detach().clone()


def test_helpers_between_solver_calls_change_nothing():
    l1, p1 = _solver_run(False)
    l2, p2 = _solver_run(True)
    assert l1 == l2 and torch.equal(p1, p2)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")
def test_non_current_device():
    from advchain.augmentor import calculate_image_diff3D, calculate_jacobian_determinant3D, jacobian_folding_stats
    d1 = torch.device("cuda:1")
    f = torch.rand(2, 3, 5, 6, 70) - 0.5
    a = calculate_jacobian_determinant3D(f.to(d1))
    assert a.device == d1 and torch.equal(a.cpu(), calculate_jacobian_determinant3D(f.to(DEV)).cpu())
    s1, s0 = jacobian_folding_stats(f.to(d1)), jacobian_folding_stats(f.to(DEV))
    for u, v in zip(s1, s0):
        assert u.device == d1 and torch.equal(u.cpu(), v.cpu())
    for u, v in zip(calculate_image_diff3D(f.to(d1)), calculate_image_diff3D(f.to(DEV))):
        assert u.device == d1 and torch.equal(u.cpu(), v.cpu())
    x = f.to(d1).requires_grad_(True)
    calculate_jacobian_determinant3D(x, type='positions').sum().backward()
    assert x.grad.device == d1 and bool(torch.isfinite(x.grad).all())
