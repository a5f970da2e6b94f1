"""Deterministic mode for the GENERAL float-atomic warps (include/advchain_hip.h: advchain_grid_sample_bwd_det,
advchain_affine_warp_bwd_det): warps of more than four channels (the K-channel prediction of a model with more than four
classes), nearest and size-changing warps, and the affine scatter of more than eight channels.  With the switch on, their
grad_in is accumulated as 64-bit fixed point (2^40 / max |grad_out| of the batch entry) with integer atomics into an int64
image and converted by a last pass.

What must hold:
  * the same gradients as CPU autograd through F.grid_sample / F.affine_grid, within the bound tests/test_deterministic_gpu.py
    uses for the same fixed-point scheme: 5e-5 * max(1, max |grad|);
  * repeated calls are equal BIT FOR BIT, also where hundreds of samples land in one cell (a contraction);
  * grad_grid / grad_theta, which never needed atomics, are bit for bit those of the default mode;
  * a batch entry's bits do not depend on the rest of the batch; a non-finite gradient turns its entry into NaN;
  * a whole solver call with a 6- or 20-class model is bit-reproducible, launch by launch and replayed from a graph.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import make_model, maxdiff, rand, smooth_data
from tests.test_ops_gpu import _smooth_field

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 5e-5


@pytest.fixture
def det():
    from advchain_amd import ops
    ops.set_deterministic(True)
    try:
        yield ops
    finally:
        ops.set_deterministic(False)


def _bound(ref):
    return TOL * max(1.0, float(ref.abs().max()))


def _identity(dims):
    from oracle import advchain_oracle as O
    return O.identity_grid(2, dims).contiguous()


def _fields(dims):
    """A smooth field of 3 px / 2 voxels, and a contraction: every output sample lands in the middle tenth of the input, so
    each cell there receives hundreds of deposits (2D; dozens per cell and channel in 3D)."""
    return [("smooth", _smooth_field(dims, 3.0 if len(dims) == 2 else 2.0, 31)), ("contract", (0.1 * _identity(dims)).contiguous())]


def _autograd(inp, grid, wv, interp, pad, clamp):
    a, g = inp.clone().requires_grad_(True), grid.clone().requires_grad_(True)
    gp = torch.clamp(g, -1, 1) if clamp else g
    perm = (0, 2, 3, 1) if inp.dim() == 4 else (0, 2, 3, 4, 1)
    (F.grid_sample(a, gp.permute(*perm), mode="nearest" if interp else "bilinear", padding_mode=pad, align_corners=True)
     * wv).sum().backward()
    return a.grad, g.grad


def _check_warp(ops, inp, grid, wv, interp, pad, clamp, tag):
    """Parity with autograd, three repeats bit for bit, grad_in the same bits without grad_grid, grad_grid the default mode's."""
    want_in, want_grid = _autograd(inp, grid, wv, interp, pad, clamp)
    args = (wv.to(DEV), inp.to(DEV), grid.to(DEV), interp, ops.pad_code(pad), clamp)
    gin, ggrid = ops.raw_grid_sample_bwd(*args, True, True)
    err_in, err_grid = maxdiff(gin.cpu(), want_in), maxdiff(ggrid.cpu(), want_grid)
    print("%s: grad_in err %.2e of bound %.2e, grad_grid err %.2e of bound %.2e"
          % (tag, err_in, _bound(want_in), err_grid, _bound(want_grid)))
    assert err_in < _bound(want_in), tag
    assert err_grid < _bound(want_grid), tag
    for _ in range(3):
        again, gg = ops.raw_grid_sample_bwd(*args, True, True)
        assert torch.equal(again, gin) and torch.equal(gg, ggrid), tag
    only, none = ops.raw_grid_sample_bwd(*args, True, False)
    assert none is None and torch.equal(only, gin), tag
    ops.set_deterministic(False)
    try:
        gin0, ggrid0 = ops.raw_grid_sample_bwd(*args, True, True)
    finally:
        ops.set_deterministic(True)
    assert torch.equal(ggrid, ggrid0), tag
    assert maxdiff(gin, gin0) < _bound(want_in), tag


@pytest.mark.parametrize("C", [5, 6, 20])
@pytest.mark.parametrize("dims", [(33, 47), (64, 96), (9, 18, 20)])
def test_wide_warp_backward_matches_autograd_and_repeats_bit_for_bit(det, dims, C):
    ops = det
    inp, wv = rand((2, C) + dims, 11 + C), rand((2, C) + dims, 21 + C)
    for name, grid in _fields(dims):
        for pad in ("zeros", "border", "reflection"):
            for clamp in (False, True):
                _check_warp(ops, inp, grid, wv, 0, pad, clamp, (dims, C, name, pad, clamp))


@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("interp", [0, 1])
def test_nearest_and_size_changing_warps_take_the_twin(det, C, interp):
    """(40, 56) -> (24, 31), linear and nearest, and nearest at equal sizes: calls that end in the general kernel at any C."""
    ops = det
    idims, odims = (40, 56), (24, 31)
    inp, wv = rand((2, C) + idims, 41 + C), rand((2, C) + odims, 51 + C)
    for name, grid in _fields(odims):
        for pad, clamp in (("zeros", False), ("border", True), ("reflection", False)):
            _check_warp(ops, inp, grid, wv, interp, pad, clamp, (C, interp, name, pad, clamp))
    if interp == 1:
        same, w2 = rand((2, C) + odims, 61 + C), rand((2, C) + odims, 71 + C)
        for name, grid in _fields(odims):
            _check_warp(ops, same, grid, w2, 1, "zeros", False, (C, "nearest, same size", name))


def test_wide_scatter_keeps_batch_entries_apart_and_surfaces_non_finite_gradients(det):
    """The rules of test_deterministic_scatter_keeps_batch_entries_apart_and_surfaces_non_finite_gradients at C = 6: the scale is
    a batch ENTRY's max |grad_out|.  (Float atomics poison only the cells a NaN touches: the NaN part fails without the twin.)"""
    ops = det
    dims, C = (33, 47), 6
    phi = _smooth_field(dims, 3.0, 71).to(DEV)
    inp, wv = rand((2, C) + dims, 72).to(DEV), rand((2, C) + dims, 73).to(DEV)
    both, _ = ops.raw_grid_sample_bwd(wv, inp, phi, 0, 0, True, True, True)
    one, _ = ops.raw_grid_sample_bwd(wv[:1].contiguous(), inp[:1].contiguous(), phi[:1].contiguous(), 0, 0, True, True, True)
    assert torch.equal(both[:1], one)
    big = wv.clone()
    big[1] *= 1e6
    scaled, _ = ops.raw_grid_sample_bwd(big, inp, phi, 0, 0, True, True, True)
    assert torch.equal(scaled[:1], one)
    bad = wv.clone()
    bad[1, 2, 5, 7] = float("nan")
    got, _ = ops.raw_grid_sample_bwd(bad, inp, phi, 0, 0, True, True, True)
    assert torch.equal(got[:1], one) and bool(torch.isnan(got[1]).all())
    bad[1, 2, 5, 7] = float("inf")
    got, _ = ops.raw_grid_sample_bwd(bad, inp, phi, 0, 0, True, True, True)
    assert torch.equal(got[:1], one) and bool(torch.isnan(got[1]).any())


def test_the_quantum_is_the_entry_maximum_over_2_to_the_40(det):
    """grad_out = 1.0 in one place and 2^-50 in a distant corner, identity grid: the deposit of the small element is 2^-10 of a
    fixed-point unit and rounds to nothing -- its cell is exactly 0.0 in deterministic mode, and 2^-50 (times a weight within an
    ulp of 1) with float atomics."""
    ops = det
    dims, C = (16, 16), 5
    grid = _identity(dims).to(DEV)
    inp = rand((2, C) + dims, 81).to(DEV)
    wv = torch.zeros((2, C) + dims, device=DEV)
    wv[0, 1, 3, 4] = 1.0
    wv[0, 1, 14, 13] = 2.0 ** -50
    gin, _ = ops.raw_grid_sample_bwd(wv, inp, grid, 0, 0, False, True, False)
    assert float(gin[0, 1, 14, 13]) == 0.0
    assert abs(float(gin[0, 1, 3, 4]) - 1.0) < 1e-5
    ops.set_deterministic(False)
    gin0, _ = ops.raw_grid_sample_bwd(wv, inp, grid, 0, 0, False, True, False)
    assert float(gin0[0, 1, 14, 13]) != 0.0 and abs(float(gin0[0, 1, 14, 13]) - 2.0 ** -50) < 2.0 ** -60


# ---- affine ---------------------------------------------------------------------------------------------------------------

def _thetas(nd, kind):
    """(2, nd, nd + 1).  "rot": a rotation with mild scale and a small shift.  "zoom_out": the matrix scaled by 6 -- the output
    shows the input at a sixth of its size, most samples fall outside.  "contract": scaled by 1/6 -- every output sample lands in
    the middle sixth of the input, so each cell there receives 36 (2D) / 216 (3D) deposits per channel."""
    th = torch.zeros(2, nd, nd + 1)
    for n in range(2):
        if kind == "rot":
            ang = torch.tensor(0.3 + 0.2 * n)
            c, s = float(torch.cos(ang)), float(torch.sin(ang))
            th[n, 0, 0], th[n, 0, 1], th[n, 1, 0], th[n, 1, 1] = 1.1 * c, -s, s, 0.9 * c
            if nd == 3:
                th[n, 2, 2] = 1.05
                th[n, 0, 2], th[n, 2, 0] = 0.1, -0.08
            th[n, :, nd] = torch.tensor([0.05, -0.03, 0.02][:nd])
        else:
            for a in range(nd):
                th[n, a, a] = 6.0 if kind == "zoom_out" else 1.0 / 6.0
            th[n, 0, 1] = 0.02 * (n + 1)
            th[n, :, nd] = 0.05 * (n + 1)
    return th


def _affine_autograd(inp, theta, wv, interp, pad):
    a, t = inp.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    grid = F.affine_grid(t, list(inp.shape), align_corners=True)
    (F.grid_sample(a, grid, mode=interp if interp == "nearest" else "bilinear", padding_mode=pad, align_corners=True)
     * wv).sum().backward()
    return a.grad, t.grad


def _affine_product(ops, inp, theta, wv, interp, pad):
    a, t = inp.to(DEV).requires_grad_(True), theta.to(DEV).requires_grad_(True)
    (ops.affine_warp(a, t, interp, pad) * wv.to(DEV)).sum().backward()
    return a.grad, t.grad


@pytest.mark.parametrize("C", [9, 20])
@pytest.mark.parametrize("dims", [(40, 56), (10, 12, 16)])
def test_wide_affine_backward_matches_autograd_and_repeats_bit_for_bit(det, dims, C):
    """C > 8: the calls that zero grad_in and scatter every sample.  grad_theta (block partials, fixed-order second stage) must be
    the default mode's bit for bit."""
    ops = det
    nd = len(dims)
    lin = "bilinear"
    inp, wv = rand((2, C) + dims, 91 + C), rand((2, C) + dims, 95 + C)
    cases = [("rot", lin, "zeros"), ("zoom_out", lin, "zeros"), ("contract", lin, "zeros"), ("rot", lin, "border"),
             ("rot", "nearest", "zeros")]
    for kind, interp, pad in cases:
        theta = _thetas(nd, kind)
        tag = (dims, C, kind, interp, pad)
        want_in, want_th = _affine_autograd(inp, theta, wv, interp, pad)
        gin, gth = _affine_product(ops, inp, theta, wv, interp, pad)
        err_in, err_th = maxdiff(gin.cpu(), want_in), maxdiff(gth.cpu(), want_th)
        print("%s: grad_in err %.2e of bound %.2e, grad_theta err %.2e of bound %.2e"
              % (tag, err_in, _bound(want_in), err_th, _bound(want_th)))
        assert err_in < _bound(want_in), tag
        assert err_th < _bound(want_th), tag
        for _ in range(3):
            again, th2 = _affine_product(ops, inp, theta, wv, interp, pad)
            assert torch.equal(again, gin) and torch.equal(th2, gth), tag
        ops.set_deterministic(False)
        try:
            gin0, gth0 = _affine_product(ops, inp, theta, wv, interp, pad)
        finally:
            ops.set_deterministic(True)
        assert torch.equal(gth, gth0), tag
        assert maxdiff(gin, gin0) < _bound(want_in), tag


# ---- solver ---------------------------------------------------------------------------------------------------------------

def _solver(dims, names, N, deterministic, graph=False):
    import bench
    from advchain_amd.augmentor import AdvAffine, AdvBias, AdvMorph, AdvNoise, ComposeAdversarialTransformSolver
    cls = {"noise": AdvNoise, "bias": AdvBias, "morph": AdvMorph, "affine": AdvAffine}
    chain = [cls[nm](spatial_dims=len(dims), config_dict=cfg, device=DEV) for nm, cfg in bench.transform_configs(dims, N, names)]
    return ComposeAdversarialTransformSolver(chain_of_transforms=chain, divergence_types=["mse", "contour"],
                                             divergence_weights=[1.0, 0.5], hip_graph=graph, deterministic=deterministic)


def _call(solver, data, model, n_iter, seed):
    """-> [loss, adv_data, warped_back_adv_output, params...] of one adversarial_training call from seeded initial parameters"""
    torch.manual_seed(seed)
    loss = solver.adversarial_training(data=data, model=model, n_iter=n_iter, lazy_load=False, step_sizes=1, power_iteration=False)
    return ([loss.detach().clone(), solver.adv_data.clone(), solver.warped_back_adv_output.detach().clone()]
            + [t.param.detach().clone() for t in solver.chain_of_transforms])


SOLVER_CASES = [(2, (64, 64), ["noise", "bias", "morph", "affine"], 6), (2, (64, 64), ["noise", "bias", "morph", "affine"], 20),
                (1, (16, 16, 16), ["bias", "morph", "affine"], 20)]


@pytest.mark.parametrize("N,dims,names,K", SOLVER_CASES, ids=["2d_k6", "2d_k20", "3d_k20"])
def test_solver_call_with_a_many_class_model_is_bit_reproducible(N, dims, names, K):
    """Two ascent steps and the final pass, twice from the same seeds: parameters, adversarial data and warped-back prediction
    equal bit for bit; the loss VALUE within 1e-6 (its partial sums arrive in any order).  Against the default mode: within
    1e-4 of scale, the allowance of test_deterministic_mode_with_a_20_class_model without its widening by the oracle's spread."""
    from advchain_amd import ops
    sd = len(dims)
    model = make_model(sd, k=K, device=DEV)
    data = smooth_data(N, 1, dims, 17).to(DEV)
    try:
        solver = _solver(dims, names, N, True)
        a = _call(solver, data, model, 2, 500)
        assert ops.is_deterministic()
        b = _call(solver, data, model, 2, 500)
    finally:
        ops.set_deterministic(False)
    assert all(bool(torch.isfinite(t).all()) for t in a)
    for i, (x, y) in enumerate(zip(a[1:], b[1:])):
        assert torch.equal(x, y), (i, maxdiff(x, y))
    assert abs(float(a[0]) - float(b[0])) <= 1e-6 * abs(float(b[0]))
    c = _call(_solver(dims, names, N, False), data, model, 2, 500)
    assert not ops.is_deterministic()
    for i, (x, y) in enumerate(zip(a[3:], c[3:])):
        err, allowed = maxdiff(x, y), 1e-4 * max(1.0, float(y.abs().max()))
        print("param %d: deterministic vs default %.2e, allowed %.2e" % (i, err, allowed))
        assert err < allowed, (i, err, allowed)
    assert abs(float(a[0]) - float(c[0])) < 1e-6 + 1e-4 * abs(float(c[0]))


def test_deterministic_ascent_with_a_6_class_model_replays_from_a_graph_bit_for_bit():
    """K = 6, 2 x 1 x 64 x 64, full chain, deterministic=True with hip_graph: after the recorded calls the loop is captured;
    two replays from the same initial parameters are equal to each other and to the launch-by-launch deterministic call -- the
    same launches enqueued the ordinary way under the graph's frozen plan, the comparison of
    tests/test_graph_gpu.py::test_replay_is_bit_identical_to_the_same_launches_enqueued_the_ordinary_way.  (Against a call that
    picks its kernels from its own read-backs a replay differs by the C <= 4 backward formulation a margin selected: 1.4e-5
    on the adversarial data here, the 1e-5 of scale tests/test_graph_gpu.py documents; that is not this comparison.)"""
    from advchain_amd import ops
    dims, names, N, n_iter = (64, 64), ["noise", "bias", "morph", "affine"], 2, 2
    model = make_model(2, k=6, device=DEV)
    data = smooth_data(N, 1, dims, 77).to(DEV)
    try:
        graph = _solver(dims, names, N, True, graph=True)
        for k in range(4):
            out = _call(graph, data, model, n_iter, 900)       # (the same draw as the replays below: inside the plan's intervals)
            assert all(bool(torch.isfinite(t).all()) for t in out)
        (rec,) = graph._graphs.values()
        assert rec["state"] == "replay", rec["state"]
        st = dict(graph.graph_stats)
        assert st["captures"] == 1 and st["refused"] == 0 and st["violations"] == 0, st
        r1 = _call(graph, data, model, n_iter, 900)
        r2 = _call(graph, data, model, n_iter, 900)
        st2 = dict(graph.graph_stats)
        assert st2["replays"] == st["replays"] + 2 and st2["violations"] == 0, (st, st2)
        for i, (x, y) in enumerate(zip(r1[1:], r2[1:])):
            assert torch.equal(x, y), ("replay vs replay", i, maxdiff(x, y))
        assert abs(float(r1[0]) - float(r2[0])) <= 1e-6 * abs(float(r2[0]))
        # the same call on a solver that runs launch by launch under the graph's frozen plan
        plain = _solver(dims, names, N, True)
        plain._apply_deterministic(data)
        assert ops.is_deterministic()
        torch.manual_seed(900)
        plain.init_random_transformation(False)
        plan = rec["plan"]
        plan.rewind()
        plan.flag.zero_()
        ops._PLAN = plan
        try:
            io = plain.get_init_output(data=data, model=model)
            plain.chain_of_transforms = plain.optimizing_transform(data=data, model=model, init_output=io, n_iter=n_iter,
                                                                   optimize_flags=[True] * len(names), step_sizes=[1] * len(names))
            plan.finish()
        finally:
            ops._PLAN = None
        assert plan.cursor == len(plan.frozen) and int(plan.flag.item()) == 0
        for i, (t, y) in enumerate(zip(plain.chain_of_transforms, r1[3:])):
            assert torch.equal(t.param.detach(), y), ("replay vs launches", i, maxdiff(t.param.detach(), y))
    finally:
        ops.set_deterministic(False)
