"""What completes the deterministic mode, on the GPU (include/advchain_hip.h, "deterministic mode"):

  * the bicubic backward through its int64 fixed-point twin (advchain_grid_sample_bicubic2d_bwd_det): parity with float64
    autograd within the bound of the default-mode test (tests/test_ops_gpu.py::test_bicubic_grid_sample_and_affine_warp:
    2e-5 * max(1, max|grad|)) plus the quantisation `deposits per cell * max|grad_out| * 2^-bits`; equal bits run to run;
    grad_grid the default mode's bit for bit; the routing, read from lib.timed();
  * the norm behind the 3D step count in a fixed order (ops.field_sumsq -> advchain_tp_interp_sumsq_ordered);
  * the VALUE of the consistency loss in a fixed order (the *_fwd_ord entries) for every forward family, on shapes whose
    launches have at least 130 workgroups and inputs for which the order shows (tests/test_det_complete_cpu.py), and the loss a
    replayed hipGraph call returns against the same call launch by launch.

Every test switches the mode back."""
import math

import pytest
import torch
import torch.nn.functional as F

from advchain_amd import _lib
from tests.helpers import make_model, maxdiff, rand, smooth_data
from tests.test_det_complete_cpu import LOSS_CASES, TYPES, WEIGHTS, launches, loss_inputs, oracle_value, query

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 2e-5          # tests/test_ops_gpu.py


def _ops():
    from advchain_amd import ops
    return ops


@pytest.fixture
def det():
    ops = _ops()
    ops.set_deterministic(True)
    try:
        yield ops
    finally:
        ops.set_deterministic(False)


def to_planar(grid_last):
    return grid_last.permute(0, 3, 1, 2).contiguous()


# ---- bicubic -----------------------------------------------------------------------------------------------------------------

def _bicubic_bits(out_pixels):
    return min(40, 62 - math.ceil(math.log2(16 * out_pixels)))


def _bicubic_product(ops, inp, grid, gout, pad, need_in=True):
    """(grad_in, grad_grid, names and grad_in arguments of the library calls) of one forward + backward."""
    lib = _lib.load()
    a = inp.to(DEV).requires_grad_(need_in)
    g = to_planar(grid).to(DEV).requires_grad_(True)
    del lib.records[:]
    with lib.timed():
        out = ops.grid_sample(a, g, "bicubic", pad)
        out.backward(gout.to(DEV))
        torch.cuda.synchronize()
    calls = [(r[0], r[1][3]) for r in lib.records]          # (argument 3 of the backward entries: grad_in)
    del lib.records[:]
    return a.grad, g.grad, calls


@pytest.mark.parametrize("pad", ["zeros", "border", "reflection"])
def test_bicubic_backward_twin_parity_and_routing(pad):
    """N = 2, C = 3, 9 x 11 -> 8 x 8 (an odd C H W: the second entry's image is 8-byte aligned only), grid points inside, on
    the border and outside."""
    ops = _ops()
    inp, gout = rand((2, 3, 9, 11), 41), rand((2, 3, 8, 8), 42)
    grid = rand((2, 8, 8, 2), 43, -1.3, 1.3)
    grid.view(-1, 2)[0] = torch.tensor([1.0, -1.0])
    grid.view(-1, 2)[1] = torch.tensor([-1.0, 0.5])
    a, g = inp.double().requires_grad_(True), grid.double().requires_grad_(True)
    F.grid_sample(a, g, mode="bicubic", padding_mode=pad, align_corners=True).backward(gout.double())
    want_in = a.grad
    fwd, bwd = "advchain_grid_sample_bicubic2d_fwd", "advchain_grid_sample_bicubic2d_bwd"
    try:
        ops.set_deterministic(False)
        gin0, ggrid0, calls0 = _bicubic_product(ops, inp, grid, gout, pad)
        assert [c[0] for c in calls0] == [fwd, bwd], calls0            # exactly today's calls
        assert calls0[1][1] is not None
        ops.set_deterministic(True)
        gin, ggrid, calls = _bicubic_product(ops, inp, grid, gout, pad)
        names = [c[0] for c in calls]
        assert names == [fwd, bwd + "_det"], calls
        assert not any(n == bwd and gi is not None for n, gi in calls)
        again_in, again_grid, _ = _bicubic_product(ops, inp, grid, gout, pad)
        # grad_grid alone: no deposits, the default entry without grad_in
        _, only_grid, calls_g = _bicubic_product(ops, inp, grid, gout, pad, need_in=False)
        assert [c[0] for c in calls_g] == [fwd, bwd] and calls_g[1][1] is None, calls_g
    finally:
        ops.set_deterministic(False)
    bound = TOL * max(1.0, float(want_in.abs().max())) + 16 * 64 * float(gout.abs().max()) * 2.0 ** -_bicubic_bits(64)
    err = float((gin.cpu().double() - want_in).abs().max())
    print("%s: grad_in err %.3e of bound %.3e (default mode: %.3e)" % (pad, err, bound,
                                                                       float((gin0.cpu().double() - want_in).abs().max())))
    assert err < bound
    assert torch.equal(ggrid, ggrid0) and torch.equal(only_grid, ggrid0)
    assert torch.equal(again_in, gin) and torch.equal(again_grid, ggrid)


def _cubic_coeffs(t):
    A = -0.75
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]


def test_bicubic_twin_under_contention_and_with_non_finite_gradients(det):
    """Every one of 64 x 64 grid points at the same interior location of a 5 x 5 image: 4096 deposits into each of 16 cells,
    bits = min(40, 62 - ceil(log2(16 * 4096))) = 40.  |cx|, |cy| <= 1, so no cell's sum exceeds 4096 * 2^40 < 2^62."""
    ops = det
    gx, gy = torch.tensor(0.15), torch.tensor(-0.2)             # x = 2.3 px (taps 1..4), y = 1.6 px (taps 0..3): all inside
    grid = torch.stack([gx.expand(64, 64), gy.expand(64, 64)], -1)[None].contiguous()
    inp = rand((1, 1, 5, 5), 51)
    ones = torch.ones(1, 1, 64, 64)
    gin, _, calls = _bicubic_product(ops, inp, grid, ones, "zeros")
    assert "advchain_grid_sample_bicubic2d_bwd_det" in [c[0] for c in calls]
    x = (gx.double() + 1) * 0.5 * 4
    y = (gy.double() + 1) * 0.5 * 4
    cx, cy = _cubic_coeffs(float(x) - 2.0), _cubic_coeffs(float(y) - 1.0)
    assert max(abs(c) for c in cx + cy) <= 1.0
    want = torch.zeros(5, 5, dtype=torch.float64)
    for j in range(4):
        for i in range(4):
            want[j, 1 + i] = 4096.0 * cx[i] * cy[j]
    assert _bicubic_bits(4096) == 40
    bound = TOL * max(1.0, float(want.abs().max())) + 16 * 4096 * 1.0 * 2.0 ** -40
    err = float((gin[0, 0].cpu().double() - want).abs().max())
    print("contention: err %.3e of bound %.3e" % (err, bound))
    assert err < bound
    again, _, _ = _bicubic_product(ops, inp, grid, ones, "zeros")
    assert torch.equal(again, gin)
    # one inf in entry 0 of a batch of two: that entry NaN, the other what it is on its own
    inp2 = torch.cat([inp, inp], 0)
    grid2 = torch.cat([grid, grid], 0)
    bad = torch.ones(2, 1, 64, 64)
    bad[0, 0, 17, 33] = float("inf")
    got, _, _ = _bicubic_product(ops, inp2, grid2, bad, "zeros")
    assert bool(torch.isnan(got[0]).all())
    assert torch.equal(got[1], gin[0])


def _chain_solver(dims, names, N, deterministic, graph=False, bicubic=False, types=("mse", "contour"), weights=(1.0, 0.5),
                  morph_vs=None):
    import bench
    from advchain_amd.augmentor import AdvAffine, AdvBias, AdvMorph, AdvNoise, ComposeAdversarialTransformSolver
    cls = {"noise": AdvNoise, "bias": AdvBias, "morph": AdvMorph, "affine": AdvAffine}
    chain = []
    for nm, cfg in bench.transform_configs(dims, N, names):
        cfg = dict(cfg)
        if bicubic and nm in ("morph", "affine"):
            cfg["backward_interp"] = "bicubic"
        if nm == "morph" and morph_vs is not None:
            cfg["vector_size"] = list(morph_vs)
        chain.append(cls[nm](spatial_dims=len(dims), config_dict=cfg, device=DEV))
    return ComposeAdversarialTransformSolver(chain_of_transforms=chain, divergence_types=list(types),
                                             divergence_weights=list(weights), hip_graph=graph, deterministic=deterministic)


def _call(solver, data, model, n_iter, seed):
    torch.manual_seed(seed)
    loss = solver.adversarial_training(data=data, model=model, n_iter=n_iter, lazy_load=False, step_sizes=1, power_iteration=False)
    return ([loss.detach().clone(), solver.adv_data.clone(), solver.warped_back_adv_output.detach().clone()]
            + [t.param.detach().clone() for t in solver.chain_of_transforms])


def test_solver_step_with_bicubic_backward_warps_is_bit_reproducible():
    """2 x 1 x 32 x 32, 4 classes, noise + bias + morph + affine with backward_interp = 'bicubic', one step: the parameters and
    the adversarial data of two identical calls are equal bit for bit, and so is the returned loss."""
    ops = _ops()
    dims, N = (32, 32), 2
    model = make_model(2, k=4, device=DEV)
    data = smooth_data(N, 1, dims, 23).to(DEV)
    lib = _lib.load()
    try:
        solver = _chain_solver(dims, ["noise", "bias", "morph", "affine"], N, True, bicubic=True)
        del lib.records[:]
        with lib.timed(names=("advchain_grid_sample_bicubic2d_bwd", "advchain_grid_sample_bicubic2d_bwd_det")):
            a = _call(solver, data, model, 1, 700)
            torch.cuda.synchronize()
        names = [r[0] for r in lib.records]
        grad_ins = [r[1][3] for r in lib.records if r[0] == "advchain_grid_sample_bicubic2d_bwd"]
        del lib.records[:]
        assert ops.is_deterministic()
        b = _call(solver, data, model, 1, 700)
    finally:
        ops.set_deterministic(False)
    assert "advchain_grid_sample_bicubic2d_bwd_det" in names
    assert all(g is None for g in grad_ins)
    assert all(bool(torch.isfinite(t).all()) for t in a)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, maxdiff(x, y))


# ---- the 3D step count ---------------------------------------------------------------------------------------------------------

def test_step_count_norm_is_ordered_and_the_chain_runs_the_count_it_gives(det):
    """Field 16 x 16 x 8 from 4 x 4 x 4, N = 2 (24 workgroups in the upsampling launch).  The value contract of the project
    (2e-5 relative) against the float64 sum of squares of the materialised field; equal bits over 5 calls; and with the field
    scaled so that norm / 2^9 = 0.35, the chain runs 9 squarings (norm / 2^8 = 0.7 > 0.5 >= norm / 2^9)."""
    from advchain_amd import bands
    ops = det
    tables = bands.upsample_tables([4, 4, 4], [16, 16, 8], DEV)
    coef = rand((2, 3, 4, 4, 4), 61).to(DEV)
    field = ops.raw_tp_interp(coef, tables, 3, want_out=True)
    want = float((field.double() ** 2).sum())
    vals = [ops.field_sumsq(coef, tables, 3) for _ in range(5)]
    assert vals[0].shape == (1,)
    for v in vals[1:]:
        assert torch.equal(v, vals[0])
    rel = abs(float(vals[0]) - want) / want
    print("ordered norm^2 %.9g want %.9g rel %.2e" % (float(vals[0]), want, rel))
    assert rel < 2e-5
    ops.set_deterministic(False)
    slotted = ops.field_sumsq(coef, tables, 3)
    ops.set_deterministic(True)
    assert abs(float(slotted) - want) / want < 2e-5
    # the chain: the smoothed velocity at scale 1 gives the norm per unit of scale
    vel = rand((2, 3, 4, 4, 4), 62).to(DEV)
    s1 = ops.raw_gauss(vel, 3, pre=1, scale=1.0, weights=ops.gauss9(1.0))
    unit = math.sqrt(float(ops.field_sumsq(s1, tables, 3)))
    scale = 0.35 * 2.0 ** 9 / unit
    ops._NSTEPS_HINT.clear()
    q1 = ops.demons_field(vel, scale, tables, True)
    assert list(ops._NSTEPS_HINT.values()) == [9], ops._NSTEPS_HINT
    q2 = ops.demons_field(vel, scale, tables, True)
    assert list(ops._NSTEPS_HINT.values()) == [9]
    assert torch.equal(q1, q2)
    ops._NSTEPS_HINT.clear()


def test_3d_morph_solver_call_is_bit_reproducible():
    """A morph-only solver call at 2 x 1 x 16 x 16 x 8 (low resolution 4 x 4 x 4), deterministic=True, twice."""
    ops = _ops()
    dims, N = (16, 16, 8), 2
    model = make_model(3, k=4, device=DEV)
    data = smooth_data(N, 1, dims, 29).to(DEV)
    try:
        solver = _chain_solver(dims, ["morph"], N, True, morph_vs=(4, 4, 4))
        a = _call(solver, data, model, 1, 800)
        assert ops.is_deterministic()
        b = _call(solver, data, model, 1, 800)
    finally:
        ops.set_deterministic(False)
    assert all(bool(torch.isfinite(t).all()) for t in a)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, maxdiff(x, y))


# ---- the loss value ------------------------------------------------------------------------------------------------------------

def _loss_eval(pred, ref, mask, cw, kl_only=False):
    """(value, prediction.grad, reference.grad) of the product; device tensors."""
    from advchain_amd.common.loss import calc_segmentation_consistency, kl_divergence
    a, b = pred.clone().requires_grad_(True), ref.clone().requires_grad_(True)
    if kl_only:
        v = kl_divergence(b, a, mask=mask, class_weights=cw)
    else:
        v = calc_segmentation_consistency(a, b, TYPES, WEIGHTS, class_weights=cw, scales=[0], mask=mask)
    v.backward()
    return v.detach(), a.grad, b.grad


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_loss_value_is_ordered_in_every_forward_family(name):
    """'mse' + 'contour' + 'kl' (and kl_divergence alone) on the case's shape and mask: with the mode on the value is equal over
    5 evaluations, within 1e-7 + 2e-5 |v| of the oracle, and the gradients are the default mode's bit for bit.  The entry that
    ran is read from lib.timed()."""
    ops = _ops()
    lib = _lib.load()
    family, N, K, dims, mch, _, _ = LOSS_CASES[name]
    assert min(launches(family, N, K, dims, mch)) >= 130 and query(lib, family, N, K, dims, mch) >= 130
    pred, ref, mask, cw = loss_inputs(name)
    want = oracle_value(pred, ref, mask, cw)
    want_kl = oracle_value(pred, ref, mask, cw, ["kl"], [1.0])
    pred, ref, mask = pred.to(DEV), ref.to(DEV), mask.to(DEV)
    entry = {"fused": "advchain_consistency_fused_fwd", "three": "advchain_consistency_fwd", "wide": "advchain_consistency_lp_fwd",
             "lp": "advchain_consistency_lp_fwd", "cw": "advchain_consistency_cw_fwd"}[family]
    ord_entry = "advchain_consistency_lp_fwd_ord" if family in ("wide", "lp", "cw") else entry + "_ord"
    try:
        ops.set_deterministic(False)
        del lib.records[:]
        with lib.timed():
            v0, gp0, gr0 = _loss_eval(pred, ref, mask, cw)
            torch.cuda.synchronize()
        names0 = [r[0] for r in lib.records]
        k0, kp0, kr0 = _loss_eval(pred, ref, mask, cw, kl_only=True)
        ops.set_deterministic(True)
        del lib.records[:]
        with lib.timed():
            v, gp, gr = _loss_eval(pred, ref, mask, cw)
            torch.cuda.synchronize()
        names = [r[0] for r in lib.records]
        del lib.records[:]
        more = [_loss_eval(pred, ref, mask, cw)[0] for _ in range(4)]
        kl = [_loss_eval(pred, ref, mask, cw, kl_only=True) for _ in range(5)]
    finally:
        ops.set_deterministic(False)
    assert entry in names0 and "advchain_consistency_finish" in names0 and not any(n.endswith("_ord") for n in names0), names0
    assert ord_entry in names and "advchain_consistency_finish_ord" in names, names
    assert entry not in names and "advchain_consistency_finish" not in names, names
    print("%s %s: value %.9g (default mode %.9g) oracle %.9g: %.3f of the bound" %
          (name, dims, float(v), float(v0), want, abs(float(v) - want) / (1e-7 + 2e-5 * abs(want))))
    for m in more:
        assert torch.equal(m, v)
    assert abs(float(v) - want) < 1e-7 + 2e-5 * abs(want)
    assert torch.equal(gp, gp0) and torch.equal(gr, gr0)
    assert abs(float(v0) - want) < 1e-7 + 2e-5 * abs(want)
    # kl_divergence
    for kv, kp, kr in kl[1:]:
        assert torch.equal(kv, kl[0][0])
    assert abs(float(kl[0][0]) - want_kl) < 1e-7 + 2e-5 * abs(want_kl), (float(kl[0][0]), want_kl)
    assert torch.equal(kl[0][1], kp0) and torch.equal(kl[0][2], kr0)


def test_replayed_call_returns_the_loss_of_the_same_call_launch_by_launch():
    """2 x 1 x 64 x 64, 4 classes, full chain, hip_graph=True, deterministic=True.  After the recorded calls the loop is
    captured.  A replayed call and the same call enqueued launch by launch under the graph's frozen plan (the comparison of
    tests/test_det_wide_gpu.py) end in the same parameters, so the final pass sees the same tensors: the returned loss is equal
    bit for bit, and so is the loss of the last ascent step, which the replay computes inside the graph (partial buffers from
    the capture's allocations)."""
    ops = _ops()
    dims, names, N, n_iter = (64, 64), ["noise", "bias", "morph", "affine"], 2, 2
    model = make_model(2, k=4, device=DEV)
    data = smooth_data(N, 1, dims, 77).to(DEV)
    try:
        graph = _chain_solver(dims, names, N, True, graph=True)
        for _ in range(4):
            out = _call(graph, data, model, n_iter, 900)
            assert all(bool(torch.isfinite(t).all()) for t in out)
        (rec,) = graph._graphs.values()
        assert rec["state"] == "replay", rec["state"]
        st = dict(graph.graph_stats)
        assert st["captures"] == 1 and st["refused"] == 0 and st["violations"] == 0, st
        r1 = _call(graph, data, model, n_iter, 900)
        inner1 = graph.last_inner_dist.detach().clone()
        r2 = _call(graph, data, model, n_iter, 900)
        st2 = dict(graph.graph_stats)
        assert st2["replays"] == st["replays"] + 2 and st2["violations"] == 0, (st, st2)
        assert torch.equal(r1[0], r2[0])
        # the same call, launch by launch, under the graph's frozen plan
        plain = _chain_solver(dims, names, N, True)
        plain._resolve_global_batch(data.size(0), data.device)
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
        dist = plain.calc_adv_consistency_loss(data.detach(), model, init_output=io,
                                               chain_of_transforms=plain.chain_of_transforms)[0]
    finally:
        ops.set_deterministic(False)
    print("loss: replay %.9g, launch by launch %.9g; last ascent step: %.9g / %.9g"
          % (float(r1[0]), float(dist.detach()), float(inner1), float(plain.last_inner_dist.detach())))
    assert torch.equal(dist.detach(), r1[0])
    assert torch.equal(plain.last_inner_dist.reshape(-1), inner1.reshape(-1))
