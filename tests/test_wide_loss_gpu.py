"""The consistency loss for a run-time class count (the fp32 kernels of csrc/loss_lp.hip, taken from ops.WIDE_LOSS_MIN_K = 17
classes on) and the solver with a 20-class model.

Tolerances are those of tests/test_ops_gpu.py::test_kl_term_in_every_kernel_variant: value 1e-7 + 2e-5 |v|, gradient 2e-5 of its
maximum + 1e-10, against the CPU oracle in fp32 (whose own fp32-against-float64 spread at these class counts is 2.5e-7 / 6.9e-7:
a factor of 30 is left to the kernels)."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import make_model, maxdiff, rand, smooth_data

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

MIXES = ((["kl"], [1.0]), (["kl", "contour"], [1.0, 0.5]), (["mse", "kl", "contour"], [0.7, 1.3, 0.5]))
MASKS = ("none", "one", "perclass", "one_gt")

# every shape with at least two K, every K with at least two shapes of each rank, K = 105 on small shapes only
PARITY = [
    ((12, 64), 17), ((12, 64), 64), ((11, 20), 20), ((11, 20), 105), ((37, 52), 17), ((37, 52), 33), ((6, 252), 20),
    ((6, 252), 33), ((64, 256), 17), ((64, 256), 20), ((5, 8), 64), ((5, 8), 105), ((1, 7), 33), ((1, 7), 105),
    ((5, 6, 64), 17), ((5, 6, 64), 33), ((7, 9, 80), 20), ((7, 9, 80), 64), ((3, 5, 7), 64), ((3, 5, 7), 105),
    ((19, 40, 128), 17), ((19, 40, 128), 20), ((2, 3, 8), 33), ((2, 3, 8), 105), ((1, 1, 5), 20), ((1, 1, 5), 105),
]


def _operands(K, dims, N=2):
    pred = rand((N, K) + dims, 311) * 3
    ref = rand((N, K) + dims, 312) * 3
    mk = (rand((N, K) + dims, 313) > -0.6).float()
    onehot = F.one_hot(ref.argmax(1), K).movedim(-1, 1).float().contiguous()
    return pred, ref, mk, onehot


def _case(mode, ref, mk, onehot):
    """(reference, mask, is_gt) of one mask mode."""
    if mode == "none":
        return ref, None, False
    if mode == "one":
        return ref, mk[:, :1].contiguous(), False
    if mode == "perclass":
        return ref, mk, False
    return onehot, mk[:, :1].contiguous(), True


def _oracle(pred, r, types, weights, mask, is_gt):
    from oracle import advchain_oracle as O
    a = pred.clone().requires_grad_(True)
    v = O.consistency_loss(a, r, types, weights, mask=mask, is_gt=is_gt)
    v.backward()
    return float(v.detach()), a.grad


def _product(pred, r, types, weights, mask, is_gt, scale=1.0):
    from advchain_amd.common.loss import calc_segmentation_consistency
    b = pred.to(DEV).requires_grad_(True)
    v = calc_segmentation_consistency(b, r.to(DEV), types, weights, scales=[0], mask=None if mask is None else mask.to(DEV),
                                      is_gt=is_gt)
    (scale * v).backward()
    return float(v.detach()), b.grad.cpu()


def _check(got, want, tag):
    v, g = got
    v_ref, g_ref = want
    ev, eg = abs(v - v_ref), maxdiff(g, g_ref)
    print("%s: value err %.3e (|v| %.3e), grad err %.3e (max %.3e)" % (tag, ev, abs(v_ref), eg, float(g_ref.abs().max())))
    assert ev < 1e-7 + 2e-5 * abs(v_ref), tag
    assert eg < 2e-5 * float(g_ref.abs().max()) + 1e-10, tag


@pytest.mark.parametrize("dims,K", PARITY)
def test_wide_loss_matches_the_oracle(dims, K):
    """Every term mix x (no mask, one-channel mask, K-channel mask with distinct channels, one-channel mask with is_gt), on
    shapes that reach whole and partial tiles along every axis, rows below / at / above a tile, and single-row volumes."""
    from advchain_amd import ops
    assert K >= ops.WIDE_LOSS_MIN_K
    pred, ref, mk, onehot = _operands(K, dims)
    for types, weights in MIXES:
        for mode in MASKS:
            r, mask, is_gt = _case(mode, ref, mk, onehot)
            _check(_product(pred, r, types, weights, mask, is_gt), _oracle(pred, r, types, weights, mask, is_gt),
                   (dims, K, types, mode))


@pytest.mark.parametrize("dims", [(12, 64), (37, 52), (7, 9, 80), (3, 5, 7)])
@pytest.mark.parametrize("K", [2, 4, 5, 8, 16])
def test_wide_and_register_kernels_agree_below_17_classes(dims, K):
    """ops.WIDE_LOSS_MIN_K = 2 routes K <= 16 through the run-time-K kernels: against the default path and the oracle."""
    from advchain_amd import ops
    pred, ref, mk, onehot = _operands(K, dims)
    for types, weights in MIXES + ((["mse", "contour"], [1.0, 0.5]),):
        for mode in MASKS:
            r, mask, is_gt = _case(mode, ref, mk, onehot)
            want = _oracle(pred, r, types, weights, mask, is_gt)
            default = _product(pred, r, types, weights, mask, is_gt)
            assert ops.WIDE_LOSS_MIN_K == 17
            ops.WIDE_LOSS_MIN_K = 2
            try:
                wide = _product(pred, r, types, weights, mask, is_gt)
            finally:
                ops.WIDE_LOSS_MIN_K = 17
            tag = (dims, K, types, mode)
            _check(default, want, tag + ("default",))
            _check(wide, want, tag + ("wide",))
            _check(wide, default, tag + ("wide vs default",))


def _outcome(fn):
    try:
        return ("ok",) + tuple(fn())
    except Exception as e:          # noqa: BLE001  (the point is to compare what the two paths raise)
        return ("raised", type(e).__name__)


def test_empty_batch_behaves_as_on_the_register_path():
    """N = 0 through the operator: whatever the K <= 16 path makes of it (a value of 0 and an empty gradient, or its error
    for the null pointers of empty tensors), the wide path makes the same of it."""
    from advchain_amd import ops

    def run(K):
        p = torch.zeros((0, K, 8, 8), device=DEV, requires_grad=True)
        v, _ = ops.consistency_sums(p, torch.zeros((0, K, 8, 8), device=DEV), None, [1.0, 0.5, 0.5, 1.0])
        v.backward()
        return float(v.detach()), tuple(p.grad.shape[1:])
    narrow = _outcome(lambda: run(4))
    ops.WIDE_LOSS_MIN_K = 2
    try:
        wide4 = _outcome(lambda: run(4))
    finally:
        ops.WIDE_LOSS_MIN_K = 17
    wide20 = _outcome(lambda: run(20))
    assert wide4 == narrow, (wide4, narrow)
    assert wide20[:2] == narrow[:2] and (narrow[0] == "raised" or wide20[2] == (20, 8, 8)), (wide20, narrow)


@pytest.mark.parametrize("dims", [(9, 20), (4, 6, 10)])
def test_one_class_through_the_wide_path(dims):
    """K = 1: softmax is 1 everywhere, there is no object class for 'contour'; as on the default path."""
    from advchain_amd import ops
    pred, ref, mk, onehot = _operands(1, dims)
    for types, weights in MIXES:
        want = _oracle(pred, ref, types, weights, mk, False)
        default = _product(pred, ref, types, weights, mk, False)
        ops.WIDE_LOSS_MIN_K = 1
        try:
            wide = _product(pred, ref, types, weights, mk, False)
        finally:
            ops.WIDE_LOSS_MIN_K = 17
        _check(default, want, (dims, types, "default"))
        _check(wide, want, (dims, types, "wide"))
        assert torch.isfinite(wide[1]).all()


def off_by_4(t):
    """A contiguous device copy of `t` that starts 4 bytes off a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("dims", [(11, 20), (5, 6, 18)])
def test_views_and_misaligned_tensors(dims):
    """A non-contiguous view (`x[..., 1:]`), its contiguous copy and a contiguous tensor that starts 4 bytes off a 16-byte
    boundary give the same result (the 16-byte loads are taken for aligned tensors only)."""
    from advchain_amd.common.loss import calc_segmentation_consistency
    K = 20
    pred, ref, mk, _ = _operands(K, dims[:-1] + (dims[-1] + 1,))
    mk = mk[:, :1]
    types, weights = ["mse", "kl", "contour"], [0.7, 1.3, 0.5]
    sl = (Ellipsis, slice(1, None))
    pc, rc, mc = pred[sl].contiguous(), ref[sl].contiguous(), mk[sl].contiguous()
    want = _oracle(pc, rc, types, weights, mc, False)

    def loss(p, r, m):
        v = calc_segmentation_consistency(p, r, types, weights, scales=[0], mask=m)
        v.backward()
        return float(v.detach())

    b = pc.to(DEV).requires_grad_(True)
    copy = (loss(b, rc.to(DEV), mc.to(DEV)), b.grad.cpu())
    B = pred.to(DEV).requires_grad_(True)
    view = (loss(B[sl], ref.to(DEV)[sl], mk.to(DEV)[sl]), B.grad[sl].cpu())
    assert float(B.grad[..., 0].abs().max()) == 0.0
    o = off_by_4(pc).requires_grad_(True)
    off = (loss(o, off_by_4(rc), off_by_4(mc)), o.grad.cpu())
    _check(copy, want, (dims, "contiguous"))
    _check(view, want, (dims, "view"))
    _check(off, want, (dims, "misaligned"))
    assert torch.equal(view[1], copy[1]) and abs(view[0] - copy[0]) <= 1e-6 * abs(copy[0])
    assert torch.equal(off[1], copy[1])      # (one gradient kernel for both; the statistics pass differs in its load width only)


@pytest.mark.parametrize("dims", [(11, 20), (5, 6, 18)])
def test_deterministic_value_does_not_depend_on_alignment(dims):
    """Deterministic mode, fp32, K = 20: the value and both gradients from 16-byte aligned operands are equal, bit for bit, to
    those from copies that start 4 bytes off a 16-byte boundary -- a lane of the statistics pass owns the same 4 voxels with
    16-byte loads and with scalar ones, so every sum has one order."""
    from advchain_amd import ops
    from advchain_amd.common.loss import calc_segmentation_consistency
    pred, ref, mk, _ = _operands(20, dims)
    mk = mk[:, :1].contiguous()
    types, weights = ["mse", "kl", "contour"], [0.7, 1.3, 0.5]

    def run(place):
        a, b, m = place(pred).requires_grad_(True), place(ref).requires_grad_(True), place(mk)
        v = calc_segmentation_consistency(a, b, types, weights, scales=[0], mask=m)
        v.backward()
        return v.detach().clone(), a.grad.clone(), b.grad.clone()

    def aligned(t):
        out = t.to(DEV)
        assert out.data_ptr() % 16 == 0 and out.is_contiguous()
        return out
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        want, got = run(aligned), run(off_by_4)
    finally:
        ops.set_deterministic(was)
    print("%s: value %.9g (aligned) %.9g (4 bytes off)" % (dims, float(want[0]), float(got[0])))
    assert float(want[1].abs().max()) > 0 and float(want[2].abs().max()) > 0
    for w, g, what in zip(want, got, ("value", "prediction.grad", "reference.grad")):
        assert torch.equal(w, g), (dims, what)


def test_grad_scale():
    pred, ref, mk, _ = _operands(20, (13, 30))
    types, weights = ["mse", "kl", "contour"], [0.7, 1.3, 0.5]
    one = _product(pred, ref, types, weights, mk, False)
    three = _product(pred, ref, types, weights, mk, False, scale=3.0)
    v_ref, g_ref = _oracle(pred, ref, types, weights, mk, False)
    _check((three[0], three[1] / 3.0), (v_ref, g_ref), "grad_scale 3")
    assert maxdiff(three[1], 3.0 * one[1]) < 1e-6 * float(one[1].abs().max()) * 3


@pytest.mark.parametrize("dims", [(37, 52), (7, 9, 80)])
def test_gradient_is_bit_reproducible(dims):
    pred, ref, mk, _ = _operands(20, dims)
    types, weights = ["mse", "kl", "contour"], [0.7, 1.3, 0.5]
    for mask in (mk[:, :1].contiguous(), mk):
        a = _product(pred, ref, types, weights, mask, False)
        b = _product(pred, ref, types, weights, mask, False)
        assert torch.equal(a[1], b[1])
        assert abs(a[0] - b[0]) <= 1e-6 * abs(a[0])      # (the value goes through float-atomic slots: last bits are free)


def test_peak_memory_has_no_room_for_P_and_D():
    """One forward + backward at 2 x 64 x 64 x 64 x 32 (N, K, D, H, W): what the evaluation allocates stays below pred + grad_pred +
    what the design saves (statistics 16 bytes per voxel, R 8 (K - 1) bytes per voxel) + 16 MiB, and below what it would
    need if P and D (8 K bytes per voxel) existed as well."""
    from advchain_amd import ops
    N, K, dims = 2, 64, (64, 64, 32)
    V = dims[0] * dims[1] * dims[2]
    g = torch.Generator(device="cpu").manual_seed(5)
    pred = (torch.rand((N, K) + dims, generator=g) * 6 - 3).to(DEV).requires_grad_(True)
    ref = (torch.rand((N, K) + dims, generator=g) * 6 - 3).to(DEV)
    mask = torch.ones((N, 1) + dims, device=DEV)
    coef = [1e-9, 1e-6, 1e-6, 1e-6]
    v, _ = ops.consistency_sums(pred.detach()[:1, :, :2].contiguous().requires_grad_(True), ref[:1, :, :2].contiguous(), None, coef)
    v.backward()                                         # (persistent accumulators and the library exist before the measurement)
    del v
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    v, _ = ops.consistency_sums(pred, ref, mask, coef)
    v.backward()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    tensor = 4 * N * K * V
    saved = 16 * N * V + 8 * (K - 1) * N * V
    bound = 2 * tensor + saved + (16 << 20)
    with_pd = tensor + saved + 2 * tensor                # grad_pred + statistics + R + P + D
    print("allocated by the evaluation %.1f MiB; bound %.1f MiB; with P and D %.1f MiB; grad_pred + saved %.1f MiB"
          % (used / 2.0 ** 20, bound / 2.0 ** 20, with_pd / 2.0 ** 20, (tensor + saved) / 2.0 ** 20))
    assert used < bound and used < with_pd
    assert torch.isfinite(pred.grad).all()


# ---- the solver with a 20-class model ---------------------------------------------------------------------------------------

def _one_step_vs_oracle(sd, N, dims, names, k, deterministic=None, seed=11):
    """tests/test_fullsize_gpu.py::_one_step_vs_oracle with the class count of the model as a parameter: one whole
    adversarial_training call (one ascent step + the final consistency pass), same initial parameters on both sides.
    Tolerances: 1e-4 (scale-relative), widened ONLY by what the oracle itself moves when its own deformation fields are
    jittered by the measured GPU-vs-oracle field difference.  Returns the product's parameters and loss and the allowances."""
    from oracle import advchain_oracle as O
    from advchain_amd.augmentor import AdvAffine, AdvBias, AdvMorph, AdvNoise, ComposeAdversarialTransformSolver
    import bench
    specs = bench.transform_configs(dims, N, names)
    data = smooth_data(N, 1, dims, seed)
    ocls = {"noise": O.OracleNoise, "bias": O.OracleBias, "morph": O.OracleMorph, "affine": O.OracleAffine}
    gcls = {"noise": AdvNoise, "bias": AdvBias, "morph": AdvMorph, "affine": AdvAffine}
    gchain = [gcls[nm](spatial_dims=sd, config_dict=cfg, device=DEV) for nm, cfg in specs]
    init = []
    for i, (nm, cfg) in enumerate(specs):
        o = ocls[nm](sd, cfg)
        o.init_parameters()
        shape = tuple(o.param.shape)
        if nm == "bias":
            p = 0.1 * rand(shape, 200 + i)
        elif nm == "affine":
            p = 0.6 * rand(shape, 200 + i)
        else:
            p = O.unit_normalize(rand(shape, 200 + i))
        init.append(p)

    def oracle_run(hook):
        chain = [ocls[nm](sd, cfg) for nm, cfg in specs]
        for o, p in zip(chain, init):
            o.init_parameters()
            o.param = p.clone()
            if o.get_name() == "morph":
                o.field_hook = hook
        solver = O.OracleSolver(chain)
        loss = solver.adversarial_training(data=data, model=make_model(sd, k=k), n_iter=1, lazy_load=True, step_sizes=1)
        return solver, chain, float(loss)
    osolver, ochain, oloss = oracle_run(None)
    for g, p in zip(gchain, init):
        g.init_parameters()
        g.set_parameters(p.to(DEV))
    dq = 0.0
    for o, g in zip(ochain, gchain):
        if g.get_name() == "morph":
            with torch.no_grad():
                om = ocls["morph"](sd, o.config_dict)
                om.init_parameters()
                om.param = init[gchain.index(g)].clone()
                dq = max(dq, maxdiff(torch.clamp(g._field(1.0), -1, 1).cpu(), om._field(1)),
                         maxdiff(torch.clamp(g._field(-1.0), -1, 1).cpu(), om._field(-1)))
    assert dq < 2e-5, dq
    gsolver = ComposeAdversarialTransformSolver(chain_of_transforms=gchain, deterministic=deterministic)
    try:
        gloss = gsolver.adversarial_training(data=data.to(DEV), model=make_model(sd, k=k, device=DEV), n_iter=1, lazy_load=True,
                                             step_sizes=1)
    finally:
        if deterministic:
            from advchain_amd import ops
            ops.set_deterministic(False)
    d0 = osolver.trace[0]["dist"]
    assert abs(float(gsolver.last_inner_dist) - d0) < 1e-7 + 1e-4 * abs(d0)
    spread_p, spread_l = [0.0] * len(specs), 0.0
    if dq > 0:
        for trial in range(2):
            _, jchain, jloss = oracle_run(O.uniform_jitter(dq, seed=trial))
            for i, (o, j) in enumerate(zip(ochain, jchain)):
                spread_p[i] = max(spread_p[i], maxdiff(o.param.detach(), j.param.detach()))
            spread_l = max(spread_l, abs(jloss - oloss))
    allowed_p = []
    for i, (nm_cfg, o, g) in enumerate(zip(specs, ochain, gchain)):
        ref = o.param.detach()
        allowed = max(1e-4 * max(1.0, float(ref.abs().max())), 3.0 * spread_p[i])
        allowed_p.append(allowed)
        err = float((g.param.detach().cpu() - ref).abs().max())
        print("%s: err %.2e allowed %.2e (oracle spread %.2e at field diff %.2e)" % (nm_cfg[0], err, allowed, spread_p[i], dq))
        assert err < allowed, (nm_cfg[0], "err %.2e allowed %.2e (oracle spread %.2e at field diff %.2e)"
                               % (err, allowed, spread_p[i], dq))
    allowed_l = max(1e-6 + 1e-4 * abs(oloss), 3.0 * spread_l)
    assert abs(float(gloss) - oloss) < allowed_l, (float(gloss), oloss, allowed_l, dq)
    return [g.param.detach().cpu() for g in gchain], float(gloss), allowed_p, allowed_l


SOLVER_CASES = {2: (2, (128, 128), ["noise", "bias", "morph", "affine"]), 3: (1, (32, 32, 16), ["bias", "morph", "affine"])}


@pytest.mark.parametrize("sd", [2, 3])
def test_one_ascent_step_with_a_20_class_model_matches_the_oracle(sd):
    N, dims, names = SOLVER_CASES[sd]
    _one_step_vs_oracle(sd, N, dims, names, k=20)


@pytest.mark.parametrize("sd", [2, 3])
def test_deterministic_mode_with_a_20_class_model(sd):
    """deterministic=True runs at K = 20 and agrees with the default mode (and the oracle) within the bounds above.  Equal
    bits are not asked for: the warps of a 20-channel prediction take the float-atomic general route (bit-reproducibility
    covers warps of at most four channels); the loss operator on its own is bit-reproducible (test above)."""
    N, dims, names = SOLVER_CASES[sd]
    p0, l0, allowed_p, allowed_l = _one_step_vs_oracle(sd, N, dims, names, k=20)
    p1, l1, _, _ = _one_step_vs_oracle(sd, N, dims, names, k=20, deterministic=True)
    for a, b, allowed in zip(p0, p1, allowed_p):
        assert maxdiff(a, b) < allowed
    assert abs(l0 - l1) < allowed_l


def _graph_solver(dims, names, N, graph):
    import bench
    from advchain_amd.augmentor import AdvAffine, AdvBias, AdvMorph, AdvNoise, ComposeAdversarialTransformSolver
    cls = {"noise": AdvNoise, "bias": AdvBias, "morph": AdvMorph, "affine": AdvAffine}
    chain = [cls[nm](spatial_dims=len(dims), config_dict=cfg, device=DEV) for nm, cfg in bench.transform_configs(dims, N, names)]
    return ComposeAdversarialTransformSolver(chain_of_transforms=chain, divergence_types=["mse", "contour"],
                                             divergence_weights=[1.0, 0.5], hip_graph=graph)


def _graph_call(solver, data, model, n_iter, seed):
    torch.manual_seed(seed)
    loss = solver.adversarial_training(data=data, model=model, n_iter=n_iter, lazy_load=False, step_sizes=1, power_iteration=False)
    return ([loss.detach().clone(), solver.adv_data.clone(), solver.warped_back_adv_output.detach().clone(),
             solver.init_output.clone()] + [t.param.detach().clone() for t in solver.chain_of_transforms])


def test_the_ascent_loop_with_a_20_class_model_replays_from_a_graph():
    """K = 20, 2D 4 x 1 x 128 x 128, full chain.  n_iter = 2: after the three recorded calls the loop is captured and every later
    call is a replay, none of them violated, in 20 calls.  One-step calls (where a replay and the ordinary path from the same
    initial parameters can be compared before a free-running ascent amplifies their difference): within 1e-4 of scale, the
    bound of tests/test_graph_gpu.py.  torch.equal is not asked for: the 20-channel warp backward uses float atomics."""
    dims, names, N = (128, 128), ["noise", "bias", "morph", "affine"], 4
    model = make_model(2, k=20, device=DEV)
    graph = _graph_solver(dims, names, N, True)
    for k in range(20):
        out = _graph_call(graph, smooth_data(N, 1, dims, 60 + k).to(DEV), model, 2, 300 + k)
        assert all(torch.isfinite(t).all() for t in out)
    st = graph.graph_stats
    print("n_iter=2:", st)
    assert st["violations"] == 0 and st["refused"] == 0 and st["captures"] == 1 and st["recorded"] == 3 and st["replays"] >= 16, st
    eager, graph1 = _graph_solver(dims, names, N, False), _graph_solver(dims, names, N, True)
    for k in range(6):
        data = smooth_data(N, 1, dims, 40 + k).to(DEV)
        want = _graph_call(eager, data, model, 1, 100 + k)
        got = _graph_call(graph1, data, model, 1, 100 + k)
        for i, (x, y) in enumerate(zip(got, want)):
            scale = max(1e-6, float(y.abs().max()))
            err = float((x - y).abs().max())
            print("call %d output %d: err %.2e of scale %.2e" % (k, i, err, scale))
            assert err <= 1e-4 * scale + 1e-7, (k, i, err, scale)
    st = graph1.graph_stats
    assert st["recorded"] == 3 + st["violations"] and st["captures"] >= 1 and st["replays"] >= 2 and st["refused"] == 0, st
