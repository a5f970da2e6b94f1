"""The consistency loss and the solver with more than 16 classes, as far as a machine without a GPU can check them: the
host side (normalisers, no class cap, solver control flow) against the oracle through the TEST-ONLY operator backend, and
the host-side argument checks of the two C entries of csrc/loss_lp.hip (no launch)."""
import contextlib
import ctypes
import io

import pytest
import torch

from oracle import advchain_oracle as O
from tests import cpu_backend
from tests.helpers import make_model, maxdiff, rand, smooth_data

CPU = torch.device("cpu")


@pytest.fixture
def cpu_ops(monkeypatch):
    cpu_backend.install(monkeypatch)
    yield


@pytest.mark.parametrize("dims", [(9, 14), (4, 5, 6)])
@pytest.mark.parametrize("K", [20, 40])
def test_consistency_and_kl_above_16_classes_match_the_oracle(cpu_ops, K, dims):
    from advchain_amd.common.loss import calc_segmentation_consistency, kl_divergence
    pred = rand((2, K) + dims, 811) * 3
    ref = rand((2, K) + dims, 812) * 3
    mk = (rand((2, 1) + dims, 813) > -0.6).float()
    for types, weights in ((["mse", "contour"], [1.0, 0.5]), (["kl", "contour"], [1.0, 0.5]), (["mse", "kl", "contour"], [0.7, 1.3, 0.5])):
        for mask in (None, mk):
            a = pred.clone().requires_grad_(True)
            v_ref = O.consistency_loss(a, ref, types, weights, mask=mask)
            v_ref.backward()
            b = pred.clone().requires_grad_(True)
            v = calc_segmentation_consistency(b, ref, types, weights, scales=[0], mask=mask)
            v.backward()
            assert abs(float(v) - float(v_ref)) < 1e-7 + 2e-5 * abs(float(v_ref)), (types, mask is not None)
            assert maxdiff(b.grad, a.grad) < 2e-5 * float(a.grad.abs().max()) + 1e-10, (types, mask is not None)
    a = pred.clone().requires_grad_(True)
    v_ref = O.consistency_loss(a, ref, ["kl"], [1.0])
    v_ref.backward()
    b = pred.clone().requires_grad_(True)
    v = kl_divergence(ref, b)
    v.backward()
    assert abs(float(v) - float(v_ref)) < 1e-7 + 2e-5 * abs(float(v_ref))
    assert maxdiff(b.grad, a.grad) < 2e-5 * float(a.grad.abs().max()) + 1e-10


def test_one_solver_call_with_a_20_class_model_matches_the_oracle(cpu_ops):
    from advchain_amd.augmentor import AdvBias, AdvNoise, ComposeAdversarialTransformSolver
    ds = [2, 1, 32, 32]
    specs = [("noise", dict(epsilon=1.0, xi=1e-6, data_size=ds)),
             ("bias", dict(epsilon=0.3, control_point_spacing=[16, 16], downscale=2, data_size=ds, interpolation_order=3,
                           init_mode="random", space="log"))]
    ocls = {"noise": O.OracleNoise, "bias": O.OracleBias}
    gcls = {"noise": AdvNoise, "bias": AdvBias}
    data = smooth_data(2, 1, (32, 32), 17)
    ochain = [ocls[nm](2, cfg) for nm, cfg in specs]
    gchain = [gcls[nm](spatial_dims=2, config_dict=cfg, device=CPU) for nm, cfg in specs]
    for i, (o, g) in enumerate(zip(ochain, gchain)):
        o.init_parameters()
        p = 0.1 * rand(tuple(o.param.shape), 300 + i) if o.get_name() == "bias" else O.unit_normalize(rand(tuple(o.param.shape), 300 + i))
        o.param = p.clone()
        g.init_parameters()
        g.set_parameters(p.clone())
    osolver = O.OracleSolver(ochain)
    gsolver = ComposeAdversarialTransformSolver(chain_of_transforms=gchain)
    with contextlib.redirect_stdout(io.StringIO()):
        oloss = float(osolver.adversarial_training(data=data, model=make_model(2, k=20), n_iter=1, lazy_load=True))
        gloss = float(gsolver.adversarial_training(data=data, model=make_model(2, k=20), n_iter=1, lazy_load=True))
    assert oloss == oloss and abs(oloss) < float("inf") and gloss == gloss and abs(gloss) < float("inf")
    assert abs(gloss - oloss) < 1e-6 + 1e-4 * abs(oloss), (gloss, oloss)
    for o, g in zip(ochain, gchain):
        assert maxdiff(g.param.detach(), o.param.detach()) < 1e-4, o.get_name()


def test_a_cpu_tensor_is_refused_by_the_operator_not_by_a_class_cap():
    from advchain_amd import _lib
    from advchain_amd.common.loss import calc_segmentation_consistency
    with pytest.raises(_lib.AdvchainHipError):
        calc_segmentation_consistency(torch.zeros(1, 20, 8, 8), torch.zeros(1, 20, 8, 8), ["mse", "contour"], [1.0, 0.5])


def test_class_count_beyond_the_c_abi_names_the_number(cpu_ops):
    from advchain_amd.common.loss import calc_segmentation_consistency
    x = torch.zeros(1, 65536, 1, 2)
    with pytest.raises(NotImplementedError, match="65536"):
        calc_segmentation_consistency(x, x, ["mse"], [1.0])


def test_wide_entries_check_their_arguments_on_the_host():
    """Null pointers and K = 0: a negative code and a message that names the entry; nothing is launched."""
    from advchain_amd import _lib
    lib = _lib.load()
    dims = _lib.dims_array((4, 8))
    buf = (ctypes.c_float * 4096)()          # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    last = lib.advchain_last_error
    last.restype = ctypes.c_char_p

    def fwd(pred=p, ref=p, stats=p, sums=p, K=20):
        return lib.advchain_consistency_wide_fwd(pred, ref, None, stats, None, sums, 1, K, 2, dims, 1, 0, 1, 0, None)

    def bwd(pred=p, ref=p, stats=p, gpred=p, K=20):
        return lib.advchain_consistency_wide_bwd(pred, ref, stats, None, None, None, gpred, 1.0, 0.0, 0.0, 0.0, 0, 1, K, 2, dims,
                                                 1, None)
    for call, name in ((fwd, b"consistency_wide_fwd"), (bwd, b"consistency_wide_bwd")):
        for kw in (dict(pred=None), dict(ref=None), dict(stats=None), dict(K=0), dict(K=65536)):
            assert call(**kw) < 0, (name, kw)
            assert name in last(), (name, kw, last())
    assert fwd(sums=None) < 0 and b"consistency_wide_fwd" in last()
    assert bwd(gpred=None) < 0 and b"consistency_wide_bwd" in last()
    # a bad mask channel count and a bad rank
    assert lib.advchain_consistency_wide_fwd(p, p, p, p, None, p, 1, 20, 2, dims, 3, 0, 1, 0, None) < 0
    assert lib.advchain_consistency_wide_fwd(p, p, None, p, None, p, 1, 20, 4, dims, 1, 0, 1, 0, None) < 0
    # an empty batch is fine and launches nothing
    assert lib.advchain_consistency_wide_fwd(p, p, None, p, None, p, 0, 20, 2, dims, 1, 0, 1, 0, None) == 0
    assert lib.advchain_consistency_wide_bwd(p, p, p, None, None, None, p, 1.0, 0.0, 0.0, 0.0, 0, 0, 20, 2, dims, 1, None) == 0


def test_the_switch_defaults_to_17():
    from advchain_amd import ops
    assert ops.WIDE_LOSS_MIN_K == 17
