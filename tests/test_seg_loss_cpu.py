"""contour_loss / One_Hot / cross_entropy_2D of common.loss without a GPU: the public names and signatures, the closed forms
of tests/seg_loss_forms.py against the reference's recorded values and gradients (g12), host-side argument checks of the
C entries, and no CPU path."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests.helpers import Fixture
from tests.seg_loss_forms import ce_closed, contour_closed

NAMES = ("contour_loss", "One_Hot", "cross_entropy_2D")


@pytest.mark.parametrize("pkg", ["advchain.common.loss", "advchain_amd.common.loss"])
def test_public_names_and_signatures(pkg):
    import importlib
    mod = importlib.import_module(pkg)
    for n in NAMES:
        assert hasattr(mod, n), "%s.%s missing" % (pkg, n)
    sig = inspect.signature(mod.contour_loss)
    assert list(sig.parameters) == ["input", "target", "use_gpu", "ignore_background", "one_hot_target", "mask", "device"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["use_gpu"] is True and d["ignore_background"] is True and d["one_hot_target"] is True and d["mask"] is None
    assert d["device"] == torch.device("cuda")
    sig = inspect.signature(mod.cross_entropy_2D)
    assert list(sig.parameters) == ["input", "target", "weight", "size_average"]
    assert sig.parameters["weight"].default is None and sig.parameters["size_average"].default is True
    sig = inspect.signature(mod.One_Hot.__init__)
    assert list(sig.parameters) == ["self", "depth", "use_gpu", "device"]
    assert sig.parameters["use_gpu"].default is True and sig.parameters["device"].default == torch.device("cuda")
    assert issubclass(mod.One_Hot, torch.nn.Module)
    assert repr(mod.One_Hot(5)) == "One_Hot(5)"


G = Fixture("g12_seg_loss")
META = G.json()


def _grad_close(got, want, tol=1e-5):
    scale = max(float(np.abs(want).max()), 1e-30)
    assert float(np.abs(got - want).max()) <= tol * scale, (float(np.abs(got - want).max()), scale)


@pytest.mark.parametrize("case", META["contour"], ids=[c["name"] for c in META["contour"]])
def test_contour_closed_form_matches_reference(case):
    n = case["name"]
    x = G.t(n + "__input").double().requires_grad_(True)
    tgt = G.t(n + "__target")
    soft = not case["one_hot_target"]
    if soft:
        tgt = tgt.double().requires_grad_(True)
    mask = G.t(n + "__mask").double() if case["mask"] else None
    v = contour_closed(x, tgt, case["ignore_background"], case["one_hot_target"], mask)
    v.backward()
    v = v.detach()
    want = G.f(n + "__value")
    if n == "c2_lab_noign_softmax":
        assert abs(want) < 1e-10 and abs(float(v)) < 1e-10      # u is pure rounding with a softmax input
    else:
        assert abs(float(v) - want) <= 1e-6 * abs(want)
        _grad_close(x.grad.numpy(), G.arr(n + "__grad_input"))
        if soft:
            _grad_close(tgt.grad.numpy(), G.arr(n + "__grad_target"))


@pytest.mark.parametrize("case", META["ce"], ids=[c["name"] for c in META["ce"]])
def test_cross_entropy_closed_form_matches_reference(case):
    n = case["name"]
    x = G.t(n + "__input").double().requires_grad_(True)
    tgt = G.t(n + "__target")
    soft = tgt.dim() == 4
    if soft:
        tgt = tgt.double().requires_grad_(True)
    w = G.t(n + "__weight").double() if case["weight"] else None
    v = ce_closed(x, tgt, w, case["size_average"])
    v.backward()
    v = v.detach()
    want = G.f(n + "__value")
    assert abs(float(v) - want) <= 1e-6 * abs(want)
    _grad_close(x.grad.numpy(), G.arr(n + "__grad_input"))
    if soft:
        _grad_close(tgt.grad.numpy(), G.arr(n + "__grad_target"))


@pytest.mark.parametrize("case", META["one_hot"], ids=[c["name"] for c in META["one_hot"]])
def test_one_hot_closed_form_matches_reference(case):
    n = case["name"]
    y = G.t(n + "__labels")
    want = G.arr(n + "__out")
    got = torch.nn.functional.one_hot(y, case["depth"]).movedim(-1, 1).float()
    if got.shape[2] == 1:
        got = got.squeeze(2)
    assert got.shape == want.shape and np.array_equal(got.numpy(), want)


def test_c_entries_reject_bad_arguments_on_the_host():
    from advchain_amd import _lib
    lib = _lib.load()
    dims2 = _lib.dims_array((8, 8))
    dims3 = _lib.dims_array((4, 8, 8))
    p = ctypes.c_void_p(16)            # never dereferenced: every call below fails validation before any launch
    # workspace query: bad sizes -> -1
    assert lib.advchain_seg_loss_workspace(2, 4, dims2) < 0
    assert lib.advchain_seg_loss_workspace(2, 2, _lib.dims_array((0, 8))) < 0
    assert lib.advchain_seg_loss_workspace(2, 2, dims2) > 0
    cases = [
        (lambda: lib.advchain_ce2d_fwd(None, 0, p, None, None, None, p, p, 2, 4, dims2, 1.0, None), b"null"),
        (lambda: lib.advchain_ce2d_fwd(p, 0, p, p, None, None, p, p, 2, 4, dims2, 1.0, None), b"exactly one"),
        (lambda: lib.advchain_ce2d_fwd(p, 0, p, None, None, None, p, p, 2, 0, dims2, 1.0, None), b"K"),
        (lambda: lib.advchain_ce2d_fwd(p, 0, p, None, None, None, p, p, 2, 4, _lib.dims_array((0, 8)), 1.0, None), b"dims"),
        (lambda: lib.advchain_ce2d_fwd(p, 2, p, None, None, None, p, p, 2, 4, dims2, 1.0, None), b"bf16"),
        (lambda: lib.advchain_ce2d_bwd(p, 0, p, None, None, None, None, p, None, 2, 4, dims2, 1.0, None), b"null"),
        (lambda: lib.advchain_ce2d_bwd(p, 0, p, None, None, p, None, None, None, 2, 4, dims2, 1.0, None), b"null"),
        (lambda: lib.advchain_ce2d_bwd(p, 0, p, None, None, p, None, p, p, 2, 4, dims2, 1.0, None), b"label"),
        (lambda: lib.advchain_ce2d_bwd(p, 0, p, None, None, p, None, p, None, 2, -3, dims2, 1.0, None), b"K"),
        (lambda: lib.advchain_contour_fwd(None, p, None, None, None, p, p, 2, 4, 2, dims2, 1, 1, None), b"null"),
        (lambda: lib.advchain_contour_fwd(p, None, None, None, None, p, p, 2, 4, 2, dims2, 1, 1, None), b"exactly one"),
        (lambda: lib.advchain_contour_fwd(p, p, None, None, None, p, p, 2, 0, 2, dims2, 1, 1, None), b"K"),
        (lambda: lib.advchain_contour_fwd(p, p, None, None, None, p, p, 2, 1, 2, dims2, 1, 1, None), b"object class"),
        (lambda: lib.advchain_contour_fwd(p, p, None, None, None, p, p, 2, 4, 4, dims2, 1, 1, None), b"dims"),
        (lambda: lib.advchain_contour_fwd(p, p, None, None, None, p, p, 2, 4, 3, dims2, 1, 1, None), b"dims"),
        (lambda: lib.advchain_contour_fwd(p, p, None, p, None, p, p, 2, 4, 2, dims2, 1, 2, None), b"mask"),
        (lambda: lib.advchain_contour_bwd(None, None, p, None, 2, 4, 3, dims3, 1, None), b"null"),
        (lambda: lib.advchain_contour_bwd(p, None, None, None, 2, 4, 3, dims3, 1, None), b"null"),
        (lambda: lib.advchain_contour_bwd(p, None, p, None, 2, 0, 3, dims3, 1, None), b"K"),
        (lambda: lib.advchain_one_hot(None, p, 2, 4, 16, None), b"null"),
        (lambda: lib.advchain_one_hot(p, p, 2, 0, 16, None), b"depth"),
    ]
    for call, word in cases:
        rc = call()
        assert rc < 0, word
        assert word in lib.advchain_last_error(), (word, lib.advchain_last_error())


def test_cpu_tensors_raise():
    from advchain.common.loss import One_Hot, contour_loss, cross_entropy_2D
    from advchain_amd import _lib
    x = torch.rand(2, 4, 8, 8)
    y = torch.randint(0, 4, (2, 8, 8))
    with pytest.raises(_lib.AdvchainHipError):
        cross_entropy_2D(x, y)
    with pytest.raises(_lib.AdvchainHipError):
        cross_entropy_2D(x, torch.softmax(x, 1), weight=[1.0, 2.0, 1.0, 1.0])
    with pytest.raises(_lib.AdvchainHipError):
        contour_loss(torch.softmax(x, 1), y, use_gpu=False, device=torch.device("cpu"))
    with pytest.raises(_lib.AdvchainHipError):
        contour_loss(torch.rand(2, 4, 4, 8, 8), torch.rand(2, 4, 4, 8, 8), one_hot_target=False)
    with pytest.raises(_lib.AdvchainHipError):
        One_Hot(4, use_gpu=False)(y)
