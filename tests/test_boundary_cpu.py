"""distance_transform_edt / signed_distance_maps / boundary_loss of common.loss without a GPU: the public names and signatures,
the brute-force forms of tests/edt_forms.py against scipy, against plain loops and against autograd (the formulas the kernels
implement), what fp32 arithmetic reaches at the cases of tests/test_boundary_gpu.py, the host-side argument checks of the Python
layer and of the C entries, and no CPU path."""
import ctypes
import inspect
import warnings

import pytest
import torch

from tests.edt_forms import (EDT_PATTERNS, EDT_SHAPES, LOSS_SHAPES, SAMPLING, SAMPLING_TOL, boundary_closed, boundary_gradient,
                             boundary_loop, boundary_scale, edt_brute, gate_of, label_case, loss_case, loss_weights, mask_pattern,
                             omega_of, signed_maps_brute)

E = inspect.Parameter.empty


@pytest.mark.parametrize("pkg", ["advchain.common.loss", "advchain_amd.common.loss"])
def test_public_names_and_signatures(pkg):
    import importlib
    mod = importlib.import_module(pkg)

    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]

    assert params(mod.distance_transform_edt) == [("mask", E), ("sampling", None), ("squared", False)]
    assert params(mod.signed_distance_maps) == [("target", E), ("num_classes", E), ("sampling", None)]
    assert params(mod.boundary_loss) == [("input", E), ("target", None), ("weight", None), ("ignore_background", True),
                                         ("sampling", None), ("dist_maps", None)]


@pytest.mark.parametrize("sampling", [False, True], ids=["unit", "sampling"])
@pytest.mark.parametrize("shape", [(2, 9, 13), (2, 5, 7, 6)], ids=["2d", "3d"])
def test_brute_force_transform_is_scipys(shape, sampling):
    ndi = pytest.importorskip("scipy.ndimage")
    s = SAMPLING[len(shape) - 1] if sampling else None
    for name in ("fg05", "fg95", "corner", "half", "checker", "sparse"):
        m = mask_pattern(shape, name, seed=3)
        m.reshape(shape[0], -1)[:, 0] = False                    # at least one zero per entry: scipy's value is defined
        got = edt_brute(m, s)
        for b in range(shape[0]):
            want = torch.from_numpy(ndi.distance_transform_edt(m[b].numpy(), sampling=s))
            assert float((got[b] - want).abs().max()) <= 1e-12, (name, b)
        sq = edt_brute(m, s, squared=True)
        assert float((sq - got * got).abs().max()) <= 1e-9
    full = torch.ones(shape, dtype=torch.bool)
    assert bool(torch.isinf(edt_brute(full, s)).all())


def _maps_and_case(shape, seed=0):
    x, y = loss_case(shape, seed)
    return x.double(), y, signed_maps_brute(y, shape[1])


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (2, 3, 3, 4, 5), (1, 1, 4, 4)], ids=["2d", "3d", "one_class"])
def test_closed_form_agrees_with_plain_loops(shape):
    x, y, maps = _maps_and_case(shape)
    K = shape[1]
    for ign in ((False,) if K == 1 else (False, True)):
        for w in (None, loss_weights(K)):
            for tgt in (y, None):
                a = float(boundary_closed(x, tgt, weight=w, ignore_background=ign, dist_maps=maps))
                b = boundary_loop(x, maps, tgt, weight=w, ignore_background=ign)
                assert abs(a - b) <= 1e-12, (ign, w, a, b)
    if K > 1:
        assert float(boundary_closed(x, y)) == float(boundary_closed(x, y, dist_maps=maps))
        yb = y.clone()
        yb[0].reshape(-1)[2] = K
        assert torch.isnan(boundary_closed(x, yb, dist_maps=maps)) and boundary_loop(x, maps, yb) != boundary_loop(x, maps, yb)


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (2, 3, 3, 4, 5)], ids=["2d", "3d"])
def test_gradient_formula_agrees_with_autograd(shape):
    x, y, maps = _maps_and_case(shape, seed=1)
    K = shape[1]
    for ign in (False, True):
        for w in (None, loss_weights(K)):
            for tgt in (y, None):
                xr = x.clone().requires_grad_(True)
                (g,) = torch.autograd.grad(boundary_closed(xr, tgt, weight=w, ignore_background=ign, dist_maps=maps), xr)
                want = boundary_gradient(x, maps, gate_of(x, tgt), omega_of(K, w, ign, x.dtype))
                assert float((g - want).abs().max()) <= 1e-14, (ign, w)
                if tgt is not None:
                    assert float(g.movedim(1, -1)[tgt == -100].abs().max()) == 0.0


def test_degenerate_planes_are_zero_and_signs():
    for K, shape in ((1, (3, 5, 7)), (4, (3, 6, 5, 4))):
        y = label_case(K, shape, seed=5)
        maps = signed_maps_brute(y, K)
        assert float(maps[-1].abs().max()) == 0.0                  # class 0 fills the last entry, the others are absent from it
        if K == 1:
            assert float(maps[1].abs().max()) == 0.0               # the class is absent (every voxel -100)
        else:
            assert float(maps[:, K - 1].abs().max()) == 0.0        # absent everywhere
        for k in range(K):
            inside = y[0] == k
            if bool(inside.any()) and not bool(inside.all()):
                assert float(maps[0, k][inside].max()) <= -1.0 and float(maps[0, k][~inside].min()) >= 1.0


def _fp32_sampling_error(shape, name):
    s = SAMPLING[len(shape) - 1]
    m = mask_pattern(shape, name, seed=len(shape))
    want = edt_brute(m, s)
    got = edt_brute(m, s, dtype=torch.float32)
    fin = torch.isfinite(want) & (want > 0)
    assert torch.equal(torch.isfinite(got), torch.isfinite(want))
    return float(((got - want).abs()[fin] / want[fin]).max()) if bool(fin.any()) else 0.0


@pytest.mark.parametrize("shape", EDT_SHAPES, ids=["x".join(map(str, s)) for s in EDT_SHAPES])
def test_fp32_stays_a_factor_of_ten_inside_the_sampling_bound_of_the_gpu_test(shape):
    """|S (v - u)| evaluated in fp32 straight from its definition (products, squares, sums, root: one rounding each) against
    float64, at the GPU test's shapes, patterns and samplings, stays a factor of ten inside SAMPLING_TOL.  That bound is widened
    from 1e-6 to 2e-6 relative: the fp32 evaluation itself reaches 1.34e-7 at 3x36x57, 1.49e-7 at 1x70x130 and 1.44e-7 at
    2x6x10x70, because besides the roundings of the squared sum and the root's each s * delta is rounded before it is squared.
    Worst case by the roundings: (3 + 2) 2^-24 on the squared sum, half of it after the root, plus the root's own half ulp =
    2.1e-7; ten times that is the bound."""
    worst = max(_fp32_sampling_error(shape, name) for name in EDT_PATTERNS)
    print("fp32 sampling error at %s: %.3g" % (shape, worst))
    assert worst <= SAMPLING_TOL / 10


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["x".join(map(str, s)) for s in LOSS_SHAPES])
def test_fp32_closed_form_stays_a_factor_of_ten_inside_the_gpu_bounds(shape):
    """Value within 2e-6 max(|want|, S) and gradient within 1e-6 of the largest |expected|: a tenth of the GPU test's bounds."""
    K = shape[1]
    x, y = loss_case(shape, seed=K)
    maps = signed_maps_brute(y, K)
    for ign in ((False,) if K == 1 else (False, True)):
        for w in (None, loss_weights(K)):
            for tgt in (y, None):
                opt = dict(weight=w, ignore_background=ign, dist_maps=maps)
                x64 = x.double().requires_grad_(True)
                x32 = x.clone().requires_grad_(True)
                v64 = boundary_closed(x64, tgt, **opt)
                v32 = boundary_closed(x32, tgt, **opt)
                (g64,), (g32,) = torch.autograd.grad(v64, x64), torch.autograd.grad(v32, x32)
                S = boundary_scale(x.double(), tgt, weight=w, ignore_background=ign, dist_maps=maps)
                err = abs(float(v32.detach()) - float(v64.detach()))
                gerr, gmax = float((g32.double() - g64).abs().max()), float(g64.abs().max())
                print("%s ign=%s w=%s labels=%s: value err %.3g of %.3g, gradient err %.3g of %.3g"
                      % (shape, ign, w is not None, tgt is not None, err, max(abs(float(v64.detach())), S), gerr, gmax))
                assert err <= 2e-6 * max(abs(float(v64.detach())), S)
                assert gerr <= 1e-6 * gmax


def test_argument_errors_come_before_any_device_work():
    from advchain.common.loss import boundary_loss, distance_transform_edt, signed_distance_maps
    x = torch.rand(2, 4, 8, 8)
    y = torch.randint(0, 4, (2, 8, 8))
    maps = torch.rand(2, 4, 8, 8)
    m = torch.ones(2, 8, 8, dtype=torch.bool)
    for bad in ((1.0,), (1.0, 2.0, 3.0), (1.0, 0.0), (1.0, -2.0), (float("nan"), 1.0), (float("inf"), 1.0), 2.0):
        with pytest.raises(ValueError, match="sampling"):
            distance_transform_edt(m, sampling=bad)
        with pytest.raises(ValueError, match="sampling"):
            signed_distance_maps(y, 4, sampling=bad)
        with pytest.raises(ValueError, match="sampling"):
            boundary_loss(x, y, sampling=bad)
    for bad in (m[0], m[None, None, None], 3):
        with pytest.raises(ValueError):
            distance_transform_edt(bad)
    for bad in (y[0], y[None, None, None]):
        with pytest.raises(ValueError):
            signed_distance_maps(bad, 4)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="num_classes"):
            signed_distance_maps(y, bad)
    with pytest.raises(ValueError):
        boundary_loss(x[0], y[0])
    with pytest.raises(ValueError, match="ignore_background"):
        boundary_loss(x[:, :1], y)
    with pytest.raises(ValueError, match="weight"):
        boundary_loss(x, y, weight=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="weight"):
        boundary_loss(x, y, weight=torch.ones(5))
    with pytest.raises(ValueError, match="weight"):
        boundary_loss(x, y, weight=2.0)
    with pytest.raises(ValueError, match="exactly one"):
        boundary_loss(x)
    with pytest.raises(ValueError, match="exactly one"):
        boundary_loss(x, y, dist_maps=maps)
    with pytest.raises(ValueError, match="target"):
        boundary_loss(x, y[:, :4])
    with pytest.raises(ValueError, match="dist_maps"):
        boundary_loss(x, dist_maps=maps[:, :3])
    with pytest.raises(ValueError, match="sampling"):
        boundary_loss(x, dist_maps=maps, sampling=(1.0, 1.0))


def test_cpu_tensors_raise():
    from advchain.common.loss import boundary_loss, distance_transform_edt, signed_distance_maps
    from advchain_amd import _lib
    for shape in ((2, 4, 8, 8), (2, 4, 4, 8, 8)):
        x = torch.rand(shape)
        y = torch.randint(0, 4, (2,) + shape[2:])
        with pytest.raises(_lib.AdvchainHipError):
            distance_transform_edt(y > 0)
        with pytest.raises(_lib.AdvchainHipError):
            signed_distance_maps(y, 4)
        with pytest.raises(_lib.AdvchainHipError):
            boundary_loss(x, y)
        with pytest.raises(_lib.AdvchainHipError):
            boundary_loss(x, dist_maps=torch.rand(shape), ignore_background=False, weight=[1.0, 2.0, 1.0, 1.0])
    maps = torch.rand(2, 4, 8, 8, requires_grad=True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with pytest.raises(_lib.AdvchainHipError):
            boundary_loss(torch.rand(2, 4, 8, 8), dist_maps=maps)
    assert any("constant" in str(w.message) for w in seen)


def test_workspace_queries_reject_bad_sizes():
    from advchain_amd import _lib
    lib = _lib.load()
    d2, d3 = _lib.dims_array((8, 8)), _lib.dims_array((4, 8, 8))
    bad = _lib.dims_array((0, 8))
    for query in (lib.advchain_signed_maps_workspace, lib.advchain_boundary_workspace):
        assert query(2, 4, 4, d2) < 0
        assert query(2, 4, 1, d2) < 0
        assert query(2, 4, 2, bad) < 0
        assert query(2, 4, 2, None) < 0
        assert query(2, 0, 2, d2) < 0
        assert query(0, 4, 2, d2) < 0
        assert query(2, 65536, 2, d2) < 0
    assert lib.advchain_signed_maps_workspace(2, 4, 2, d2) == 2 * 4 * 2 * 64
    assert lib.advchain_signed_maps_workspace(2, 4, 3, d3) == 2 * 4 * 2 * 256
    assert lib.advchain_boundary_workspace(2, 4, 2, d2) == 2
    assert lib.advchain_boundary_workspace(2, 4, 3, d3) == 2
    assert lib.advchain_boundary_workspace(3, 4, 2, _lib.dims_array((36, 57))) == 9
    # the distance fields: an axis above 32767, a squared diagonal of 2^30 or more, a line that does not fit in LDS
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8, 32768))) < 0
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8, 32767))) > 0
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8192, 32767))) < 0          # 8191^2 + 32766^2 >= 2^30
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8193, 8))) < 0
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8192, 8))) > 0
    assert lib.advchain_signed_maps_workspace(65535, 65535, 3, _lib.dims_array((8192, 8192, 8192))) < 0


def test_c_entries_reject_bad_arguments_on_the_host():
    from advchain_amd import _lib
    lib = _lib.load()
    d2 = _lib.dims_array((8, 8))
    bad = _lib.dims_array((0, 8))
    p = ctypes.c_void_p(16)            # never dereferenced: every call below fails validation before any launch
    ok_s, neg_s, nan_s = _lib.float_array([1.5, 0.7]), _lib.float_array([1.5, -0.7]), _lib.float_array([float("nan"), 1.0])

    def edt(mask=p, kind=1, s=None, sq=0, out=p, B=2, ndim=2, dims=d2):
        return lib.advchain_edt(mask, kind, s, sq, out, B, ndim, dims, None)

    def maps(lab=p, s=None, out=p, ws=p, N=2, K=4, ndim=2, dims=d2):
        return lib.advchain_signed_maps(lab, s, out, ws, N, K, ndim, dims, None)

    def fwd(x=p, bf16=0, lab=p, m=p, ws=p, value=p, N=2, K=4, ndim=2, dims=d2, flags=0):
        return lib.advchain_boundary_fwd(x, bf16, lab, m, None, p, ws, value, N, K, ndim, dims, flags, None)

    def bwd(x=p, bf16=0, lab=None, m=p, saved=p, gx=p, N=2, K=4, ndim=2, dims=d2, flags=0):
        return lib.advchain_boundary_bwd(x, bf16, lab, m, None, saved, None, gx, N, K, ndim, dims, flags, None)

    cases = [
        (lambda: edt(mask=None), b"null"), (lambda: edt(out=None), b"null"), (lambda: edt(kind=0), b"kind"),
        (lambda: edt(kind=4), b"kind"), (lambda: edt(sq=2), b"squared"), (lambda: edt(ndim=4), b"dims"),
        (lambda: edt(ndim=1), b"dims"), (lambda: edt(dims=bad), b"dims"), (lambda: edt(dims=None), b"dims"),
        (lambda: edt(B=0), b"B"), (lambda: edt(s=neg_s), b"sampling"), (lambda: edt(s=nan_s), b"sampling"),
        (lambda: edt(s=ok_s, out=None), b"null"),
        (lambda: edt(dims=_lib.dims_array((8, 40000))), b"too large"),
        (lambda: edt(dims=_lib.dims_array((30000, 30000))), b"too large"),
        (lambda: edt(dims=_lib.dims_array((20000, 8))), b"too large"),
        (lambda: maps(lab=None), b"null"), (lambda: maps(out=None), b"null"), (lambda: maps(ws=None), b"null"),
        (lambda: maps(K=0), b"K"), (lambda: maps(K=65536), b"K"), (lambda: maps(N=0), b"N"),
        (lambda: maps(ndim=5), b"dims"), (lambda: maps(dims=bad), b"dims"), (lambda: maps(s=neg_s), b"sampling"),
        (lambda: maps(dims=_lib.dims_array((8, 40000))), b"too large"),
        (lambda: maps(dims=_lib.dims_array((9000, 8))), b"too large"),
        (lambda: fwd(x=None), b"null"), (lambda: fwd(m=None), b"null"), (lambda: fwd(ws=None), b"null"),
        (lambda: fwd(value=None), b"null"), (lambda: fwd(K=0), b"K"), (lambda: fwd(K=65536), b"K"),
        (lambda: fwd(dims=bad), b"dims"), (lambda: fwd(ndim=4), b"dims"), (lambda: fwd(N=0), b"dims"),
        (lambda: fwd(bf16=2), b"bf16"), (lambda: fwd(flags=2), b"flags"), (lambda: fwd(K=1, flags=1), b"ignore_background"),
        (lambda: bwd(x=None), b"null"), (lambda: bwd(m=None), b"null"), (lambda: bwd(saved=None), b"null"),
        (lambda: bwd(gx=None), b"null"), (lambda: bwd(K=0), b"K"), (lambda: bwd(dims=bad), b"dims"),
        (lambda: bwd(bf16=-1), b"bf16"), (lambda: bwd(flags=4), b"flags"), (lambda: bwd(K=1, flags=1), b"ignore_background"),
    ]
    for i, (call, word) in enumerate(cases):
        rc = call()
        assert rc < 0, (i, word)
        assert word in lib.advchain_last_error(), (i, word, lib.advchain_last_error())
    assert edt(dims=_lib.dims_array((8, 40000))) == -2 and maps(dims=_lib.dims_array((9000, 8))) == -2
