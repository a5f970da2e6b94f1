"""3D differences, Jacobian determinant and folding statistics without a GPU: the public names, the argument errors, the
host-side validation of the C entries, and the float64 closed forms of tests/jacobian_forms.py checked against algebra."""
import ctypes

import pytest
import torch

from tests import jacobian_forms as F

NEW = ("calculate_image_diff3D", "calculate_jacobian_determinant3D", "jacobian_folding_stats")


def test_names_are_public():
    import advchain.augmentor
    import advchain_amd.augmentor
    from advchain.augmentor import adv_morph
    from advchain_amd import ops
    for mod in (advchain.augmentor, advchain_amd.augmentor, adv_morph):
        for n in NEW:
            assert callable(getattr(mod, n)), (mod.__name__, n)
    for n in NEW:
        assert n in advchain_amd.augmentor.__all__
    from advchain.augmentor import AdvMorph
    assert callable(AdvMorph.jacobian_determinant) and callable(AdvMorph.folding_stats)
    for n in ("image_diff3d", "jacobian_det", "jacobian_stats"):
        assert callable(getattr(ops, n))
    assert ops.JACOBIAN_COLS == 62 and 2 <= ops.JACOBIAN_ROWS_MIN <= ops.JACOBIAN_ROWS_MAX
    assert ops.JacobianStats._fields == ("neg", "nonpos", "min", "max")


def test_argument_errors():
    from advchain.augmentor import calculate_image_diff3D, calculate_jacobian_determinant3D, jacobian_folding_stats
    from advchain_amd import ops
    z = torch.zeros
    for bad in (lambda: calculate_image_diff3D(z(1, 1, 4, 4)),
                lambda: calculate_image_diff3D(z(1, 1, 4, 4, 4, 4)),
                lambda: calculate_jacobian_determinant3D(z(1, 3, 4, 4)),
                lambda: calculate_jacobian_determinant3D(z(1, 2, 4, 4, 4)),
                lambda: calculate_jacobian_determinant3D(z(1, 3, 4, 4, 4), type='deformation'),
                lambda: jacobian_folding_stats(z(1, 3, 4, 4)),
                lambda: jacobian_folding_stats(z(1, 2, 4, 4, 4)),
                lambda: jacobian_folding_stats(z(1, 2, 4)),
                lambda: jacobian_folding_stats(z(1, 2, 4, 4), type='grid'),
                lambda: ops.jacobian_det(z(1, 3, 4, 4)),
                lambda: ops.jacobian_stats(z(1, 2, 4, 4, 4))):
        with pytest.raises(AssertionError):
            bad()
    for shape in ((1, 3, 1, 4, 4), (1, 3, 4, 1, 4), (1, 3, 4, 4, 1)):
        with pytest.raises(IndexError):
            calculate_image_diff3D(z(*shape))
        with pytest.raises(IndexError):
            calculate_jacobian_determinant3D(z(*shape))
        with pytest.raises(IndexError):
            jacobian_folding_stats(z(*shape), type='positions')
    with pytest.raises(IndexError):
        jacobian_folding_stats(z(1, 2, 1, 4))
    with pytest.raises(ValueError):
        ops.jacobian_det(z(1, 3, 4, 4, 4), positions=False, clamp=True)


def test_cpu_tensors_have_no_path():
    from advchain.augmentor import calculate_image_diff3D, calculate_jacobian_determinant3D, jacobian_folding_stats
    from advchain_amd import _lib, ops
    z = torch.zeros
    for call in (lambda: calculate_image_diff3D(z(1, 2, 4, 4, 4)),
                 lambda: calculate_jacobian_determinant3D(z(1, 3, 4, 4, 4)),
                 lambda: calculate_jacobian_determinant3D(z(1, 3, 4, 4, 4), type='positions'),
                 lambda: jacobian_folding_stats(z(1, 3, 4, 4, 4)),
                 lambda: jacobian_folding_stats(z(1, 2, 4, 4)),
                 lambda: ops.jacobian_det(z(1, 2, 4, 4), positions=True, clamp=True),
                 lambda: ops.jacobian_stats(z(1, 2, 4, 4))):
        with pytest.raises(_lib.AdvchainHipError):
            call()


def test_2d_names_still_refuse_3d():
    from advchain.augmentor import calculate_image_diff, calculate_jacobian_determinant
    with pytest.raises(AssertionError):
        calculate_image_diff(torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(AssertionError):
        calculate_jacobian_determinant(torch.zeros(1, 3, 4, 4, 4))
    with pytest.raises(AssertionError):
        calculate_jacobian_determinant(torch.zeros(1, 2, 4, 4), type='positions')


def test_c_entries_validate_on_the_host():
    """No launch: a null pointer, an ndim other than 2 or 3 and an axis below 2 are refused with the entry's name."""
    from advchain_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)           # never dereferenced: every call below fails before a launch
    d3, d2 = _lib.dims_array((4, 4, 4)), _lib.dims_array((4, 4))
    thin3, thin2 = _lib.dims_array((4, 1, 4)), _lib.dims_array((1, 4))

    def refused(rc, name):
        assert rc < 0 and name in lib.advchain_last_error(), (rc, lib.advchain_last_error())

    refused(lib.advchain_image_diff3d_fwd(None, p, p, p, 1, 1, d3, None), b"image_diff3d_fwd")
    refused(lib.advchain_image_diff3d_fwd(p, p, p, None, 1, 1, d3, None), b"image_diff3d_fwd")
    refused(lib.advchain_image_diff3d_fwd(p, p, p, p, 1, 1, thin3, None), b"image_diff3d_fwd")
    refused(lib.advchain_image_diff3d_fwd(p, p, p, p, 1, 1, None, None), b"image_diff3d_fwd")
    refused(lib.advchain_image_diff3d_bwd(None, None, None, p, 1, 1, d3, None), b"image_diff3d_bwd")
    refused(lib.advchain_image_diff3d_bwd(p, None, None, None, 1, 1, d3, None), b"image_diff3d_bwd")
    refused(lib.advchain_image_diff3d_bwd(p, p, p, p, 1, 1, thin3, None), b"image_diff3d_bwd")
    for nd, dims, thin in ((3, d3, thin3), (2, d2, thin2)):
        refused(lib.advchain_jacobian_det_fwd(None, p, 1, nd, dims, 0, None), b"jacobian_det_fwd")
        refused(lib.advchain_jacobian_det_fwd(p, p, 1, nd, thin, 0, None), b"jacobian_det_fwd")
        refused(lib.advchain_jacobian_det_fwd(p, p, 1, nd, dims, 2, None), b"jacobian_det_fwd")
        refused(lib.advchain_jacobian_det_bwd(p, p, None, None, 1, nd, dims, 1, None), b"jacobian_det_bwd")
        refused(lib.advchain_jacobian_det_bwd(p, p, p, None, 1, nd, thin, 3, None), b"jacobian_det_bwd")
        refused(lib.advchain_jacobian_stats(p, p, p, p, None, p, 1, nd, dims, 0, None), b"jacobian_stats")
        refused(lib.advchain_jacobian_stats(p, None, p, p, p, p, 1, nd, dims, 0, None), b"jacobian_stats")
        refused(lib.advchain_jacobian_stats(p, p, p, p, p, p, 1, nd, thin, 1, None), b"jacobian_stats")
    for nd in (1, 4):
        refused(lib.advchain_jacobian_det_fwd(p, p, 1, nd, d3, 0, None), b"jacobian_det_fwd")
        refused(lib.advchain_jacobian_det_bwd(p, p, p, None, 1, nd, d3, 0, None), b"jacobian_det_bwd")
        refused(lib.advchain_jacobian_stats(p, p, p, p, p, p, 1, nd, d3, 0, None), b"jacobian_stats")
    refused(lib.advchain_jacobian_stats(p, p, p, p, p, None, 1, 3, d3, 0, None), b"jacobian_stats")
    assert lib.advchain_jacobian_det_workspace(2, 3, d3) == 0
    # one 16-byte partial per wave: 4 planes x 1 column chunk x 1 row strip per entry
    assert lib.advchain_jacobian_stats_workspace(2, 3, d3) == 2 * 4 * 4 and lib.advchain_jacobian_stats_workspace(2, 2, d2) == 2 * 4
    assert lib.advchain_jacobian_stats_workspace(2, 3, thin3) == -1 and lib.advchain_jacobian_stats_workspace(2, 4, d3) == -1


def _coords(shape):
    """voxel index coordinates (x, y[, z]) of a spatial shape, float64, x along the last axis"""
    axes = [torch.arange(s, dtype=torch.float64) for s in shape]
    return list(reversed(torch.meshgrid(axes, indexing="ij")))


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 4), (6, 7)])
def test_closed_form_of_an_affine_displacement(shape):
    """f = A x + b: the one-sided stencils are exact on linear data, so det == det(I + A) at EVERY voxel, borders included."""
    nd = len(shape)
    A = torch.rand(nd, nd, dtype=torch.float64, generator=torch.Generator().manual_seed(7)) - 0.5
    c = _coords(shape)
    field = torch.stack([sum(A[i, j] * c[j] for j in range(nd)) + 0.25 * i for i in range(nd)]).unsqueeze(0)
    det = F.jacobian_det64(field)
    want = torch.linalg.det(torch.eye(nd, dtype=torch.float64) + A)
    assert det.shape == (1, 1) + tuple(shape)
    assert float((det - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs()))
    err32 = float((F.jacobian_det32(field).double() - want).abs().max())
    assert err32 <= 1e-5 * max(1.0, float(want.abs()))
    neg, nonpos, mn, mx = F.stats_of(det)
    assert int(neg) == (det.numel() if want < 0 else 0) and int(nonpos) == int(neg)
    assert abs(float(mn) - float(want)) <= 1e-13 and abs(float(mx) - float(want)) <= 1e-13


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 4, 5), (5, 3)])
def test_closed_form_of_the_identity_grid(shape):
    """positions mode: the identity sampling grid has J = I"""
    from advchain.augmentor import get_base_grid
    grid = get_base_grid(2, *shape, device=torch.device("cpu"))
    for clamp in (False, True):
        det = F.jacobian_det64(grid, positions=True, clamp=clamp)
        assert float((det - 1).abs().max()) <= 1e-6          # (the grid itself is fp32 linspace)
    half = F.jacobian_det64(0.5 * grid.double(), positions=True)
    assert float((half - 0.5 ** len(shape)).abs().max()) <= 1e-6
    # the clamp acts before the stencil: a grid pushed wholly past +1 collapses to one point, det = 0
    gone = F.jacobian_det64(grid.double() + 3.0, positions=True, clamp=True)
    assert float(gone.abs().max()) == 0.0


def test_stencil_and_nan_rules_of_the_forms():
    x = torch.tensor([[[[1.0, 4.0, 9.0, 16.0]] * 2]], dtype=torch.float64)       # (1,1,2,4)
    dx, dy = F.image_diff(x)
    assert dx[0, 0, 0].tolist() == [3.0, 4.0, 6.0, 7.0] and float(dy.abs().max()) == 0.0
    with pytest.raises(IndexError):
        F.diff_axis(torch.zeros(1, 1, 1, 4), 2)
    det = torch.tensor([[1.0, -2.0, 0.0, float("nan")]])
    neg, nonpos, mn, mx = F.stats_of(det)
    assert (int(neg), int(nonpos), float(mn), float(mx)) == (1, 3, -2.0, 1.0)
