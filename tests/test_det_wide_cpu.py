"""Host paths of the deterministic general warps (include/advchain_hip.h: advchain_det_warp_workspace,
advchain_grid_sample_bwd_det, advchain_affine_warp_bwd_det): the workspace formula and the argument checks.  No kernel is
launched, no GPU needed."""
import ctypes

import pytest

from advchain_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from advchain_amd.build import build_library
    build_library()
    return _lib.load()


def test_version_and_symbols(lib):
    assert lib.advchain_version() >= 170
    for name in ("advchain_det_warp_workspace", "advchain_grid_sample_bwd_det", "advchain_affine_warp_bwd_det"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)


@pytest.mark.parametrize("N,C,dims", [(3, 20, (12, 20, 16)), (2, 6, (33, 47)), (5, 1, (7, 9)), (4, 9, (3, 4, 5))])
def test_det_warp_workspace_is_the_documented_formula_whatever_the_switch_says(lib, N, C, dims):
    """int32 elements: the int64 image (2 N C V) plus one maximum per batch entry, padded to a multiple of four as
    advchain_scatter_workspace pads its own."""
    V = 1
    for s in dims:
        V *= s
    want = 2 * N * C * V + ((N + 3) // 4) * 4
    was = lib.advchain_get_deterministic()
    try:
        got = []
        for on in (0, 1):
            lib.advchain_set_deterministic(on)
            got.append(lib.advchain_det_warp_workspace(N, C, len(dims), _lib.dims_array(dims)))
    finally:
        lib.advchain_set_deterministic(was)
    assert got == [want, want], (got, want)
    assert want % 2 == 0          # the maxima start on an 8-byte boundary, the image being first


def test_det_warp_workspace_rejects_bad_arguments(lib):
    assert lib.advchain_det_warp_workspace(2, 0, 2, _lib.dims_array((8, 8))) < 0
    assert lib.advchain_det_warp_workspace(-1, 3, 2, _lib.dims_array((8, 8))) < 0
    assert lib.advchain_det_warp_workspace(2, 3, 4, _lib.dims_array((8, 8, 8, 8))) < 0
    assert lib.advchain_det_warp_workspace(2, 3, 2, None) < 0


P = ctypes.c_void_p(64)      # a non-null address: the checks fail before anything is read or launched


def _grid_bwd_det(lib, gout=P, inp=P, grid=P, gin=P, ggrid=P, ws=P, N=2, C=6, nd=2, idims=(8, 8), odims=(8, 8), interp=0,
                  padding=0):
    return lib.advchain_grid_sample_bwd_det(gout, inp, grid, gin, ggrid, ws, N, C, nd, _lib.dims_array(idims),
                                            _lib.dims_array(odims), interp, padding, 0, None)


def _affine_bwd_det(lib, gout=P, inp=P, theta=P, gin=P, gth=P, ws=P, dws=P, N=2, C=9, nd=2, dims=(8, 8), interp=0, padding=0):
    return lib.advchain_affine_warp_bwd_det(gout, inp, theta, gin, gth, ws, dws, N, C, nd, _lib.dims_array(dims), interp,
                                            padding, None)


@pytest.mark.parametrize("kw", [dict(gout=None), dict(inp=None), dict(grid=None), dict(gin=None, ggrid=None), dict(ws=None),
                                dict(interp=2), dict(interp=-1), dict(padding=3), dict(C=0), dict(nd=4), dict(idims=(1, 1)),
                                dict(N=70000)])
def test_grid_sample_bwd_det_checks_its_arguments(lib, kw):
    assert _grid_bwd_det(lib, **kw) < 0
    assert b"grid_sample_bwd_det" in lib.advchain_last_error()


def test_grid_sample_bwd_det_needs_no_workspace_for_grad_grid_alone_and_nothing_for_an_empty_batch(lib):
    assert _grid_bwd_det(lib, N=0) == 0
    assert _grid_bwd_det(lib, N=0, gin=None, ws=None) == 0


@pytest.mark.parametrize("kw", [dict(gout=None), dict(inp=None), dict(theta=None), dict(gin=None, gth=None), dict(ws=None),
                                dict(dws=None), dict(interp=2), dict(padding=-1), dict(C=0), dict(nd=1), dict(dims=(1, 1))])
def test_affine_warp_bwd_det_checks_its_arguments(lib, kw):
    assert _affine_bwd_det(lib, **kw) < 0
    assert b"affine_warp_bwd_det" in lib.advchain_last_error()


def test_affine_warp_bwd_det_accepts_an_empty_batch(lib):
    assert _affine_bwd_det(lib, N=0) == 0
    assert _affine_bwd_det(lib, N=0, gin=None, dws=None) == 0


def test_ops_sends_only_the_general_kernels_calls_to_the_twin():
    """The helper mirrors the dispatch condition of advchain_grid_sample_bwd: C <= 4, linear, same size -> a fast route."""
    from advchain_amd import ops
    g = ops._general_warp_kernel
    assert not g(4, 0, (8, 8), (8, 8)) and not g(1, 0, (4, 5, 6), (4, 5, 6))
    assert g(5, 0, (8, 8), (8, 8)) and g(3, 1, (8, 8), (8, 8)) and g(3, 0, (8, 8), (8, 9))
