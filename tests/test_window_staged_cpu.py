"""Host paths of the staged deterministic window scatter (include/advchain_hip.h: advchain_window_stage_workspace,
advchain_grid_sample_bwd_staged, advchain_last_bwd_route): the size formula and the argument checks.  No kernel is launched, no
GPU needed."""
import ctypes

import pytest

from advchain_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from advchain_amd.build import build_library
    build_library()
    return _lib.load()


def test_version_and_symbols(lib):
    assert lib.advchain_version() >= 190
    for name in ("advchain_window_stage_workspace", "advchain_grid_sample_bwd_staged", "advchain_last_bwd_route"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)


@pytest.mark.parametrize("N,C,dims", [(32, 4, (256, 256)), (3, 1, (64, 96)), (3, 2, (100, 72)), (2, 4, (33, 40)), (1, 1, (1, 2))])
def test_stage_workspace_is_the_documented_formula_whatever_the_switch_says(lib, N, C, dims):
    """int32 elements per batch entry: tiles of 32 x 32 samples, each with a header of 8 and a window slot of the LDS budget
    (8192 cells, 12288 for four channels)."""
    tiles = ((dims[0] + 31) // 32) * ((dims[1] + 31) // 32)
    want = N * tiles * ((12288 if C == 4 else 8192) + 8)
    was = lib.advchain_get_deterministic()
    try:
        got = []
        for on in (0, 1):
            lib.advchain_set_deterministic(on)
            got.append(lib.advchain_window_stage_workspace(N, C, 2, _lib.dims_array(dims)))
    finally:
        lib.advchain_set_deterministic(was)
    assert got == [want, want], (got, want)


def test_stage_workspace_is_zero_where_the_form_does_not_exist_and_negative_for_bad_arguments(lib):
    assert lib.advchain_window_stage_workspace(2, 3, 2, _lib.dims_array((64, 64))) == 0
    assert lib.advchain_window_stage_workspace(2, 8, 2, _lib.dims_array((64, 64))) == 0
    assert lib.advchain_window_stage_workspace(2, 4, 3, _lib.dims_array((8, 64, 64))) == 0
    assert lib.advchain_window_stage_workspace(0, 4, 2, _lib.dims_array((64, 64))) == 0
    assert lib.advchain_window_stage_workspace(2, 0, 2, _lib.dims_array((64, 64))) < 0
    assert lib.advchain_window_stage_workspace(-1, 4, 2, _lib.dims_array((64, 64))) < 0
    assert lib.advchain_window_stage_workspace(2, 4, 4, _lib.dims_array((8, 8, 8, 8))) < 0
    assert lib.advchain_window_stage_workspace(2, 4, 2, None) < 0


def test_scatter_workspace_keeps_its_sizes(lib):
    dims = (64, 96)
    V = 64 * 96
    was = lib.advchain_get_deterministic()
    try:
        lib.advchain_set_deterministic(0)
        small = lib.advchain_scatter_workspace(3, 2, _lib.dims_array(dims))
        lib.advchain_set_deterministic(1)
        big = lib.advchain_scatter_workspace(3, 2, _lib.dims_array(dims))
    finally:
        lib.advchain_set_deterministic(was)
    assert small == 4 + 2 * 3 * V and big == small + 8 * 3 * V + 4, (small, big)


P = ctypes.c_void_p(64)      # a non-null, 16-byte aligned address: the checks fail before anything is read or launched


def _staged(lib, gout=P, inp=P, grid=P, gin=P, ggrid=P, ws=P, N=2, C=4, nd=2, idims=(8, 8), odims=(8, 8), interp=0, padding=0,
            stage=P):
    return lib.advchain_grid_sample_bwd_staged(gout, inp, grid, gin, ggrid, ws, N, C, nd, _lib.dims_array(idims),
                                               _lib.dims_array(odims), interp, padding, 0, 16, None, stage)


def test_staged_entry_rejects_bad_arguments(lib):
    bad = [
        dict(gout=None), dict(inp=None), dict(grid=None),          # the checks of advchain_grid_sample_bwd
        dict(gin=None, ggrid=None),
        dict(N=-1), dict(N=65536), dict(C=0),
        dict(interp=2), dict(padding=3),
        dict(nd=4, idims=(8, 8, 8, 8), odims=(8, 8, 8, 8)),
        dict(idims=(0, 8)),
        dict(ws=None),                                             # a staging buffer without the scatter workspace
        dict(gin=None),                                            # ... or without grad_in
        dict(stage=ctypes.c_void_p(68)),                           # not 16-byte aligned
        dict(C=3), dict(C=8),                                      # no staged form for these
        dict(nd=3, idims=(8, 8, 8), odims=(8, 8, 8)),
    ]
    for kw in bad:
        assert _staged(lib, **kw) == -1, kw
        assert lib.advchain_last_error(), kw


def test_nothing_runs_for_an_empty_batch_and_the_route_getter_is_host_only(lib):
    assert _staged(lib, N=0) == 0
    assert 0 <= lib.advchain_last_bwd_route() <= 8
