"""Host side of the bias kernels' rows per workgroup and of the backward that reduces its rows along x (include/advchain_hip.h:
advchain_bias_rows_per_wg, advchain_bias_field_fwd_rows / _bwd_rows, advchain_bias_field_bwd_reduced): the header, the prototype
table and the library agree on the names, and null pointers fail on the host with a message.  No kernel is launched, no GPU
needed."""
import ctypes
import os

import pytest

from advchain_amd import _lib

NAMES = ("advchain_bias_rows_per_wg", "advchain_bias_field_fwd_rows", "advchain_bias_field_bwd_rows",
         "advchain_bias_field_bwd_reduced")


@pytest.fixture(scope="module")
def lib():
    from advchain_amd.build import build_library
    build_library()
    return _lib.load()


def test_version_header_prototypes_and_exports(lib):
    assert lib.advchain_version() >= 200
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "advchain_hip.h")).read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    # one more argument (rows_per_wg) than the entries they extend; the reduced entry adds t1's table and rows_per_wg
    n = lambda k: len(_lib.PROTOTYPES[k][1])      # noqa: E731
    assert n("advchain_bias_field_fwd_rows") == n("advchain_bias_field_fwd") + 1
    assert n("advchain_bias_field_bwd_rows") == n("advchain_bias_field_bwd") + 1
    assert n("advchain_bias_field_bwd_reduced") == n("advchain_bias_field_bwd") + 4


def test_the_query_is_host_only(lib):
    q = lambda S, N: lib.advchain_bias_rows_per_wg(_lib.dims_array(S), N)      # noqa: E731
    assert [q((1, 1024, 8), 64), q((1, 512, 8), 16), q((1, 256, 8), 16), q((1, 16, 16), 2)] == [32, 16, 8, 4]
    assert q((1, 256, 256), 32) == 16
    assert q((1, 256, 256), 65536) == -1 and q((1, 256, 0), 1) == -1 and lib.advchain_bias_rows_per_wg(None, 1) == -1


P = ctypes.c_void_p(64)      # a non-null, 16-byte aligned address: the checks fail before anything is read or launched
D = _lib.dims_array((1, 8, 8))


def _fwd(lib, cp=P, data=P, out=P, field=P, itab=P, ftab=P, S=D, g=D, B=D, rows=0):
    return lib.advchain_bias_field_fwd_rows(cp, data, out, field, itab, ftab, S, g, B, 2, 1, 0.3, 1, 1.0, rows, None)


def _bwd(lib, cp=P, data=P, gout=P, gL=P, gdata=P, itab=P, ftab=P, S=D, g=D, B=D, rows=0):
    return lib.advchain_bias_field_bwd_rows(cp, data, gout, gL, gdata, itab, ftab, S, g, B, 2, 1, 0.3, 1, 1.0, rows, None)


def _red(lib, cp=P, data=P, gout=P, t1=P, gdata=P, itab=P, ftab=P, S=D, g=D, B=D, wd=P, lo=P, WB=8, rows=0):
    return lib.advchain_bias_field_bwd_reduced(cp, data, gout, t1, gdata, itab, ftab, S, g, B, 2, 1, 0.3, 1, 1.0, wd, lo, WB, rows,
                                               None)


def test_null_pointers_and_bad_rows_fail_on_the_host_with_a_message(lib):
    cases = [(_fwd, k) for k in (dict(cp=None), dict(field=None), dict(out=None), dict(itab=None), dict(ftab=None), dict(S=None),
                                 dict(g=None), dict(B=None), dict(rows=5), dict(rows=-4), dict(rows=64))]
    cases += [(_bwd, k) for k in (dict(cp=None), dict(data=None), dict(gout=None), dict(gL=None, gdata=None), dict(itab=None),
                                  dict(S=None), dict(rows=12))]
    cases += [(_red, k) for k in (dict(cp=None), dict(data=None), dict(gout=None), dict(wd=None), dict(lo=None), dict(itab=None),
                                  dict(ftab=None), dict(g=None), dict(WB=0), dict(rows=3))]
    for fn, kw in cases:
        lib.advchain_set_error_(b"") if hasattr(lib, "advchain_set_error_") else None
        assert fn(lib, **kw) == -1, (fn.__name__, kw)
        assert lib.advchain_last_error(), (fn.__name__, kw)


def test_the_reduced_entry_refuses_on_the_host(lib):
    """-2 before anything is enqueued: no t1, a row length that is no multiple of 4, a misaligned operand, a dense table beyond
    4096 floats, more than 64 coefficients per row, a row beyond 1024"""
    assert _red(lib, t1=None) == -2
    assert _red(lib, S=_lib.dims_array((1, 30, 30)), WB=30) == -2
    assert _red(lib, data=ctypes.c_void_p(68)) == -2
    assert _red(lib, gout=ctypes.c_void_p(72)) == -2
    assert _red(lib, gdata=ctypes.c_void_p(76)) == -2
    assert _red(lib, S=_lib.dims_array((1, 8, 2048)), WB=2) == -2
    assert _red(lib, S=_lib.dims_array((1, 8, 512)), g=_lib.dims_array((1, 8, 80)), WB=16) == -2
    assert _red(lib, S=_lib.dims_array((1, 8, 512)), g=_lib.dims_array((1, 8, 16)), WB=512) == -2
