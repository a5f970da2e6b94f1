"""The bias-field kernels over AdvBias's configuration space, against OracleBias in double (tests/bias_config_cases.py).

Every case goes through the public class, once in eval() and once in train() with power_iteration (the kernels then get
cp_scale = xi), and is held to the project's bounds for these quantities: field and output 5e-6, control-point gradient
2e-5 * max(1, |g_ref|.max()), data gradient 1e-5.  Each case prints one line with its worst errors and the bounds.  The route
a case is meant for is asserted with the library's own queries and return codes, never by kernel names.

Two kernel-level tests drive the raw entries on the tables with a control-point row of 68 and with bands of 7, at every
rows_per_wg, against the dense band matrices in double (tests/cpu_backend): the rows entries of the bias field, and the plain
interpolation and its adjoint, which AdvBias.forward does not use."""
import functools

import numpy as np
import pytest
import torch

from tests import bias_config_cases as K
from tests import cpu_backend
from tests.layout_cases import offset_copy

pytestmark = pytest.mark.gpu

NAMES = list(K.CASES)
ROWS = (0, 4, 8, 16, 32)
SENTINEL = 7.0
U = 2.0 ** -24      # unit roundoff of float32


def _ops():
    from advchain_amd import ops
    return ops


def _transform(name, power_iteration=False):
    from advchain_amd.augmentor import AdvBias
    t = AdvBias(K.CASES[name][0], K.config(name), power_iteration=power_iteration, device=torch.device("cuda"))
    t.init_parameters()
    assert (tuple(t._tables.g), tuple(t._tables.B)) == K.EXPECT[name], (name, t._tables.g, t._tables.B)
    return t


class _Noting(object):
    """the library with the two backward entries noted as (name, return code); refuse: the reduced backward answers -2 unasked"""

    def __init__(self, lib, seen, refuse=False):
        self._lib, self._seen, self._refuse = lib, seen, refuse

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("advchain_bias_field_bwd_reduced", "advchain_bias_field_bwd"):
            return fn

        def call(*a):
            rc = -2 if (self._refuse and name == "advchain_bias_field_bwd_reduced") else fn(*a)
            self._seen.append((name, rc))
            return rc
        return call


def _note(monkeypatch, refuse=False):
    from advchain_amd import _lib
    lib, seen = _lib.load(), []
    monkeypatch.setattr(_lib, "load", lambda: _Noting(lib, seen, refuse))
    return seen


def _route(accepts):
    return [("advchain_bias_field_bwd_reduced", 0)] if accepts else \
        [("advchain_bias_field_bwd_reduced", -2), ("advchain_bias_field_bwd", 0)]


def _run(t, param, data, gout):
    """forward and backward through the class -> (field, out, grad_param, grad_data)"""
    p = param.detach().requires_grad_(True)
    d = data.detach().requires_grad_(True)       # (a view stays a view: a misaligned `data` stays so)
    t.param = p
    out = t.forward(d)
    (out * gout).sum().backward()
    torch.cuda.synchronize()
    return t.bias_field, out, p.grad, d.grad


@pytest.mark.parametrize("mode", ["eval", "power_iteration"])
@pytest.mark.parametrize("name", NAMES)
def test_case_against_the_double_reference(name, mode, monkeypatch):
    from advchain_amd import _lib
    pi = mode == "power_iteration"
    lib = _lib.load()
    t = _transform(name, pi)
    tb = t._tables
    if name in K.LONG_ROW:
        assert tb.g[2] > 64
    assert lib.advchain_tp_wide_band(tb.B[2]) == (tb.B[2] if tb.B[2] in (2, 4) else 0)
    param, data, gout = (x.cuda() for x in K.inputs(name, pi))
    ref = K.reference(name, pi)
    if pi:
        t.train()
        assert t.is_training and t.power_iteration
    else:
        # the field the class computes from its parameters alone (advchain_bias_field_fwd without data)
        t.param = param
        t.bias_field = None
        own = t.bias_field
        assert tuple(own.shape) == (data.shape[0], 1) + tuple(data.shape[2:])
        assert float((own.cpu().double() - ref[0][:, :1]).abs().max()) <= 5e-6
    seen = _note(monkeypatch)
    got = _run(t, param, data, gout)
    assert tuple(got[0].shape) == tuple(data.shape) and tuple(got[2].shape) == tuple(param.shape)
    K.check("%s %s" % (name, mode), got, ref, pi)
    assert seen == _route(K.reduced_backward_accepts(tb)), (name, seen)
    # both branches of the clip were taken, as the case list promises
    clipped = float(((got[0] - 1).abs() >= K.EPSILON - 1e-6).float().mean())
    assert K.CLIPPED_SHARE[0] <= clipped <= K.CLIPPED_SHARE[1], clipped


@pytest.mark.parametrize("name", [n for n in NAMES if K.CASES[n][1][-1] % 4 == 0 and K.CASES[n][1][-1] <= 1024
                                  and K.EXPECT[n][0][2] <= 64])
def test_the_same_gradient_with_the_reduced_backward_refused(name, monkeypatch):
    """the two launches behind a refusal (advchain_bias_field_bwd, then the adjoint passes over grad_L) give what the reduced
    backward gives: the same bits (the contract of tests/test_bias_rows_gpu.py), and so the same distance from the reference"""
    t = _transform(name)
    assert K.reduced_backward_accepts(t._tables)
    param, data, gout = (x.cuda() for x in K.inputs(name))
    seen = _note(monkeypatch)
    want = _run(t, param, data, gout)
    assert seen == _route(True), seen
    del seen[:]
    monkeypatch.undo()
    seen = _note(monkeypatch, refuse=True)
    got = _run(t, param, data, gout)
    assert seen == _route(False), seen
    K.check("%s refused" % name, got, K.reference(name))
    for what, a, b in zip(("field", "out", "grad_param", "grad_data"), got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, what)


@pytest.mark.parametrize("name", [K.G68, "2d_o5_b6_nc", "3d_o1_nc"])
def test_data_four_bytes_into_its_storage(name, monkeypatch):
    """data and grad_out contiguous but not 16-byte aligned: one voxel a thread, the reduced backward refused"""
    t = _transform(name)
    param, data, gout = (x.cuda() for x in K.inputs(name))
    seen = _note(monkeypatch)
    got = _run(t, param, offset_copy(data, 1), offset_copy(gout, 1))
    K.check("%s offset" % name, got, K.reference(name))
    assert seen == _route(False), seen


# ------------------------------------------------------------------------------------------------ the raw entries
def _guarded(shape, k):
    """(buffer, view): a view of `shape`, k floats into a buffer of sentinels with four more behind it (k = 4: 16-byte aligned)"""
    n = int(np.prod(shape))
    buf = torch.full((n + k + 4,), SENTINEL, device="cuda")
    view = buf[k:k + n].view(shape)
    assert view.data_ptr() % 16 == (4 * k) % 16 and view.is_contiguous()
    return buf, view


def _untouched(buf, view, k):
    n = view.numel()
    return bool((buf[:k] == SENTINEL).all()) and bool((buf[k + n:] == SENTINEL).all())


def _args(ops, tables):
    from advchain_amd import _lib
    return (ops._ptr(tables.itab), ops._ptr(tables.ftab), _lib.dims_array(tables.S), _lib.dims_array(tables.g),
            _lib.dims_array(tables.B))


@functools.lru_cache(maxsize=None)
def _dense_reference(name):
    """float64 dense form of the case (tests/cpu_backend.bias_apply on the host copies of the band matrices) ->
    (field, out, grad_cp, grad_data)"""
    t = _transform(name)
    param, data, gout = K.inputs(name)
    cpd, dd = param.double().requires_grad_(True), data.double().requires_grad_(True)
    out, field = cpu_backend.bias_apply(cpd, dd, t._tables, K.EPSILON, K.CASES[name][5] == "log", 1.0)
    out.backward(gout.double())
    return field.expand(data.shape), out.detach(), cpd.grad, dd.grad


@pytest.mark.parametrize("k", [4, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("name", [K.G68, K.BAND7])
def test_rows_entries_against_the_dense_form(name, k):
    """advchain_bias_field_fwd_rows / _bwd_rows at every rows_per_wg; the outputs are views of larger buffers.  k = 1: every
    operand 4 bytes off a 16-byte boundary, the kernels with one voxel a thread."""
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    t = _transform(name)
    tb = t._tables
    use_log = int(K.CASES[name][5] == "log")
    param, data, gout = (x.cuda() for x in K.inputs(name))
    if k != 4:
        data, gout = offset_copy(data, k), offset_copy(gout, k)
    N, C = data.shape[:2]
    one = (N, 1) + tuple(data.shape[2:])
    ref = _dense_reference(name)
    for rows in ROWS:
        (bo, out), (bf, field) = _guarded(data.shape, k), _guarded(one, k)
        _lib.check(lib.advchain_bias_field_fwd_rows(ops._ptr(param), ops._ptr(data), ops._ptr(out), ops._ptr(field), *_args(ops, tb),
                                                    N, C, K.EPSILON, use_log, 1.0, rows, ops._stream()), "bias_field_fwd_rows")
        (bl, gL), (bd, gdata) = _guarded(one, k), _guarded(data.shape, k)
        _lib.check(lib.advchain_bias_field_bwd_rows(ops._ptr(param), ops._ptr(data), ops._ptr(gout), ops._ptr(gL), ops._ptr(gdata),
                                                    *_args(ops, tb), N, C, K.EPSILON, use_log, 1.0, rows, ops._stream()),
                   "bias_field_bwd_rows")
        gcp = ops.raw_tp_adjoint(gL, tb).reshape(param.shape)
        torch.cuda.synchronize()
        K.check("%s rows=%d %s" % (name, rows, "aligned" if k == 4 else "offset"), (field.expand(data.shape), out, gcp, gdata), ref)
        for buf, view in ((bo, out), (bf, field), (bl, gL), (bd, gdata)):
            assert _untouched(buf, view, k), (name, rows)
        assert float(gL.abs().max()) > 0


def _dense(tables, dtype=torch.float64):
    return [torch.from_numpy(np.asarray(m)).to(dtype) for m in tables.mats]


def _apply(mats, x, adjoint=False):
    """the tensor product of the three band matrices on (N, C, a0, a1, a2), or of their transposes"""
    return torch.einsum("ncijk,xi,yj,zk->ncxyz", x, *mats) if not adjoint else torch.einsum("ncxyz,xi,yj,zk->ncijk", x, *mats)


@pytest.mark.parametrize("name", [K.G68, K.BAND7, "3d_g68"])
def test_plain_interpolation_and_adjoint_against_the_dense_matrices(name):
    """ops.raw_tp_interp (k_tp_interp_fwd: 32 rows a workgroup, so a row of 68 control points takes two passes through the
    2048 floats of LDS; bands of 7 in the run-time band loop) and ops.raw_tp_adjoint (no dense reduction at g2 > 64).

    Bound, element by element: every output is a chain of at most n products and sums of float32 numbers over the three axes,
    n = the sum of the per-axis chain lengths (the band widths forward; the longest column support hi - lo for the adjoint)
    plus 3 for the rounding of the three weights to float32 and 3 for the scale and the stores -- the standard bound
    n u |W| |x| of a dot product with u = 2^-24, with |W| |x| from the absolute values in double, doubled for slack in the
    order of the sums."""
    ops = _ops()
    t = _transform(name)
    tb = t._tables
    nd = tb.ndim
    mats = _dense(tb)
    amats = [m.abs() for m in mats]
    g = torch.Generator().manual_seed(5)
    N, C = 2, 2
    coef = torch.randn((N, C) + tuple(tb.coef_dims), generator=g)
    full = torch.randn((N, C) + tuple(tb.full_dims), generator=g)
    pad3 = lambda x: x.reshape(x.shape[:2] + (1,) * (3 - nd) + tuple(x.shape[2:])).double()      # noqa: E731
    # forward
    want = _apply(mats, pad3(coef)).reshape(full.shape)
    bound = 2 * (sum(tb.B) + 6) * U * _apply(amats, pad3(coef).abs()).reshape(full.shape)
    for k in (4, 1):
        buf, out = _guarded(full.shape, k)
        got = ops.raw_tp_interp(coef.cuda(), tb, C, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and _untouched(buf, out, k)
        err = (got.cpu().double() - want).abs()
        print("%s interp k=%d: worst error %.3g, worst error/bound %.3g" % (name, k, float(err.max()), float((err / bound).max())))
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    # adjoint
    itab = tb.itab.cpu().numpy()
    span, o = [], 0
    for S, gg in zip(tb.S, tb.g):
        lo, hi = itab[o + S:o + S + gg], itab[o + S + gg:o + S + 2 * gg]
        span.append(int((hi - lo).max()))
        o += S + 2 * gg
    want = _apply(mats, pad3(full), adjoint=True).reshape(coef.shape)
    bound = 2 * (sum(span) + 6) * U * _apply(amats, pad3(full).abs(), adjoint=True).reshape(coef.shape)
    for k in (0, 1):
        x = full.cuda() if k == 0 else offset_copy(full.cuda(), k)
        got = ops.raw_tp_adjoint(x, tb).reshape(coef.shape)
        torch.cuda.synchronize()
        err = (got.cpu().double() - want).abs()
        print("%s adjoint k=%d: worst error %.3g, worst error/bound %.3g" % (name, k, float(err.max()), float((err / bound).max())))
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0 and bool((err <= bound).all())
