"""The bias kernels with their rows per workgroup chosen at run time, and the backward that reduces its rows along x itself
(include/advchain_hip.h: advchain_bias_rows_per_wg, advchain_bias_field_fwd_rows / _bwd_rows, advchain_bias_field_bwd_reduced).

The contract is bit-identity: the fused backward against advchain_bias_field_bwd followed by advchain_band_reduce_rows_dense, and
every rows_per_wg value against every other.  Against float64 (tests/cpu_backend.bias_apply in double) the bounds are those of
tests/test_ops_gpu.py for this operator."""
import functools

import pytest
import torch

from tests import cpu_backend

pytestmark = pytest.mark.gpu

ROWS = (4, 8, 16, 32)
# (data shape, control point spacing): rows that are no multiple of 16 or 32 with 10 column groups on 16 lanes; the channel
# loop; the smallest; 3D with a dense table that is no multiple of 4 floats (6 x 13); 3D with two channels
SHAPES = [((2, 1, 24, 40), (8, 8)), ((3, 3, 32, 32), (16, 16)), ((2, 1, 8, 8), (4, 4)),
          ((2, 1, 8, 12, 16), (4, 4, 4)), ((1, 2, 16, 16, 8), (8, 8, 4))]
IDS = ["x".join(map(str, s)) for s, _ in SHAPES]


def _ops():
    from advchain_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _geometry(shape, spacing):
    """(band tables on the GPU, control point shape) of AdvBias at this size"""
    from advchain_amd.augmentor import AdvBias
    cfg = dict(epsilon=0.3, control_point_spacing=list(spacing), downscale=2, data_size=list(shape), interpolation_order=3,
               init_mode="random", space="log")
    t = AdvBias(len(shape) - 2, cfg, device=torch.device("cuda"))
    t.init_parameters()
    return t._tables, tuple(t.param.shape)


@functools.lru_cache(maxsize=None)
def _case(shape, spacing, use_log, cp_scale):
    """cp, data, grad_out on the GPU and an eps that the clamp passes for about half of the voxels: the midpoint of the widest
    gap between the sorted |field - 1| of the float64 field in its 40 % .. 60 % quantiles, so that no voxel sits at the bound.
    The fraction is asserted here."""
    tables, cps = _geometry(shape, spacing)
    g = torch.Generator().manual_seed(1234 + len(shape) + shape[-1])
    cp = (torch.randn(cps, generator=g) * 0.4 / cp_scale).float()
    data = torch.rand(shape, generator=g) + 0.5
    gout = torch.randn(shape, generator=g)
    L = cp_scale * cpu_backend._tp_eval(cp.double(), tables)
    b = ((torch.exp(L) if use_log else 1 + L) - 1).abs().reshape(-1).sort().values
    n = b.numel()
    mid = b[int(0.4 * n):int(0.6 * n) + 2]
    i = int((mid[1:] - mid[:-1]).argmax())
    eps = float(0.5 * (mid[i] + mid[i + 1]))
    frac = float((b <= eps).double().mean())
    assert 0.1 <= frac <= 0.9, frac
    return cp.cuda(), data.cuda(), gout.cuda(), eps


def _args(ops, tables):
    from advchain_amd import _lib
    return (ops._ptr(tables.itab), ops._ptr(tables.ftab), _lib.dims_array(tables.S), _lib.dims_array(tables.g),
            _lib.dims_array(tables.B))


def _t1_shape(data, tables):
    return (data.shape[0], 1) + tuple(data.shape[2:-1]) + (int(tables.g[2]),)


def two_launches(tables, cp, data, gout, eps, use_log, cp_scale, rows=0, want_gdata=True):
    """advchain_bias_field_bwd_rows, then advchain_band_reduce_rows_dense over grad_L -> (t1, grad_data, control point gradient)"""
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    N, C = data.shape[:2]
    gL = torch.empty((N, 1) + tuple(data.shape[2:]), device="cuda")
    gdata = torch.empty_like(data) if want_gdata else None
    _lib.check(lib.advchain_bias_field_bwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(gout), ops._ptr(gL), ops._ptr(gdata),
                                                *_args(ops, tables), N, C, eps, int(use_log), cp_scale, rows, ops._stream()),
               "bias_field_bwd_rows")
    wd, lo, WB = tables.dense_inner
    t1 = torch.empty(_t1_shape(data, tables), device="cuda")
    rc = lib.advchain_band_reduce_rows_dense(ops._ptr(gL), None, ops._ptr(t1), ops._ptr(wd), ops._ptr(lo), t1.numel() // t1.shape[-1],
                                             tables.S[2], tables.g[2], WB, 1.0, ops._stream())
    assert rc == 0, rc
    return t1, gdata, ops.raw_tp_adjoint_from_t1(t1, tables).reshape(cp.shape)


def fused_rc(tables, cp, data, gout, eps, use_log, cp_scale, t1, gdata, rows=0):
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    N, C = data.shape[:2]
    wd, lo, WB = tables.dense_inner
    return lib.advchain_bias_field_bwd_reduced(ops._ptr(cp), ops._ptr(data), ops._ptr(gout), ops._ptr(t1), ops._ptr(gdata),
                                               *_args(ops, tables), N, C, eps, int(use_log), cp_scale, ops._ptr(wd), ops._ptr(lo), WB,
                                               rows, ops._stream())


def fused(tables, cp, data, gout, eps, use_log, cp_scale, rows=0, want_gdata=True):
    ops = _ops()
    t1 = torch.empty(_t1_shape(data, tables), device="cuda")
    gdata = torch.empty_like(data) if want_gdata else None
    rc = fused_rc(tables, cp, data, gout, eps, use_log, cp_scale, t1, gdata, rows)
    assert rc == 0, rc
    return t1, gdata, ops.raw_tp_adjoint_from_t1(t1, tables).reshape(cp.shape)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("want_gdata", [True, False], ids=["gdata", "nogdata"])
@pytest.mark.parametrize("cp_scale", [1.0, 1e-6])
@pytest.mark.parametrize("use_log", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("shape,spacing", SHAPES, ids=IDS)
def test_fused_equals_two_launches(shape, spacing, use_log, cp_scale, want_gdata):
    tables, _ = _geometry(shape, spacing)
    cp, data, gout, eps = _case(shape, spacing, use_log, cp_scale)
    want = two_launches(tables, cp, data, gout, eps, use_log, cp_scale, want_gdata=want_gdata)
    got = fused(tables, cp, data, gout, eps, use_log, cp_scale, want_gdata=want_gdata)
    for name, a, b in zip(("t1", "grad_data", "grad_cp"), got, want):
        assert _same(a, b), name
    assert float(want[0].abs().max()) > 0


@pytest.mark.parametrize("shape,spacing", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_every_rows_per_wg_gives_the_same_bits(shape, spacing):
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    tables, _ = _geometry(shape, spacing)
    cp, data, gout, eps = _case(shape, spacing, True, 1.0)
    N, C = data.shape[:2]
    fwd, bwd, red = [], [], []
    for rows in (0,) + ROWS:
        out = torch.empty_like(data)
        field = torch.empty((N, 1) + tuple(data.shape[2:]), device="cuda")
        _lib.check(lib.advchain_bias_field_fwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(out), ops._ptr(field), *_args(ops, tables),
                                                    N, C, eps, 1, 1.0, rows, ops._stream()), "bias_field_fwd_rows")
        fwd.append((out, field))
        bwd.append(two_launches(tables, cp, data, gout, eps, True, 1.0, rows=rows))
        red.append(fused(tables, cp, data, gout, eps, True, 1.0, rows=rows))
    for i in range(1, len(fwd)):
        assert all(_same(a, b) for a, b in zip(fwd[i], fwd[0])), ("forward", i)
        assert all(_same(a, b) for a, b in zip(bwd[i], bwd[0])), ("backward", i)
        assert all(_same(a, b) for a, b in zip(red[i], bwd[0])), ("reduced", i)
    # a value outside {0, 4, 8, 16, 32} is an argument error
    assert lib.advchain_bias_field_fwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(out), ops._ptr(field), *_args(ops, tables),
                                            N, C, eps, 1, 1.0, 5, ops._stream()) == -1


def test_the_query_returns_each_value():
    from advchain_amd import _lib
    lib = _lib.load()
    q = lambda S, N: lib.advchain_bias_rows_per_wg(_lib.dims_array(S), N)      # noqa: E731
    assert q((1, 1024, 8), 64) == 32          # 32 chunks x 64 = 2048 workgroups
    assert q((1, 512, 8), 16) == 16           # 256 workgroups at 32 rows, 512 at 16
    assert q((1, 256, 8), 16) == 8            # 512 at 8
    assert q((1, 16, 16), 2) == 4             # small launches: one row per thread
    assert q((8, 12, 16), 2) == 4
    assert q((1, 256, 256), 32) == 16         # what bench.py times: two workgroups a CU
    assert q((128, 128, 64), 4) == 32         # 4 x 128 x 4 = 2048
    assert q((1, 0, 8), 2) == -1 and q((1, 8, 8), -1) == -1 and lib.advchain_bias_rows_per_wg(None, 2) == -1


def _refusal_case(misalign):
    shape, spacing = ((2, 1, 30, 30), (10, 10)) if not misalign else SHAPES[0]
    tables, cps = _geometry(shape, spacing)
    g = torch.Generator().manual_seed(7)
    cp = (torch.randn(cps, generator=g) * 0.4).cuda()
    gout = torch.randn(shape, generator=g).cuda()
    data = torch.rand(shape, generator=g) + 0.5
    if misalign:
        flat = torch.empty(data.numel() + 4, device="cuda")
        flat[1:1 + data.numel()] = data.reshape(-1)
        data = flat[1:1 + data.numel()].view(shape)
        assert data.data_ptr() % 16 == 4 and data.is_contiguous()
    else:
        data = data.cuda()
    return tables, cp, data, gout


@pytest.mark.parametrize("misalign", [False, True], ids=["30x30", "misaligned"])
def test_refusals_leave_the_outputs_alone(misalign):
    tables, cp, data, gout = _refusal_case(misalign)
    t1 = torch.full(_t1_shape(data, tables), 7.0, device="cuda")
    gdata = torch.full(tuple(data.shape), 7.0, device="cuda")
    assert fused_rc(tables, cp, data, gout, 0.2, True, 1.0, t1, gdata) == -2
    # grad_L not wanted: nothing to reduce
    assert fused_rc(tables, cp, data.contiguous().clone(), gout, 0.2, True, 1.0, None, gdata) == -2
    torch.cuda.synchronize()
    assert bool((t1 == 7.0).all()) and bool((gdata == 7.0).all())


def _float64(tables, cp, data, gout, eps, use_log, cp_scale):
    cpd = cp.detach().cpu().double().requires_grad_(True)
    dd = data.detach().cpu().double().requires_grad_(True)
    out, field = cpu_backend.bias_apply(cpd, dd, tables, eps, use_log, cp_scale)
    out.backward(gout.cpu().double())
    return out.detach(), field, cpd.grad, dd.grad


def _check_against_float64(tables, cp, data, gout, eps, use_log, cp_scale):
    ops = _ops()
    cpg, dg = cp.detach().requires_grad_(True), data.detach().requires_grad_(True)      # (views: a misaligned `data` stays so)
    out, field = ops.bias_apply(cpg, dg, tables, eps, use_log, cp_scale)
    out.backward(gout)
    rout, rfield, rgcp, rgd = _float64(tables, cp, data, gout, eps, use_log, cp_scale)
    err = lambda a, b: float((a.detach().cpu().double() - b).abs().max())      # noqa: E731
    figures = dict(out=err(out, rout), field=err(field, rfield), gcp=err(cpg.grad, rgcp), gdata=err(dg.grad, rgd),
                   gcp_max=float(rgcp.abs().max()))
    print(figures)
    assert figures["gcp"] <= 2e-5 * max(1.0, figures["gcp_max"]), figures
    assert figures["gdata"] <= 1e-5, figures
    assert figures["field"] <= 5e-6 and figures["out"] <= 5e-6, figures


@pytest.mark.parametrize("misalign", [False, True], ids=["30x30", "misaligned"])
def test_ops_falls_back_after_a_refusal(misalign, monkeypatch):
    from advchain_amd import _lib
    tables, cp, data, gout = _refusal_case(misalign)
    lib, seen = _lib.load(), []

    class Noting(object):
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in ("advchain_bias_field_bwd_reduced", "advchain_bias_field_bwd"):
                return fn

            def call(*a):
                rc = fn(*a)
                seen.append((name, rc))
                return rc
            return call
    monkeypatch.setattr(_lib, "load", lambda: Noting())
    _check_against_float64(tables, cp, data, gout, 0.2, True, 1.0)
    assert seen == [("advchain_bias_field_bwd_reduced", -2), ("advchain_bias_field_bwd", 0)], seen


@pytest.mark.parametrize("reduced", [True, False], ids=["reduced", "two_launches"])
@pytest.mark.parametrize("cp_scale", [1.0, 1e-6])
@pytest.mark.parametrize("use_log", [True, False], ids=["log", "linear"])
@pytest.mark.parametrize("shape,spacing", SHAPES, ids=IDS)
def test_against_float64(shape, spacing, use_log, cp_scale, reduced, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "BIAS_REDUCED", reduced)
    tables, _ = _geometry(shape, spacing)
    cp, data, gout, eps = _case(shape, spacing, use_log, cp_scale)
    _check_against_float64(tables, cp, data, gout, eps, use_log, cp_scale)


@pytest.mark.parametrize("shape,spacing", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_a_nan_row_stays_in_its_row(shape, spacing):
    """every voxel passes the clamp here (eps = 10), so each coefficient's band of the row holds a NaN"""
    tables, _ = _geometry(shape, spacing)
    cp, data, gout, _ = _case(shape, spacing, True, 1.0)
    gout = gout.clone()
    gout[0, 0, ..., 3, :] = float("nan")
    a = two_launches(tables, cp, data, gout, 10.0, True, 1.0)[0]
    b = fused(tables, cp, data, gout, 10.0, True, 1.0)[0]
    assert torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)
    for t in (a, b):
        nan = torch.isnan(t)
        assert bool(nan[0, 0, ..., 3, :].all())
        nan[0, 0, ..., 3, :] = False
        assert not bool(nan.any()) and bool(torch.isfinite(t[1:]).all())
