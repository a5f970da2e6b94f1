"""The band tables of the row-blended kernels by 16-byte requests (fields.hip: tp_run with WB = 2 or 4) against the dword
loads (WB = 0), in one process: ops.set_tp_wide_loads(False) keeps every launch on the dword form.

The contract is bit-identity -- the same table values reach the same sums in the same order -- so every comparison is
torch.equal on the int32 view (NaN and inf included).  The shapes are the smallest that reach each branch: rows of 2, 3, 16,
64 and 65 column groups (the last one reloads its bands for a second group), rows that are no multiple of 4 (one voxel a
thread: untouched), row counts of 1, 5, 33 and 37 with every rows_per_wg of the bias entries, a leading axis of 3, bands of 2
and 4 and bands that are neither, 1 and 3 planes, tables at an odd element offset of a larger buffer."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (0, 4, 8, 16, 32)


def _ops():
    from advchain_amd import ops
    return ops


def _band_matrix(S, g, B, seed):
    """(S, g) matrix with exactly B consecutive non-zeros a row, the first at a start that walks from 0 to g - B"""
    rng = np.random.RandomState(seed)
    M = np.zeros((S, g))
    for o in range(S):
        st = 0 if S == 1 else (o * (g - B)) // (S - 1)
        M[o, st:st + B] = rng.uniform(0.1, 1.0, B) * rng.choice([-1.0, 1.0], B)
    return M


# name -> (full size S, low-resolution grid g, band per axis, batch N, band form expected of a VEC = 4 launch)
GEOMETRIES = {
    "37x256_g16x16_b2_n3": ((37, 256), (16, 16), (2, 2), 3, 2),
    "33x260_g5x7_b4_n1": ((33, 260), (5, 7), (4, 4), 1, 4),
    "5x64_g4x4_b4_n3": ((5, 64), (4, 4), (4, 4), 3, 4),
    "37x12_g5x7_b2x4_n3": ((37, 12), (5, 7), (2, 4), 3, 4),
    "1x8_g4x4_b2_n1": ((1, 8), (4, 4), (2, 2), 1, 2),
    "33x10_g4x4_b4_n3": ((33, 10), (4, 4), (4, 4), 3, 4),          # S2 % 4 != 0: one voxel a thread, dword loads whatever B
    "37x256_g16x16_b3_n1": ((37, 256), (16, 16), (3, 3), 1, 0),    # a band that is neither 2 nor 4
    "5x128_g4x3_b4x3_n3": ((5, 128), (4, 3), (4, 3), 3, 0),        # a grid narrower than the cubic band
    "3x33x256_g2x5x16_b2_n1": ((3, 33, 256), (2, 5, 16), (2, 2, 2), 1, 2),
    "3x5x64_g4x4x16_b4_n3": ((3, 5, 64), (4, 4, 16), (4, 4, 4), 3, 4),
    "33x256_g4x4_b4x2_n3": ((33, 256), (4, 4), (4, 2), 3, 2),
}


@functools.lru_cache(maxsize=None)
def _tables(name, odd_offset=False):
    from advchain_amd import bands
    S, g, B, _, _ = GEOMETRIES[name]
    t = bands.BandTables([_band_matrix(s, gg, b, 11 + 7 * a) for a, (s, gg, b) in enumerate(zip(S, g, B))], torch.device(DEV))
    assert tuple(t.B[3 - len(S):]) == tuple(B), t.B
    if odd_offset:      # the same tables as views that start one element into a larger buffer: 4-byte aligned, no more
        t = copy.copy(t)
        for attr in ("itab", "ftab"):
            src = getattr(t, attr)
            big = torch.zeros(src.numel() + 7, dtype=src.dtype, device=DEV)
            big[1:1 + src.numel()] = src
            view = big[1:1 + src.numel()]
            assert view.data_ptr() % 16 == 4
            setattr(t, attr, view)
    return t


def _args(ops, tables):
    from advchain_amd import _lib
    return (ops._ptr(tables.itab), ops._ptr(tables.ftab), _lib.dims_array(tables.S), _lib.dims_array(tables.g),
            _lib.dims_array(tables.B))


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Form(object):
    """with _Form(wide): every launch inside takes that form of the table loads"""

    def __init__(self, wide):
        self.wide = wide

    def __enter__(self):
        ops = _ops()
        self.was = ops.tp_wide_loads()
        ops.set_tp_wide_loads(self.wide)

    def __exit__(self, *exc):
        _ops().set_tp_wide_loads(self.was)


def _both(fn):
    """fn() under the dword form and under the 16-byte form -> (dword results, wide results)"""
    with _Form(False):
        want = fn()
    with _Form(True):
        got = fn()
    torch.cuda.synchronize()
    return want, got


def _assert_same(want, got, what):
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert _same(a, b), (what, i)


def _coef(shape, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(shape, generator=g)
    if special:      # a NaN and both infinities in the first plane, away from each other
        flat = c.view(c.shape[0], -1)
        flat[0, 0] = float("nan")
        flat[0, flat.shape[1] // 2] = float("inf")
        flat[0, -1] = float("-inf")
    return c.to(DEV)


def test_the_switch_and_the_query():
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    assert ops.tp_wide_loads()      # the default
    assert [lib.advchain_tp_wide_band(b) for b in range(1, 9)] == [0, 2, 0, 4, 0, 0, 0, 0]
    with _Form(False):
        assert not ops.tp_wide_loads()
        assert [lib.advchain_tp_wide_band(b) for b in range(1, 9)] == [0] * 8
    assert ops.tp_wide_loads()
    for name, (S, g, B, N, form) in GEOMETRIES.items():
        assert lib.advchain_tp_wide_band(_tables(name).B[2]) == form, name


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_tp_interp_fwd(name):
    ops = _ops()
    S, g, B, N, _ = GEOMETRIES[name]
    d = len(S)
    for odd_offset, special in ((False, False), (True, False), (False, True)):
        tables = _tables(name, odd_offset)
        coef = _coef((N, d) + tuple(g), 5 + N, special)

        def run():
            disp = torch.zeros(ops.DISP_SLOTS, device=DEV)
            slots = torch.zeros(64, device=DEV)
            out = ops.raw_tp_interp(coef, tables, d, add_identity=True, scale=0.0625, disp_out=disp)
            plain = ops.raw_tp_interp(coef, tables, d)
            ops.raw_tp_interp(coef, tables, d, want_out=False, sumsq=slots)
            return out, plain, disp, (slots if N == 1 and S[-2] <= 32 and len(S) == 2 else None)      # (one workgroup: no atomic order)
        want, got = _both(run)
        _assert_same(want, got, "tp_interp_fwd odd=%s special=%s" % (odd_offset, special))
        if not special:
            assert bool(torch.isfinite(got[0]).all()) and float(got[1].abs().max()) > 0


@pytest.mark.parametrize("name", ["37x256_g16x16_b2_n3", "33x260_g5x7_b4_n1", "37x256_g16x16_b3_n1", "33x256_g4x4_b4x2_n3",
                                  "37x12_g5x7_b2x4_n3", "33x10_g4x4_b4_n3"])
def test_tp_interp_fwd_smoothed_pair(name):
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    S, g, B, N, _ = GEOMETRIES[name]
    for odd_offset in (False, True):
        tables = _tables(name, odd_offset)
        for special in (False, True):
            vel = _coef((N, 2) + tuple(g), 21 + N, special)

            def run():
                s1 = torch.empty((2 * N, 2) + tuple(g), device=DEV)
                out = torch.empty((2 * N, 2) + tuple(S), device=DEV)
                disp = torch.zeros(ops.DISP_SLOTS, device=DEV)
                rc = lib.advchain_tp_interp_fwd_smoothed_pair(ops._ptr(vel), ops._ptr(s1), ops._ptr(out), *_args(ops, tables), 2 * N, 2, 1,
                                                              0.0625, ops._ptr(disp), ops._GAUSS9, 1.5, ops._stream())
                assert rc == 0, rc
                return s1, out, disp
            want, got = _both(run)
            _assert_same(want, got, "smoothed_pair odd=%s special=%s" % (odd_offset, special))
            if not special:
                assert bool(torch.isfinite(got[1]).all())


def _bias_case(name, special):
    S, g, B, N, _ = GEOMETRIES[name]
    C = 2 if N == 3 else 1
    gen = torch.Generator().manual_seed(77 + N + S[-1])
    cp = _coef((N, 1) + tuple(g), 31 + N, special) * 0.3
    data = (torch.rand((N, C) + tuple(S), generator=gen) + 0.5).to(DEV)
    gout = torch.randn((N, C) + tuple(S), generator=gen).to(DEV)
    return cp, data, gout, C


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_bias_field_entries(name):
    """advchain_bias_field_fwd_rows / _bwd_rows / _bwd_reduced at every rows_per_wg, the tables packed and at an odd offset"""
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    S, g, B, N, _ = GEOMETRIES[name]
    eps, use_log, cp_scale = 0.25, 1, 1.0
    for odd_offset, special in ((False, False), (True, False), (False, True)):
        tables = _tables(name, odd_offset)
        cp, data, gout, C = _bias_case(name, special)
        wd, lo, WB = tables.dense_inner
        rows_list = ROWS if not (odd_offset or special) else (0, 8)

        def run():
            res = []
            for rows in rows_list:
                out, field = torch.empty_like(data), torch.empty((N, 1) + tuple(S), device=DEV)
                _lib.check(lib.advchain_bias_field_fwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(out), ops._ptr(field),
                                                            *_args(ops, tables), N, C, eps, use_log, cp_scale, rows, ops._stream()), "fwd")
                only = torch.empty((N, 1) + tuple(S), device=DEV)
                _lib.check(lib.advchain_bias_field_fwd_rows(ops._ptr(cp), None, None, ops._ptr(only),
                                                            *_args(ops, tables), N, 1, eps, use_log, cp_scale, rows, ops._stream()), "fwd")
                gL, gdata = torch.empty((N, 1) + tuple(S), device=DEV), torch.empty_like(data)
                _lib.check(lib.advchain_bias_field_bwd_rows(ops._ptr(cp), ops._ptr(data), ops._ptr(gout), ops._ptr(gL), ops._ptr(gdata),
                                                            *_args(ops, tables), N, C, eps, use_log, cp_scale, rows, ops._stream()), "bwd")
                t1 = torch.zeros((N, 1) + tuple(S[:-1]) + (int(tables.g[2]),), device=DEV)
                gd2 = torch.zeros_like(data)
                rc = lib.advchain_bias_field_bwd_reduced(ops._ptr(cp), ops._ptr(data), ops._ptr(gout), ops._ptr(t1), ops._ptr(gd2),
                                                         *_args(ops, tables), N, C, eps, use_log, cp_scale, ops._ptr(wd), ops._ptr(lo), WB,
                                                         rows, ops._stream())
                assert rc == (0 if S[-1] % 4 == 0 else -2), rc
                res += [out, field, only, gL, gdata, t1, gd2]
            return res
        want, got = _both(run)
        _assert_same(want, got, "bias odd=%s special=%s" % (odd_offset, special))
        if not special:
            assert all(bool(torch.isfinite(t).all()) for t in got)
            assert float(got[3].abs().max()) > 0 and float(got[1].min()) >= 1 - eps - 1e-6


def test_bias_apply_autograd():
    """ops.bias_apply forward and backward (the solver's path: the library's rows rule, the reduced backward)"""
    ops = _ops()
    name = "33x260_g5x7_b4_n1"
    tables = _tables(name)
    cp, data, gout, C = _bias_case(name, False)

    def run():
        a, b = cp.clone().requires_grad_(True), data.clone().requires_grad_(True)
        out, field = ops.bias_apply(a, b, tables, 0.25, True, 1.0)
        out.backward(gout)
        return out.detach(), field, a.grad, b.grad
    want, got = _both(run)
    _assert_same(want, got, "bias_apply")
    assert float(got[2].abs().max()) > 0


@pytest.mark.parametrize("low,full", [((16, 16), (64, 256)), ((5, 7), (33, 260))], ids=["16x16_64x256", "5x7_33x260"])
def test_demons_field_pair(low, full):
    """one paired 2D field, forward and backward, through the composite entry: linear upsampling tables (bands of 2)"""
    from advchain_amd import bands
    ops = _ops()
    tables = bands.upsample_tables(list(low), list(full), torch.device(DEV))
    assert tables.B[2] == 2
    g = torch.Generator().manual_seed(3)
    vel = torch.randn((3, 2) + low, generator=g)
    vel = (vel / vel.flatten(1).norm(dim=1).view(-1, 1, 1, 1)).to(DEV)
    gp = torch.randn((3, 2) + full, generator=g).to(DEV)
    gm = torch.randn((3, 2) + full, generator=g).to(DEV)
    was = ops.is_deterministic()
    ops.set_deterministic(True)      # the backward's scatters in their bit-reproducible form
    try:
        def run():
            a = vel.clone().requires_grad_(True)
            qp, qm = ops.demons_field_pair(a, 1.5, tables, False)
            ((qp * gp).sum() + (qm * gm).sum()).backward()
            return qp.detach(), qm.detach(), a.grad
        run()      # (the kernel-selection hints of this shape are in place for both forms)
        want, got = _both(run)
    finally:
        ops.set_deterministic(was)
    _assert_same(want, got, "demons_field_pair")
    assert bool(torch.isfinite(got[2]).all()) and float(got[2].abs().max()) > 0


@pytest.mark.parametrize("shape,spacing", [((3, 3, 32, 32), (16, 16)), ((2, 1, 24, 40), (8, 8)), ((2, 1, 8, 12, 16), (4, 4, 4))],
                         ids=["3x3x32x32", "2x1x24x40", "2x1x8x12x16"])
def test_bias_apply_with_the_transform_s_own_tables(shape, spacing):
    """the order-3 tables AdvBias builds (B-spline synthesis composed with the upsampling), through ops.bias_apply"""
    from advchain_amd.augmentor import AdvBias
    ops = _ops()
    cfg = dict(epsilon=0.3, control_point_spacing=list(spacing), downscale=2, data_size=list(shape), interpolation_order=3,
               init_mode="random", space="log")
    t = AdvBias(len(shape) - 2, cfg, device=torch.device(DEV))
    t.init_parameters()
    tables = t._tables
    gen = torch.Generator().manual_seed(9)
    cp = (torch.randn(tuple(t.param.shape), generator=gen) * 0.4).to(DEV)
    data = (torch.rand(shape, generator=gen) + 0.5).to(DEV)
    gout = torch.randn(shape, generator=gen).to(DEV)

    def run():
        a, b = cp.clone().requires_grad_(True), data.clone().requires_grad_(True)
        out, field = ops.bias_apply(a, b, tables, 0.3, True, 1.0)
        out.backward(gout)
        return out.detach(), field, a.grad, b.grad
    want, got = _both(run)
    _assert_same(want, got, "bias_apply %s" % (tables.B,))
    assert float(got[2].abs().max()) > 0


@pytest.mark.parametrize("name", ["37x256_g16x16_b2_n3", "33x260_g5x7_b4_n1", "33x10_g4x4_b4_n3"])
def test_smoothed_pair_rows_per_wg_gives_the_same_bits(name):
    """advchain_tp_interp_fwd_smoothed_pair_rows at every rows_per_wg, under either form, against the entry without the argument"""
    from advchain_amd import _lib
    ops, lib = _ops(), _lib.load()
    S, g, B, N, _ = GEOMETRIES[name]
    tables = _tables(name)
    vel = _coef((N, 2) + tuple(g), 41 + N)

    def run():
        res = []
        for rows in (None,) + ROWS:
            s1 = torch.empty((2 * N, 2) + tuple(g), device=DEV)
            out = torch.empty((2 * N, 2) + tuple(S), device=DEV)
            disp = torch.zeros(ops.DISP_SLOTS, device=DEV)
            head = (ops._ptr(vel), ops._ptr(s1), ops._ptr(out)) + _args(ops, tables) + (2 * N, 2, 1, 0.0625, ops._ptr(disp), ops._GAUSS9, 1.5)
            if rows is None:
                rc = lib.advchain_tp_interp_fwd_smoothed_pair(*head, ops._stream())
            else:
                rc = lib.advchain_tp_interp_fwd_smoothed_pair_rows(*head, rows, ops._stream())
            assert rc == 0, rc
            res.append((s1, out, disp.max().reshape(1)))      # (which slot a workgroup's maximum lands in depends on the grid)
        return res
    want, got = _both(run)
    for res in (want, got):
        for i in range(1, len(res)):
            _assert_same(res[0], res[i], "rows %s" % ((None,) + ROWS)[i])
    _assert_same(want[0], got[0], "forms")
    assert lib.advchain_tp_interp_fwd_smoothed_pair_rows(ops._ptr(vel), ops._ptr(want[0][0]), ops._ptr(want[0][1]), *_args(ops, tables),
                                                         2 * N, 2, 1, 0.0625, None, ops._GAUSS9, 1.5, 5, ops._stream()) == -1
