"""Host paths that look at the 16-byte alignment of their operands (include/advchain_hip.h): the entries that promise
ADVCHAIN_ERR_UNSUPPORTED (-2) with nothing enqueued for a misaligned operand, each operand moved alone, and the query forms that
promise not to look at pointers at all.  Fake addresses (multiples of 64: aligned; + 4, 8, 12 bytes: off): every call here returns
before anything is read or launched -- the all-aligned call, which would launch, is never made.  No GPU needed.  Also the layout
helpers and float64 references of tests/layout_cases.py against ATen and the oracle on the CPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from advchain_amd import _lib
from tests import layout_cases as L
from tests.helpers import maxdiff, rand

OK_ADDR = 64
OFF_ADDRS = (68, 72, 76)
W9 = _lib.float_array([0.1] * 9)


@pytest.fixture(scope="module")
def lib():
    from advchain_amd.build import build_library
    build_library()
    return _lib.load()


def _p(addr):
    return ctypes.c_void_p(addr)


def _moved(names, name, addr):
    """pointer arguments: every operand at an aligned fake address of its own (64, 128, ...: no two alias), `name` moved by
    addr - 64 bytes"""
    return {k: _p(OK_ADDR * (i + 1) + (addr - OK_ADDR if k == name else 0)) for i, k in enumerate(names)}


# ------------------------------------------------------------------------------------------------ refusals
GXY_DIMS = [(64, 256), (33, 80), (12, 20), (35, 20, 80)]


@pytest.mark.parametrize("addr", OFF_ADDRS)
@pytest.mark.parametrize("operand", ["in", "out", "aux", "in_hi"])
@pytest.mark.parametrize("dims", GXY_DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("entry", ["advchain_gauss_xy", "advchain_gauss_xy_staged", "advchain_gauss_xy_lanes"])
def test_gauss_xy_refuses_a_misaligned_operand(lib, entry, dims, operand, addr):
    """'Returns -2 (unsupported, no error text) for ... unaligned tensors': the shape is one the plan query takes."""
    nd = len(dims)
    planes = 2 * nd
    form, ty, nt = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.advchain_gauss_xy_plan(nd, _lib.dims_array(dims), planes, ctypes.byref(form), ctypes.byref(ty), ctypes.byref(nt)) == 0
    assert form.value in (1, 2)
    a = _moved(("in", "out", "aux", "in_hi"), operand, addr)
    post = 2 if nd == 2 else 0      # (aux is read by the epilogue of the last axis: 2D only)
    args = [a["in"], a["out"], a["aux"], planes, nd, nd, _lib.dims_array(dims), W9, 0, post, 1.0, None, a["in_hi"], nd]
    if entry.endswith("lanes"):
        args += [32, 512]
    assert getattr(lib, entry)(*args) == -2


@pytest.mark.parametrize("addr", OFF_ADDRS)
@pytest.mark.parametrize("operand", ["in", "in2"])
def test_band_reduce_rows_dense_refuses_a_misaligned_input(lib, operand, addr):
    a = _moved(("in", "in2"), operand, addr)
    assert lib.advchain_band_reduce_rows_dense(a["in"], a["in2"], _p(OK_ADDR), _p(OK_ADDR), _p(OK_ADDR), 128, 64, 8, 12, 1.0, None) == -2


def _tables3(S, g):
    return _lib.dims_array((1,) + tuple(S)), _lib.dims_array((1,) + tuple(g)), _lib.dims_array((1, 2, 2))


@pytest.mark.parametrize("addr", OFF_ADDRS)
@pytest.mark.parametrize("operand", ["pos", "q"])
def test_demons_compose_pair_fwd_refuses_before_anything_is_enqueued(lib, operand, addr):
    """'Returns ADVCHAIN_ERR_UNSUPPORTED (-2) with NOTHING enqueued': pos and q are what its x+y Gaussian reads and writes."""
    S3, g3, B3 = _tables3((64, 256), (4, 16))
    assert lib.advchain_gauss_xy_plan(2, _lib.dims_array((64, 256)), 8, *(ctypes.byref(ctypes.c_int()) for _ in range(3))) == 0
    a = _moved(("vel", "s1", "phi0", "fields", "pos", "q", "disp", "rows_max", "itab", "ftab"), operand, addr)
    rc = lib.advchain_demons_compose_pair_fwd(a["vel"], a["s1"], a["phi0"], a["fields"], a["pos"], a["q"], a["disp"], a["rows_max"],
                                              a["itab"], a["ftab"], S3, g3, B3, 2, 2, 4, None, W9, 1.0, 1.0 / 16, 1, None)
    assert rc == -2


@pytest.mark.parametrize("addr", OFF_ADDRS)
@pytest.mark.parametrize("operand", ["gq_lo", "gq_hi", "gpos", "pos"])
def test_demons_compose_pair_bwd_refuses_before_anything_is_enqueued(lib, operand, addr):
    S3, g3, B3 = _tables3((64, 256), (4, 16))
    names = ("gq_lo", "gq_hi", "pos", "phi0", "fields", "gpos", "g", "scratch", "ws", "t1", "gs1", "gvel", "itab", "ftab", "wd", "wlo")
    a = _moved(names, operand, addr)
    halos = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    rc = lib.advchain_demons_compose_pair_bwd(a["gq_lo"], a["gq_hi"], a["pos"], a["phi0"], a["fields"], a["gpos"], a["g"], a["scratch"],
                                              a["ws"], a["t1"], a["gs1"], a["gvel"], halos, a["itab"], a["ftab"], a["wd"], a["wlo"], 12,
                                              S3, g3, B3, 2, 2, 4, W9, 1.0, 1.0 / 16, None)
    assert rc == -2


# ------------------------------------------------------------------------------------------------ queries
def test_the_query_forms_take_no_pointers_and_answer_per_shape(lib):
    """advchain_expo_chain_fused_levels and advchain_gauss_xy_plan have no tensor arguments: what they say cannot depend on an
    alignment.  Their answers for the shapes tests/test_layout_gpu.py relies on: 16 fields of 256 x 64 with sub-pixel hints fuse
    at least two levels, the same fields in a batch of 8 (128 windows) and any 3D chain none."""
    for name in ("advchain_expo_chain_fused_levels", "advchain_gauss_xy_plan"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    sub = (ctypes.c_int32 * 4)(*[(300 << 8) | 1] * 4)      # 300 / 1024 px
    dims = _lib.dims_array((256, 64))
    assert lib.advchain_expo_chain_fused_levels(16, 2, dims, 4, sub) >= 2
    assert lib.advchain_expo_chain_fused_levels(16, 2, dims, 4, sub) == lib.advchain_expo_chain_fused_levels(16, 2, dims, 4, sub)
    assert lib.advchain_expo_chain_fused_levels(8, 2, dims, 4, sub) == 0
    assert lib.advchain_expo_chain_fused_levels(16, 2, dims, 4, None) == 0
    assert lib.advchain_expo_chain_fused_levels(16, 3, _lib.dims_array((6, 9, 80)), 4, sub) == 0
    form, ty, nt = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_int(0)
    want = {(64, 256): 2, (33, 80): 1, (12, 20): 1, (35, 20, 80): 1, (40, 12, 16): 1, (9, 11): 0}
    for d, f in want.items():
        assert lib.advchain_gauss_xy_plan(len(d), _lib.dims_array(d), 4, ctypes.byref(form), ctypes.byref(ty), ctypes.byref(nt)) == 0
        assert form.value == f, (d, form.value)


# ------------------------------------------------------------------------------------------------ the helpers themselves
@pytest.mark.parametrize("k", [1, 2, 3])
def test_offset_copy(k):
    t = rand((2, 3, 5, 8), 1)
    v = L.offset_copy(t, k)
    assert torch.equal(v, t) and v.is_contiguous() and v.data_ptr() % 16 == 4 * k and v.shape == t.shape


def test_strided_variants_are_the_same_values_and_not_contiguous():
    t = rand((2, 3, 5, 8), 2)
    got = L.strided_variants(t)
    assert [n for n, _ in got] == ["transposed", "channel_slice", "step2"]
    for _, v in got:
        assert torch.equal(v, t) and not v.is_contiguous()
    g = L.expanded_grad((2, 3, 5, 8), "cpu")
    assert not g.is_contiguous() and float(g.sum()) == 2 * 3 * 5 * 8


def test_gauss_ref_is_the_oracles_dense_gaussian():
    from advchain_amd import ops
    from oracle import advchain_oracle as O
    w = list(ops._GAUSS9)
    for shape in [(2, 2, 12, 20), (1, 3, 7, 9, 11)]:
        x = rand(shape, 3)
        assert maxdiff(L.gauss_ref(x, w), O.gaussian_smooth(x)) < 2e-6
        assert maxdiff(L.gauss_ref(x, w, pre=1, scale=-1.5), O.gaussian_smooth(-1.5 * x)) < 3e-6
        d = len(shape) - 2
        xd = x[:, :d]
        ident = O.identity_grid(shape[0], shape[2:])
        pos = ident * 1.05 + 0.1 * xd
        want = O.gaussian_smooth(O.compose_fields(ident, pos) - ident) + ident      # adv_morph.py:486-489
        assert maxdiff(L.gauss_ref(pos, w, pre=2, post=1), want) < 3e-6
        if d == 2:      # post 2 is the adjoint of pre 2
            p = pos.double().requires_grad_(True)
            g = rand(tuple(pos.shape), 4).double()
            (L._conv_axis(L._conv_axis(torch.clamp(p, -1, 1), w, 2), w, 3) * g).sum().backward()
            assert maxdiff(L.gauss_ref(g, w, post=2, aux=pos), p.grad) < 2 * 20 * 2.0 ** -24      # (the slope is the float32 one: rows of 20)


def test_sampler_references_are_aten_in_double():
    inp, grid = rand((2, 2, 6, 7), 5), rand((2, 6, 7, 2), 6, -1.2, 1.2)
    w = rand((2, 2, 6, 7), 7)
    a, g = inp.clone().requires_grad_(True), grid.clone().requires_grad_(True)
    ref = F.grid_sample(a, g, padding_mode="border", align_corners=True)
    (ref * w).sum().backward()
    out, gin, ggrid = L.grid_sample_ref(inp, L.to_planar(grid), w, pad="border")
    assert maxdiff(out, ref) < 1e-5 and maxdiff(gin, a.grad) < 1e-5 and maxdiff(ggrid, L.to_planar(g.grad)) < 1e-4
    from oracle import advchain_oracle as O
    assert maxdiff(L.identity_grid64(2, (5, 6, 7)), O.identity_grid(2, (5, 6, 7))) < 1e-6
    phi = O.identity_grid(2, (6, 7)) + 0.1 * rand((2, 2, 6, 7), 8)
    fields, pos, _ = L.chain_ref(phi, 2)
    want = O.compose_fields(phi, phi)
    assert maxdiff(fields[0], want) < 1e-5
    assert maxdiff(pos, O.compose_fields(want, want) - phi + O.identity_grid(2, (6, 7))) < 1e-5
