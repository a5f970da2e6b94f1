"""The lane form of the x+y Gaussian launch (k_gauss_xy_lanes: x taps from the neighbouring lanes, y taps from LDS) against the
staged form (k_gauss_xy): the same bits for every prologue / epilogue, the split input, every tile, NaN and inf included;
against a float64 separable convolution on the CPU; and through the solver."""
import ctypes

import pytest
import torch

from tests.helpers import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"

TILES = [(16, 256), (16, 512), (32, 256), (32, 512), (64, 1024)]
# (planes, dims): Q = 2 with every quad a row end and a tile shorter than TY; rows that are no multiple of TY with four rows
# a wave; 16 quads a row; one row a wave with a last tile of one row
SHAPES_2D = [(3, (8, 8)), (2, (20, 16)), (2, (40, 64)), (1, (33, 256))]
PRE_POST = [(pre, post) for pre in range(3) for post in range(3)]


def _lib_ops():
    from advchain_amd import _lib, ops
    return _lib, _lib.load(), ops


def _plan(dims, planes):
    _lib, lib, _ = _lib_ops()
    form, ty, nt = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.advchain_gauss_xy_plan(len(dims), _lib.dims_array(dims), planes, ctypes.byref(form), ctypes.byref(ty),
                                      ctypes.byref(nt)) == 0
    return form.value, ty.value, nt.value


def _inputs(planes, dims, pre, post, seed=7):
    """planes = batch x C with C = len(dims); positions around the identity for pre 2 and for aux"""
    from oracle import advchain_oracle as O
    d = len(dims)
    n = planes // d if planes % d == 0 else planes
    C = d if planes % d == 0 else 1
    ident = O.identity_grid(n, dims) if C == d else 0.0
    x = (rand((n, C) + tuple(dims), seed) * 0.5 + (ident if pre == 2 else 0)).contiguous().to(DEV)
    aux = ((ident * 1.05 if C == d else 0) + 0.1 * rand((n, C) + tuple(dims), seed + 1)).contiguous().to(DEV) if post == 2 else None
    return x, aux, C


def _entry(which, x, aux, C, pre, post, x_hi=None, ty=0, nt=0, scale=1.5):
    """One of the three C entries on (x[, x_hi]); returns (rc, out)."""
    _lib, lib, ops = _lib_ops()
    dims = tuple(x.shape[2:])
    planes = x.shape[0] * x.shape[1] + (x_hi.shape[0] * x_hi.shape[1] if x_hi is not None else 0)
    out = torch.full((planes,) + dims, float("nan"), device=DEV)
    a = (ops._ptr(x), ops._ptr(out), ops._ptr(aux), planes, C, len(dims), _lib.dims_array(dims), ops._GAUSS9, pre, post,
         scale if pre == 1 else 1.0, ops._stream(), ops._ptr(x_hi), x.shape[0] * x.shape[1])
    if which == "lanes":
        rc = lib.advchain_gauss_xy_lanes(*a, ty, nt)
    else:
        rc = getattr(lib, "advchain_gauss_xy" if which == "auto" else "advchain_gauss_xy_staged")(*a)
    torch.cuda.synchronize()
    return rc, out


RULE_TILE = (32, 512)      # the tile advchain_gauss_xy runs for rows of 256 voxels (the plan says so below)


def _lane(x, aux, C, pre, post, x_hi=None, scale=1.5):
    """The lane form at the rule's tile.  advchain_gauss_xy runs it by itself for rows of 256 voxels only (where it was
    measured to win); the shapes at which the form can go wrong are narrower, so the tile is forced through
    advchain_gauss_xy_lanes, and where the plan says lanes the default entry must give the same bits."""
    dims = tuple(x.shape[2:])
    planes = x.shape[0] * x.shape[1] + (x_hi.shape[0] * x_hi.shape[1] if x_hi is not None else 0)
    form, ty, nt = _plan(dims, planes)
    assert form == (2 if dims[-1] == 256 else 1)
    rc, out = _entry("lanes", x, aux, C, pre, post, x_hi=x_hi, ty=RULE_TILE[0], nt=RULE_TILE[1], scale=scale)
    if form == 2:
        assert (ty, nt) == (min(RULE_TILE[0], (dims[-2] + 7) // 8 * 8), RULE_TILE[1])
        rc_a, out_a = _entry("auto", x, aux, C, pre, post, x_hi=x_hi, scale=scale)
        assert rc_a == rc and _same_bits(out_a, out)
    return rc, out


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("planes,dims", SHAPES_2D)
@pytest.mark.parametrize("pre,post", PRE_POST)
def test_lane_form_equals_staged_form(planes, dims, pre, post):
    """The lane form against advchain_gauss_xy_staged, for the single input and for the input in two halves; and ops.raw_gauss
    with GAUSS_XY_LANES on and off (the default entry against the staged one: the lane form for rows of 256 voxels)."""
    _, _, ops = _lib_ops()
    x, aux, C = _inputs(planes, dims, pre, post)
    flat = x.reshape((1, -1) + tuple(dims))
    a = aux.reshape(flat.shape) if aux is not None else None
    rc_s, out_s = _entry("staged", flat, a, C, pre, post)
    rc_l, out_l = _lane(flat, a, C, pre, post)
    assert rc_s == 0 and rc_l == 0
    assert _same_bits(out_l, out_s)
    assert bool(torch.isfinite(out_l).all())
    if planes >= 2:                            # the same planes as two tensors (in / in_hi)
        lo, hi = flat[:, :1].contiguous(), flat[:, 1:].contiguous()
        rc_s2, out_s2 = _entry("staged", lo, a, C, pre, post, x_hi=hi)
        rc_l2, out_l2 = _lane(lo, a, C, pre, post, x_hi=hi)
        assert rc_s2 == 0 and rc_l2 == 0
        assert _same_bits(out_l2, out_s2) and _same_bits(out_l2, out_l)
    res = {}
    for lanes in (True, False):
        ops.GAUSS_XY_LANES = lanes
        try:
            res[lanes] = ops.raw_gauss(x, C, pre=pre, post=post, scale=1.5, aux=aux)
        finally:
            ops.GAUSS_XY_LANES = True
    assert torch.equal(res[True], res[False])
    if post != 0:
        assert _same_bits(res[True].reshape(out_l.shape), out_l)


@pytest.mark.parametrize("ty,nt", TILES)
@pytest.mark.parametrize("planes,dims,pre,post", [(2, (72, 256), 2, 1), (2, (72, 256), 0, 2), (3, (70, 32), 1, 0), (3, (8, 8), 2, 2)])
def test_every_tile_equals_staged_form(ty, nt, planes, dims, pre, post):
    """Each (rows, threads) the lane form is built for, forced through advchain_gauss_xy_lanes: 72 rows of 256 are more than
    one workgroup at every tile, with a last tile of 8 rows; 70 rows of 32 leave items past the last quad in the last round;
    8 x 8 is shorter than every tile.  The tile the rule chooses is among them."""
    x, aux, C = _inputs(planes, dims, pre, post, seed=11)
    flat = x.reshape((1, -1) + tuple(dims))
    a = aux.reshape(flat.shape) if aux is not None else None
    rc_s, out_s = _entry("staged", flat, a, C, pre, post)
    rc_l, out_l = _entry("lanes", flat, a, C, pre, post, ty=ty, nt=nt)
    assert rc_s == 0 and rc_l == 0
    assert _same_bits(out_l, out_s)
    assert RULE_TILE in TILES


def test_nan_and_inf_give_the_same_bits():
    _, _, ops = _lib_ops()
    x, _, C = _inputs(2, (24, 128), 0, 0, seed=3)
    x[0, 0, 5, 17] = float("nan")
    x[0, 1, 23, 127] = float("inf")
    x[0, 1, 0, 0] = float("-inf")
    rc_s, out_s = _entry("staged", x, None, C, 0, 0)
    rc_l, out_l = _lane(x, None, C, 0, 0)
    assert rc_s == 0 and rc_l == 0
    assert _same_bits(out_l, out_s)
    assert bool(torch.isnan(out_l).any()) and bool(torch.isinf(out_l).any())


@pytest.mark.parametrize("pre,post", [(0, 0), (1, 0), (2, 1), (0, 2)])
def test_3d_xy_launch_then_z_pass(pre, post):
    """2 planes of 5 x 12 x 32 (C = 1: channel 0 is x): the xy launch alone at the C entries, and through raw_gauss with the z
    pass behind it (an epilogue keeps raw_gauss off the small-plane kernel)."""
    _, _, ops = _lib_ops()
    dims = (5, 12, 32)
    x = rand((2, 1) + dims, 21).mul(0.5).contiguous().to(DEV)
    aux = rand((2, 1) + dims, 22).mul(1.1).contiguous().to(DEV) if post == 2 else None
    rc_s, out_s = _entry("staged", x, None, 1, pre, 0)
    rc_l, out_l = _lane(x, None, 1, pre, 0)
    assert rc_s == 0 and rc_l == 0 and _same_bits(out_l, out_s)
    res = {}
    for lanes in (True, False):
        ops.GAUSS_XY_LANES = lanes
        try:
            res[lanes] = ops.raw_gauss(x, 1, pre=pre, post=post, scale=1.5, aux=aux)
        finally:
            ops.GAUSS_XY_LANES = True
    assert torch.equal(res[True], res[False])


@pytest.mark.parametrize("planes,dims,form", [(2, (16, 80), 1), (1, (16, 512), 0)])
def test_fallback_shapes_keep_their_kernels(planes, dims, form):
    """Rows of 80 voxels (quads that do not divide a wave): the plan says staged.  Rows of 512 voxels: the staged kernel's
    smallest tile (8 rows) is 66048 bytes, above 64 KiB, so the plan says the per-axis passes, as before.
    advchain_gauss_xy_lanes refuses both, both entries return the same code and the same bits, and so do both settings of
    raw_gauss."""
    _, _, ops = _lib_ops()
    assert _plan(dims, planes)[0] == form
    x, _, C = _inputs(planes, dims, 1, 0)
    flat = x.reshape((1, -1) + tuple(dims))
    assert _entry("lanes", flat, None, C, 1, 0, ty=16, nt=256)[0] == -2
    rc_a, out_a = _entry("auto", flat, None, C, 1, 0)
    rc_s, out_s = _entry("staged", flat, None, C, 1, 0)
    assert rc_a == rc_s == (0 if form else -2) and _same_bits(out_a, out_s)
    res = {}
    for lanes in (True, False):
        ops.GAUSS_XY_LANES = lanes
        try:
            res[lanes] = ops.raw_gauss(x, C, pre=2, post=1)
        finally:
            ops.GAUSS_XY_LANES = True
    assert torch.equal(res[True], res[False])


def _conv64(x, w, axes):
    """zero-padded separable 9-tap convolution in float64"""
    y = x.double()
    for ax in axes:
        pad = [0, 0] * y.dim()
        acc = torch.zeros_like(y)
        S = y.shape[ax]
        for k in range(-4, 5):
            lo, hi = max(0, -k), min(S, S - k)            # out[i] += w[k+4] * in[i+k]
            if hi > lo:
                acc.narrow(ax, lo, hi - lo).add_(w[k + 4] * y.narrow(ax, lo + k, hi - lo))
        y = acc
    return y


@pytest.mark.parametrize("planes,dims", [(2, (40, 64)), (1, (33, 256))])
def test_lane_form_against_float64(planes, dims):
    """The tolerance of tests/test_ops_gpu.py::test_gauss_separable_vs_dense (2e-6 for inputs in [-1, 1), 3e-6 scaled by 1.5)."""
    _, _, ops = _lib_ops()
    x = rand((1, planes) + tuple(dims), 41)
    w = [float(v) for v in ops._GAUSS9]
    rc, out = _lane(x.to(DEV), None, 1, 0, 0)
    assert rc == 0
    assert maxdiff(out.cpu(), _conv64(x, w, (2, 3))[0]) < 2e-6
    rc, out2 = _lane(x.to(DEV), None, 1, 1, 0, scale=-1.5)
    assert rc == 0
    assert maxdiff(out2.cpu(), _conv64(-1.5 * x, w, (2, 3))[0]) < 3e-6


@pytest.mark.parametrize("dims,vs,form", [((64, 64), [4, 4], 1), ((64, 256), [4, 16], 2)])
def test_solver_step_same_bits_with_and_without_lanes(dims, vs, form):
    """Batch 2, the full 2D chain, two ascent steps in deterministic mode: the composite DemonsCompose entries
    (advchain_demons_compose_pair_*) run, and the loss and every parameter are torch.equal for GAUSS_XY_LANES on, off, and
    off with the separate calls (COMPOSITE off: every x+y launch of the step is then the staged kernel).  At 64 x 64 the
    paired field keeps the staged kernel either way; at 64 x 256 the default is the lane form."""
    from advchain_amd import _lib, ops
    from advchain_amd.augmentor import AdvAffine, AdvBias, AdvMorph, AdvNoise, ComposeAdversarialTransformSolver
    lib = _lib.load()
    ds = [2, 1] + list(dims)
    assert _plan(dims, 2 * 2 * 2)[0] == form
    cfgs = [
        (AdvNoise, dict(epsilon=1.0, xi=1e-6, data_size=ds)),
        (AdvBias, dict(epsilon=0.3, control_point_spacing=[32, 32], downscale=2, data_size=ds, interpolation_order=3,
                       init_mode="random", space="log")),
        (AdvMorph, dict(epsilon=1.5, data_size=ds, vector_size=vs)),
        (AdvAffine, dict(rot=30 / 180., scale_x=0.2, scale_y=0.2, shift_x=0.1, shift_y=0.1, data_size=ds)),
    ]
    torch.manual_seed(0)
    model = torch.nn.Conv2d(1, 4, 3, 1, 1).eval().to(DEV)
    data = torch.nn.functional.interpolate(torch.rand(2, 1, 6, 6), size=ds[2:], mode="bilinear", align_corners=True).contiguous().to(DEV)
    init = None
    res = {}
    for lanes, comp in ((True, True), (False, True), (False, False)):
        ops.GAUSS_XY_LANES, ops.COMPOSITE = lanes, comp
        ops._CHAIN_HINTS.clear()
        try:
            chain = [cls(2, cfg, device=torch.device(DEV)) for cls, cfg in cfgs]
            for t in chain:
                t.init_parameters()
            if init is None:
                init = [t.param.detach().clone() for t in chain]
            for t, p in zip(chain, init):
                t.set_parameters(p.clone())
            solver = ComposeAdversarialTransformSolver(chain_of_transforms=chain)
            solver.deterministic = True
            calls = []
            if lanes:
                with lib.timed(names=("advchain_demons_compose_pair_fwd", "advchain_demons_compose_pair_bwd")):
                    loss = solver.adversarial_training(data=data, model=model, n_iter=2, lazy_load=True)
                calls = sorted(set(r[0] for r in lib.records))
                del lib.records[:]
                assert calls == ["advchain_demons_compose_pair_bwd", "advchain_demons_compose_pair_fwd"], calls
            else:
                loss = solver.adversarial_training(data=data, model=model, n_iter=2, lazy_load=True)
            torch.cuda.synchronize()
            res[(lanes, comp)] = [torch.as_tensor(loss).detach().clone()] + [t.param.detach().clone() for t in chain]
        finally:
            ops.GAUSS_XY_LANES, ops.COMPOSITE = True, True
            ops.set_deterministic(False)
    for key in ((False, True), (False, False)):
        for a, b in zip(res[(True, True)], res[key]):
            assert torch.equal(a, b), key
