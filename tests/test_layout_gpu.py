"""Solver-path operators on operands the rest of the suite never hands them: contiguous tensors 4, 8 or 12 bytes off a 16-byte
boundary (part A: one operand moved at a time, then all of them by different amounts), non-contiguous inputs and incoming
gradients (part B), and batches of 1 and 5 whose entries must not depend on their neighbours (part C).

Every run is held to a float64 reference on the CPU (tests/layout_cases.py) within the bound the existing test of the same entry
uses (named beside each constant), and to the bits of its control run wherever DESIGN / LESSONS call the formulations involved
bit-identical: the forward samplers, the fused 2D chain against the per-squaring launches, the deterministic-mode scatters,
the reduced bias backward against its two launches, the gather-form Jacobian backwards, max reductions.  Where the two runs
may take formulations that sum in another order (tile against march against owner-computes scatter, float-atomic window
scatter, x+y Gaussian launch against the per-axis passes, k_norm_axpy against k_update_multi) only the reference bound holds and
the measured difference from the control is noted (printed at the end of the module with the backward routes taken: -s shows it).

The shapes are the smallest that cross each alignment gate at row lengths that ARE multiples of 4 -- 16, 64, 72, 80, 128, 132,
256 -- where only the base pointer can make a row misaligned."""
import ctypes
import json

import pytest
import torch
import torch.nn.functional as F

from tests import jacobian_forms as JF
from tests import layout_cases as L
from tests.helpers import maxdiff, rand

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOL = 2e-5                 # values: tests/test_ops_gpu.py TOL
G_SAMPLER = 5e-5           # x max(1, |g|max): sampler gradients, test_grid_sample_bwd_gather_form
G_CHAIN = 5e-4             # x max(1, |g|max): chained adjoints -- 2e-4 after two, 5e-4 after three steps in test_scatter_march_3d_exact_bounds
#                            and test_window_scatter_3d (each step differentiates the float32 fields of the step before); the
#                            four steps here are held to the three-step figure
G_BICUBIC = 1e-4          # x max(1, |g|max): bicubic grad_grid, test_deterministic_gpu / test_det_complete_gpu
G_THETA = (2e-5, 5e-5)     # relative, grad_theta: test_affine_warp (plain, 8 x minification)
AXPY = 1e-6                # test_axpy_and_normalized_update
GAUSS = (2e-6, 3e-6)       # test_gauss_separable_vs_dense (plain, with a prologue); x max(1, |ref|max) for the identity epilogue
GAUSS_FORMS = 5e-7         # x max(1, |ref|max): x+y launch against per-axis passes, test_gauss_xy_launch_equals_the_per_axis_passes
TP = (2e-6, 2e-5)          # test_tp_interp_upsample_and_adjoint: values absolute, adjoint relative

FIGURES = {}               # entry -> {"case/operand": "bit-equal" | measured max difference from the control}


def _ops():
    from advchain_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    print("\nLAYOUT_FIGURES " + json.dumps(FIGURES, sort_keys=True))


def note(entry, key, got, control):
    """bit-equal, or the largest difference from the control (information: the assertion is the caller's)"""
    d = FIGURES.setdefault(entry, {})
    same = all(torch.equal(a, b) for a, b in zip(got, control))
    worst = max(maxdiff(a, b) for a, b in zip(got, control))
    prev = d.get(key, "bit-equal")
    d[key] = "bit-equal" if (same and prev == "bit-equal") else max(worst, 0.0 if prev == "bit-equal" else prev)
    return same


def note_route(entry, key, route):
    r = FIGURES.setdefault(entry + ".routes", {}).setdefault(key, [])
    if route not in r:
        r.append(route)


def moves(operands):
    """("control", operands), then each tensor operand alone one element into a fresh storage, then all of them 1, 2, 3, 1 ..
    elements in"""
    yield "control", dict(operands)
    names = [k for k, t in operands.items() if t is not None]
    for k in names:
        m = dict(operands)
        m[k] = L.offset_copy(operands[k], 1)
        yield k, m
    m = dict(operands)
    for i, k in enumerate(names):
        m[k] = L.offset_copy(operands[k], 1 + i % 3)
    yield "all", m


def gbound(g, c=G_SAMPLER):
    return c * max(1.0, float(g.abs().max()))


def ident(n, dims):
    from oracle import advchain_oracle as O
    return O.identity_grid(n, dims)


def smooth_field(dims, amp_vox, seed, n=2):
    """identity + a smooth displacement of at most amp_vox voxels along every axis (tests/test_ops_gpu._smooth_field)"""
    d = len(dims)
    low = rand((n, d) + tuple(max(2, s // 8) for s in dims), seed)
    up = F.interpolate(low, size=dims, mode="trilinear" if d == 3 else "bilinear", align_corners=True)
    up = up / up.abs().amax(dim=tuple(range(1, d + 2)), keepdim=True)
    scale = torch.tensor([2.0 * amp_vox / (dims[d - 1 - a] - 1) for a in range(d)]).view(1, d, *([1] * d))
    return (ident(n, dims) + up * scale).contiguous()


def drift_field(dims, lo, hi, seed, n=2):
    """identity + a smooth displacement between lo and hi voxels (both positive) along every axis.  The coordinate gradient
    of a linear sampler jumps where a position crosses a voxel centre: a displacement that passes through zero puts some
    positions within rounding of their own voxel, float32 and float64 then differentiate different cells, and four chained
    adjoints are off by 1 % of the gradient's maximum on a field that is right to 1e-7 (measured with float32 autograd through
    the oracle against float64: 0.19 of 25 at 6 x 9 x 80).  A one-sided drift keeps every position of every squaring inside
    its cell (or unambiguously beyond the border), where float64 is a reference for the gradient."""
    d = len(dims)
    low = rand((n, d) + tuple(max(2, s // 8) for s in dims), seed)
    up = F.interpolate(low, size=dims, mode="trilinear" if d == 3 else "bilinear", align_corners=True)
    up = up / up.abs().amax(dim=tuple(range(1, d + 2)), keepdim=True)
    vox = 0.5 * (lo + hi) + 0.5 * (hi - lo) * up
    scale = torch.tensor([2.0 / (dims[d - 1 - a] - 1) for a in range(d)]).view(1, d, *([1] * d))
    return (ident(n, dims) + vox * scale).contiguous()


def sid(dims):
    return "x".join(map(str, dims))


# ================================================================================================ A: grid_sample
PADS = [("zeros", True), ("zeros", False), ("border", False)]
FIELDS_3D = [("amp", 0.004, None), ("amp", 0.5, None), ("vox", 2.7, 3), ("vox", 3.6, 4), ("vox", 7.5, 8)]
FIELDS_2D = [("vox", 0.5, 1), ("vox", 3.3, 4), ("vox", 26.0, 32)]


def _grid(dims, field, n=2):
    kind, amp, bound = field
    if kind == "amp":      # a little beyond [-1, 1] (test_grid_sample_bwd_gather_form)
        return (ident(n, dims) * 1.02 + amp * rand((n, len(dims)) + dims, 41)).contiguous()
    return smooth_field(dims, amp, 61, n)


def _halos(ops, grid, field, d):
    """the product's own choice for this grid (ops.warp_halo), the same number as a hint (tile kernels with an overflow list),
    no bound at all, and the exact bound the existing exact-bound tests hand the C ABI"""
    measured = float(ops.raw_max_displacement(grid.to(DEV)).item())
    policy = ops._warp_halo_of(measured, d)
    hs = [0, policy, abs(policy)]
    if field[2] is not None:
        assert measured < field[2] - 0.001, measured
        if d == 3 or field[2] <= 16:      # (2D image warps: exact bounds up to 16 px -- test_scatter_rows_2d_exact_bounds)
            hs.append(-field[2])
    out = []
    for h in hs:
        if h not in out:
            out.append(h)
    return out, measured


def _sampler_case(entry, dims, C, field, deterministic=False):
    ops = _ops()
    d = len(dims)
    grid = _grid(dims, field)
    # TOL is absolute: it presumes |d out / d position| x the rounding of a position stays below it.  A position near 255 is
    # rounded to 2^-17 voxels per operation, and white noise in [-1, 1] has slopes of up to 2 a voxel (measured on the control:
    # 2.6e-5 at rows of 256) -- rows that long get an image of half the amplitude, every other shape the one of test_ops_gpu
    inp, gout = rand((2, C) + dims, 42) * (0.5 if dims[-1] >= 256 else 1.0), rand((2, C) + dims, 43)
    halos, measured = _halos(ops, grid, field, d)
    case = "%s/C%d/%s%g" % (sid(dims), C, field[0], field[1])
    base = dict(inp=inp.to(DEV), grid=grid.to(DEV), gout=gout.to(DEV))
    for pad, clamp in PADS:
        ref_out, ref_gin, ref_gg = L.grid_sample_ref(inp, grid, gout, pad=pad, clamp=clamp)
        control = {}
        for name, m in moves(base):
            tag = (name, pad, clamp)
            out = ops.raw_grid_sample_fwd(m["inp"], m["grid"], 0, ops.pad_code(pad), clamp)
            hinted = ops.raw_grid_sample_fwd(m["inp"], m["grid"], 0, ops.pad_code(pad), clamp, disp_hint=measured)
            assert maxdiff(out.cpu(), ref_out) < TOL, tag
            # "chosen from a displacement hint, results identical" (DESIGN section 2): whatever kernel either run took
            assert torch.equal(out, hinted), tag
            control.setdefault("out", out)
            assert torch.equal(out, control["out"]), tag
            for halo in halos:
                gin, gg = ops.raw_grid_sample_bwd(m["gout"], m["inp"], m["grid"], 0, ops.pad_code(pad), clamp, True, True, halo)
                route = ops.last_bwd_route()
                note_route(entry, "%s/halo%d/%s" % (case, halo, "control" if name == "control" else "offset"), route)
                assert maxdiff(gin.cpu(), ref_gin) < gbound(ref_gin), tag + (halo, route)
                assert maxdiff(gg.cpu(), ref_gg) < gbound(ref_gg), tag + (halo, route)
                gin2, none = ops.raw_grid_sample_bwd(m["gout"], m["inp"], m["grid"], 0, ops.pad_code(pad), clamp, True, False, halo)
                assert none is None and maxdiff(gin2.cpu(), ref_gin) < gbound(ref_gin), tag + (halo, "no grad_grid")
                c = control.setdefault(halo, (gin, gg))
                same = note(entry, "%s/halo%d/%s" % (case, halo, name), (gin, gg), c)
                if deterministic:      # fixed-point accumulation: no sum depends on an order, whichever kernel ran
                    assert same or route not in ("window_int64", "window_staged"), tag + (halo, route)


@pytest.mark.parametrize("field", FIELDS_3D, ids=lambda f: "%s%g" % (f[0], f[1]))
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("dims", [(5, 7, 16), (10, 12, 64), (6, 10, 72), (5, 9, 80), (4, 6, 132)], ids=sid)
def test_a_grid_sample_3d(dims, C, field):
    _sampler_case("grid_sample_3d", dims, C, field)


@pytest.mark.parametrize("field", FIELDS_2D, ids=lambda f: "%s%g" % (f[0], f[1]))
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("dims", [(24, 40), (40, 72), (64, 256)], ids=sid)
def test_a_grid_sample_2d(dims, C, field):
    _sampler_case("grid_sample_2d", dims, C, field)


@pytest.mark.parametrize("C", [1, 4])
def test_a_grid_sample_2d_deterministic_mode(C):
    """the staged window merge and the int64 twin with offset gout / inp / grid: equal bits whatever moved"""
    ops = _ops()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        for staged in (True, False):
            old, ops.WINDOW_STAGED = ops.WINDOW_STAGED, staged
            try:
                _sampler_case("grid_sample_2d_det_%s" % ("staged" if staged else "int64"), (40, 72), C, ("vox", 26.0, 32), True)
            finally:
                ops.WINDOW_STAGED = old
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("C", [1, 4])
def test_a_grid_sample_bicubic(C, deterministic):
    ops = _ops()
    dims = (32, 40)
    grid = _grid(dims, ("amp", 0.05, None))
    inp, gout = rand((2, C) + dims, 42), rand((2, C) + dims, 43)
    was = ops.is_deterministic()
    ops.set_deterministic(deterministic)
    try:
        for pad in ("zeros", "border"):
            ref_out, ref_gin, ref_gg = L.grid_sample_ref(inp, grid, gout, mode="bicubic", pad=pad)
            control = None
            for name, m in moves(dict(inp=inp.to(DEV), grid=grid.to(DEV), gout=gout.to(DEV))):
                a, g = m["inp"].detach().requires_grad_(True), m["grid"].detach().requires_grad_(True)
                out = ops.grid_sample(a, g, "bicubic", pad)
                out.backward(m["gout"])
                assert maxdiff(out.detach().cpu(), ref_out) < TOL, (name, pad)
                assert maxdiff(a.grad.cpu(), ref_gin) < gbound(ref_gin), (name, pad)
                assert maxdiff(g.grad.cpu(), ref_gg) < gbound(ref_gg, G_BICUBIC), (name, pad)
                got = (out.detach(), a.grad, g.grad)
                control = control or got
                same = note("grid_sample_bicubic", "%s/C%d/%s/%s" % ("det" if deterministic else "atomic", C, pad, name), got, control)
                assert torch.equal(got[0], control[0]) and torch.equal(got[2], control[2]), (name, pad)
                assert same or not deterministic, (name, pad)
    finally:
        ops.set_deterministic(was)


# ================================================================================================ A: compose_self and the chain
@pytest.mark.parametrize("amp", [0.3, 2.6])
@pytest.mark.parametrize("dims", [(20, 28), (64, 256), (8, 12, 16), (9, 18, 64)], ids=sid)
def test_a_compose_self(dims, amp):
    ops = _ops()
    d = len(dims)
    phi = smooth_field(dims, amp, 11)
    phi0 = (ident(2, dims) + 0.01 * rand((2, d) + dims, 13)).contiguous()
    gout = rand((2, d) + dims, 12)
    ref_out, ref_g = L.compose_self_ref(phi, gout)
    ref_fin = (ref_out - phi0.double()) + L.identity_grid64(2, dims)
    measured = float(ops.raw_max_displacement(phi.to(DEV)).item())
    policy = ops.squaring_halo(measured, d)
    control = {}
    for name, m in moves(dict(phi=phi.to(DEV), phi0=phi0.to(DEV), gout=gout.to(DEV))):
        slots = torch.zeros(ops.DISP_SLOTS, device=DEV)
        out = ops.raw_compose_self_fwd(m["phi"], disp_out=slots)
        hinted = ops.raw_compose_self_fwd(m["phi"], disp_hint=measured)
        fin = ops.raw_compose_self_fwd(m["phi"], phi0=m["phi0"], final_mode=1)
        assert maxdiff(out.cpu(), ref_out) < TOL and maxdiff(fin.cpu(), ref_fin) < TOL, name
        c = control.setdefault("fwd", (out, fin, slots.max().reshape(1)))
        assert torch.equal(out, hinted) and torch.equal(out, c[0]) and torch.equal(fin, c[1]) and torch.equal(slots.max().reshape(1), c[2]), name
        for halo in dict.fromkeys([0, policy, abs(policy)]):
            ws = ops._scatter_workspace(2, dims, DEV)
            g = ops.raw_compose_self_bwd(m["gout"], m["phi"], ws, chain=False, halo=halo)
            assert maxdiff(g.cpu(), ref_g) < gbound(ref_g), (name, halo)
            note("compose_self_bwd", "%s/amp%g/halo%d/%s" % (sid(dims), amp, halo, name), (g,), control.setdefault(halo, (g,)))


def _chain_fwd(ops, m, n, hints, fuse):
    from advchain_amd import _lib
    phi0 = m["phi0"]
    N, d, dims = phi0.shape[0], phi0.dim() - 2, tuple(phi0.shape[2:])
    rows = torch.zeros(n + 2, ops.DISP_SLOTS, device=DEV)
    harr = None if hints is None else (ctypes.c_int32 * n)(*hints)
    m["fields"].fill_(float("nan"))
    m["pos"].fill_(float("nan"))
    _lib.check(_lib.load().advchain_expo_chain_fwd(ops._ptr(phi0), ops._ptr(m["fields"]), ops._ptr(m["pos"]), N, d, _lib.dims_array(dims),
                                                   n, ops._ptr(rows), harr, ops._ptr(rows[n + 1]) if fuse else None, ops._stream()),
               "expo_chain_fwd")
    torch.cuda.synchronize()
    return rows[:n + 1].max(1).values, float(rows[n + 1, 0])


def _chain_bwd(ops, m, n, halos):
    from advchain_amd import _lib
    phi0 = m["phi0"]
    N, d, dims = phi0.shape[0], phi0.dim() - 2, tuple(phi0.shape[2:])
    ws = ops._scatter_workspace(N, dims, DEV)
    m["g0"].fill_(float("nan"))
    m["scratch"].fill_(float("nan"))
    _lib.check(_lib.load().advchain_expo_chain_bwd(ops._ptr(m["gk"]), ops._ptr(phi0), ops._ptr(m["fields"]), ops._ptr(m["g0"]),
                                                   ops._ptr(m["scratch"]), ops._ptr(ws), (ctypes.c_int32 * n)(*halos), N, d,
                                                   _lib.dims_array(dims), n, ops._stream()), "expo_chain_bwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,dims,fused", [(16, (256, 64), True), (2, (6, 9, 80), False)], ids=["2d_16x256x64", "3d_6x9x80"])
def test_a_expo_chain(N, dims, fused):
    """advchain_expo_chain_fwd / _bwd, n = 4 sub-voxel squarings.  2D: 16 fields of 256 x 64 are the smallest batch the fused
    launch takes (rows of 64 pixels, 16 windows a field, 256 workgroups): the query says so, the control's flag stays down, and a
    run with phi0 or fields off a 16-byte boundary is refused by the fused launch and must give the same bits from the
    per-squaring launches."""
    from advchain_amd import _lib
    ops = _ops()
    d, n = len(dims), 4
    phi0 = drift_field(dims, 0.005, 0.04, 21, N)                 # at most 0.04 -> 0.64 voxels over the four squarings
    gk = rand((N, d) + dims, 22)
    hints = [1 | (1 << 8)] * n                                   # "known and tiny" (tests/test_fused2d_gpu._chain)
    levels = _lib.load().advchain_expo_chain_fused_levels(N, d, _lib.dims_array(dims), n, (ctypes.c_int32 * n)(*hints))
    assert (levels >= 2) if fused else (levels == 0), levels
    ref_fields, ref_pos, ref_g0 = L.chain_ref(phi0, n, gk)
    base = dict(phi0=phi0.to(DEV), fields=torch.empty((n - 1, N, d) + dims, device=DEV), pos=torch.empty((N, d) + dims, device=DEV),
                gk=gk.to(DEV), g0=torch.empty((N, d) + dims, device=DEV), scratch=torch.empty((N, d) + dims, device=DEV))
    control = None
    for name, m in moves(base):
        dm, flag = _chain_fwd(ops, m, n, hints, d == 2)
        assert flag == 0.0, (name, flag)
        for k in range(n - 1):
            assert maxdiff(m["fields"][k].cpu(), ref_fields[k]) < TOL, (name, k)
        assert maxdiff(m["pos"].cpu(), ref_pos) < TOL, name
        halos = [ops.squaring_halo(v, d) for v in reversed(dm.tolist()[:n])]
        assert halos == [-1] * n, halos
        _chain_bwd(ops, m, n, halos)
        assert maxdiff(m["g0"].cpu(), ref_g0) < gbound(ref_g0, G_CHAIN), name
        got = (m["fields"].clone(), m["pos"].clone(), dm.clone(), m["g0"].clone())
        control = control or got
        same = note("expo_chain", "%s/%s" % (sid(dims), name), got, control)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], control[:3])), name      # forward: bit-identical formulations
        if d == 2:      # fused sub-pixel tail of the backward against the per-squaring gather form: bit for bit (test_fused2d_gpu)
            assert same, name
    # the chain without hints never fuses: the same bits again
    dm, _ = _chain_fwd(ops, base, n, None, False)
    assert torch.equal(base["fields"], control[0]) and torch.equal(base["pos"], control[1]) and torch.equal(dm, control[2])


# ================================================================================================ A: affine_warp
def _theta(d, minify):
    theta = (torch.eye(d, d + 1).repeat(2, 1, 1) + 0.2 * rand((2, d, d + 1), 21)).contiguous()      # test_affine_warp
    if minify:
        theta[0, :, :d] *= 8.0
    return theta


@pytest.mark.parametrize("theta_grad", [False, True], ids=["gin_only", "gin_gtheta"])
@pytest.mark.parametrize("minify", [False, True], ids=["plain", "x8"])
@pytest.mark.parametrize("dims,C", [((40, 64), 1), ((70, 48), 4), ((20, 24, 16), 1), ((24, 40, 32), 4)], ids=lambda v: sid(v) if isinstance(v, tuple) else "C%d" % v)
def test_a_affine_warp(dims, C, minify, theta_grad):
    ops = _ops()
    d = len(dims)
    theta = _theta(d, minify)
    inp, gout, ride = rand((2, C) + dims, 22), rand((2, C) + dims, 23), (rand((2, 1) + dims, 24) > 0).float()
    for pad in ("zeros", "border"):
        ref_out, ref_gin, ref_gth = L.affine_warp_ref(inp, theta, gout, pad=pad)
        ref_ride, _, _ = L.affine_warp_ref(ride, theta, pad=pad)
        control = None
        for name, m in moves(dict(inp=inp.to(DEV), theta=theta.to(DEV), gout=gout.to(DEV), ride=ride.to(DEV))):
            a, t = m["inp"].detach().requires_grad_(True), m["theta"].detach().requires_grad_(theta_grad)
            out, rout = ops.affine_warp(a, t, "bilinear", pad, ride=m["ride"])
            plain = ops.affine_warp(m["inp"].detach(), m["theta"].detach(), "bilinear", pad)
            out.backward(m["gout"])
            tag = (name, pad)
            # values under the 8 x minification: test_affine_warp has no bound (it checks the gradients there).  A normalised
            # position is a sum of three products of magnitude up to 8 x |theta|: its rounding, and with it the error of a
            # sample, is 8 times that of the plain warp -- 8 x TOL
            vtol = TOL * (8.0 if minify else 1.0)
            assert maxdiff(out.detach().cpu(), ref_out) < vtol and maxdiff(rout.cpu(), ref_ride) < vtol, tag
            assert maxdiff(plain.cpu(), ref_out) < vtol, tag
            # (against float64 rather than ATen's float32: relative to the largest gradient, as test_affine_warp has it where
            # border padding piles samples on a voxel)
            assert maxdiff(a.grad.cpu(), ref_gin) < TOL * max(1.0, float(ref_gin.abs().max())), tag
            got = [out.detach(), rout, plain, a.grad]
            if theta_grad:
                rel = maxdiff(t.grad.cpu(), ref_gth) / max(1e-6, float(ref_gth.abs().max()))
                assert rel < G_THETA[1 if minify else 0], tag + (rel,)
                got.append(t.grad)
            control = control or got
            note("affine_warp", "%s/C%d/%s/%s/%s/%s" % (sid(dims), C, "x8" if minify else "plain", "gth" if theta_grad else "gin", pad, name),
                 got, control)


# ================================================================================================ A: Gaussian
GAUSS_JOBS = [(0, 0), (1, 0), (2, 1), (0, 2)]      # test_gauss_xy_launch_equals_the_per_axis_passes


@pytest.mark.parametrize("pre,post", GAUSS_JOBS)
@pytest.mark.parametrize("dims", [(64, 256), (33, 80), (12, 20), (35, 20, 80), (40, 12, 16)], ids=sid)
def test_a_raw_gauss(dims, pre, post):
    ops = _ops()
    d = len(dims)
    x = (rand((2, d) + dims, 64) * 0.5 + (ident(2, dims) if pre == 2 else 0)).contiguous()
    aux = (ident(2, dims) * 1.05 + 0.1 * rand((2, d) + dims, 65)).contiguous() if post == 2 else None
    ref = L.gauss_ref(x, list(ops._GAUSS9), pre, post, 1.5, aux)
    bound = (GAUSS[0] if pre == 0 and post == 0 else GAUSS[1]) * max(1.0, float(ref.abs().max()))
    control = None
    for name, m in moves(dict(x=x.to(DEV), aux=None if aux is None else aux.to(DEV))):
        outs = []
        for lanes in (True, False):
            old, ops.GAUSS_XY_LANES = ops.GAUSS_XY_LANES, lanes
            try:
                outs.append(ops.raw_gauss(m["x"], d, pre=pre, post=post, scale=1.5, aux=m["aux"]))
            finally:
                ops.GAUSS_XY_LANES = old
        assert torch.equal(outs[0], outs[1]), name          # lane form == staged form, bit for bit (test_gauss_lanes_gpu)
        assert maxdiff(outs[0].cpu(), ref) < bound, name
        control = control or outs
        note("raw_gauss", "%s/pre%d_post%d/%s" % (sid(dims), pre, post, name), outs[:1], control[:1])
        # another formulation at most (x+y launch refused -> per-axis passes): the bound between the two forms
        assert maxdiff(outs[0], control[0]) <= GAUSS_FORMS * max(1.0, float(ref.abs().max())), name


@pytest.mark.parametrize("dims", [(64, 256), (72, 96), (35, 20, 80)], ids=sid)      # (planes above 4096 voxels: the x+y route)
def test_a_gauss_out_operand(dims):
    """ops.raw_gauss allocates its result, so `out` moves here through the C ABI: advchain_gauss_xy refuses an `out` off a
    16-byte boundary (-2, nothing written) and advchain_gauss_axis, the route raw_gauss then takes, writes it with its 1-voxel
    form -- same values as the aligned passes to the bound between the forms, float64 within the entry's bound."""
    from advchain_amd import _lib
    ops = _ops()
    lib = _lib.load()
    d = len(dims)
    x = (rand((2, d) + dims, 64) * 0.5).contiguous()
    ref = L.gauss_ref(x, list(ops._GAUSS9), 1, 0, 1.5)
    xd = x.to(DEV)
    control = ops.raw_gauss(xd, d, pre=1, scale=1.5)
    for k in (1, 2, 3):
        out = L.offset_copy(torch.full((2, d) + dims, 7.0, device=DEV), k)
        rc = lib.advchain_gauss_xy(ops._ptr(xd), ops._ptr(out), None, 2 * d, d, d, _lib.dims_array(dims), ops._GAUSS9, 1, 0, 1.5,
                                   ops._stream(), None, 2 * d)
        torch.cuda.synchronize()
        assert rc == -2 and bool((out == 7.0).all()), (k, rc)
        cur = xd
        for i, ax in enumerate([2, 1, 0][:d]):
            nxt = L.offset_copy(torch.full((2, d) + dims, float("nan"), device=DEV), 1 + (k + i) % 3)
            _lib.check(lib.advchain_gauss_axis(ops._ptr(cur), ops._ptr(nxt), None, 2 * d, d, d, _lib.dims_array(dims), ax, ops._GAUSS9,
                                               1 if i == 0 else 0, 0, 1.5 if i == 0 else 1.0, ops._stream()), "gauss_axis")
            cur = nxt
        assert maxdiff(cur.cpu(), ref) < GAUSS[1] * max(1.0, float(ref.abs().max())), k
        assert maxdiff(cur, control) <= GAUSS_FORMS * max(1.0, float(ref.abs().max())), k
        note("raw_gauss_out", "%s/out+%d" % (sid(dims), k), (cur,), (control,))


def test_a_gauss_small_pair():
    ops = _ops()
    w = list(ops._GAUSS9)
    x = rand((2, 2, 16, 16), 66)
    ref = torch.cat([L.gauss_ref(x, w, 1, 0, 1.5), L.gauss_ref(x, w, 1, 0, -1.5)], 0)
    x2 = rand((4, 2, 16, 16), 67)
    ref_adj = L.gauss_ref(x2[:2], w, 1, 0, 1.5) - L.gauss_ref(x2[2:], w, 1, 0, 1.5)
    control = None
    for name, m in moves(dict(x=x.to(DEV), x2=x2.to(DEV), out=torch.empty((4, 2, 16, 16), device=DEV))):
        fwd = ops.raw_gauss_small_pair(m["x"], 1.5)
        adj = ops.raw_gauss_small_pair(m["x2"], 1.5, adjoint=True)
        ops.raw_gauss_small_pair_into(m["x"], m["out"], 1.5)
        assert maxdiff(fwd.cpu(), ref) < GAUSS[1] and maxdiff(adj.cpu(), ref_adj) < 2 * GAUSS[1], name
        got = (fwd, adj, m["out"].clone())
        control = control or got
        assert torch.equal(got[0], got[2]), name
        assert note("gauss_small_pair", name, got, control), name      # one kernel, scalar accesses: the same bits


# ================================================================================================ A: tensor-product upsampling
TP_SHAPES = [((12, 12), (192, 192)), ((3, 5), (24, 40)), ((4, 4, 8), (32, 32, 64)), ((4, 5, 10), (32, 40, 80)), ((4, 4, 16), (32, 32, 128))]


@pytest.mark.parametrize("low,full", TP_SHAPES, ids=lambda v: sid(v))
def test_a_tp_interp_and_adjoint(low, full):
    from advchain_amd import bands
    ops = _ops()
    d = len(low)
    coef, gfull, gfull2 = rand((2, d) + low, 51), rand((2, d) + full, 52), rand((2, d) + full, 53)
    ref, ref_adj = L.interp_ref(coef, full, (gfull.double() - gfull2.double()) * 0.25)
    tabs = bands.upsample_tables(low, full, DEV)
    ref_adj1 = L.interp_ref(coef, full, gfull)[1]
    control = None
    for name, m in moves(dict(coef=coef.to(DEV), out=torch.empty((2, d) + full, device=DEV), gfull=gfull.to(DEV), gfull2=gfull2.to(DEV))):
        m["out"].fill_(float("nan"))
        out = ops.raw_tp_interp(m["coef"], tabs, d, out=m["out"])
        out2 = ops.raw_tp_interp(m["coef"], tabs, d, add_identity=True, scale=0.125)
        adj = ops.raw_tp_adjoint(m["gfull"], tabs, gfull2=m["gfull2"], scale=0.25)
        adj1 = ops.raw_tp_adjoint(m["gfull"], tabs)
        assert maxdiff(out.cpu(), ref) < TP[0], name
        assert maxdiff(out2.cpu(), L.identity_grid64(2, full) + 0.125 * ref) < TP[0], name
        assert maxdiff(adj.cpu(), ref_adj) / float(ref_adj.abs().max()) < TP[1], name
        assert maxdiff(adj1.cpu(), ref_adj1) / float(ref_adj1.abs().max()) < TP[1], name
        got = (out.clone(), out2, adj, adj1)
        control = control or got
        note("tp_interp", "%s/%s" % (sid(full), name), got, control)


@pytest.mark.parametrize("low,full", TP_SHAPES[:2], ids=lambda v: sid(v))
def test_a_tp_interp_smoothed_pair(low, full):
    """advchain_tp_interp_fwd_smoothed_pair against advchain_gauss_small_pair + advchain_tp_interp_fwd: "same arithmetic as the two
    calls, bit for bit", with each operand of either moved"""
    from advchain_amd import _lib, bands
    ops = _ops()
    lib = _lib.load()
    vel = rand((2, 2) + low, 54)
    tabs = bands.upsample_tables(low, full, DEV)
    control = None
    for name, m in moves(dict(vel=vel.to(DEV), s1=torch.empty((4, 2) + low, device=DEV), out=torch.empty((4, 2) + full, device=DEV))):
        m["s1"].fill_(float("nan"))
        m["out"].fill_(float("nan"))
        rc = lib.advchain_tp_interp_fwd_smoothed_pair(ops._ptr(m["vel"]), ops._ptr(m["s1"]), ops._ptr(m["out"]), ops._ptr(tabs.itab),
                                                      ops._ptr(tabs.ftab), _lib.dims_array(tabs.S), _lib.dims_array(tabs.g),
                                                      _lib.dims_array(tabs.B), 4, 2, 1, 0.0625, None, ops._GAUSS9, 1.5, ops._stream())
        s1 = ops.raw_gauss_small_pair(m["vel"], 1.5)
        two = ops.raw_tp_interp(s1, tabs, 2, add_identity=True, scale=0.0625)
        FIGURES.setdefault("tp_interp_smoothed_pair", {})["%s/%s" % (sid(full), name)] = "rc %d" % rc
        assert rc in (0, -2), rc
        if rc == 0:
            assert torch.equal(m["s1"], s1) and torch.equal(m["out"], two), name
        control = control or (s1, two)
        assert torch.equal(s1, control[0]), name
        assert maxdiff(two, control[1]) <= TP[0], name
        ref = L.interp_ref(s1.cpu(), full)[0] * 0.0625 + L.identity_grid64(4, full)
        assert maxdiff(two.cpu(), ref) < TP[0], name


# ================================================================================================ A: bias field
def _bias_shapes():
    from tests.test_bias_rows_gpu import SHAPES      # (plain data: importing the module needs no GPU)
    return [s for s in SHAPES if s[0][-1] % 4 == 0]


BIAS_SHAPES = _bias_shapes()
BIAS_IDS = [sid(s) for s, _ in BIAS_SHAPES]


@pytest.mark.parametrize("shape,spacing", BIAS_SHAPES, ids=BIAS_IDS)
def test_a_bias_apply(shape, spacing):
    """bounds: tests/test_bias_rows_gpu._check_against_float64"""
    from tests import cpu_backend
    from tests.test_bias_rows_gpu import _case, _geometry
    ops = _ops()
    assert len(BIAS_SHAPES) == 5
    tables, _ = _geometry(shape, spacing)
    cp, data, gout, eps = _case(shape, spacing, True, 1.0)
    cpd, dd = cp.cpu().double().requires_grad_(True), data.cpu().double().requires_grad_(True)
    r_out, r_field = cpu_backend.bias_apply(cpd, dd, tables, eps, True, 1.0)
    r_out.backward(gout.cpu().double())
    control = None
    for name, m in moves(dict(cp=cp, data=data, gout=gout)):
        got = []
        for reduced in (True, False):
            old, ops.BIAS_REDUCED = ops.BIAS_REDUCED, reduced
            try:
                c, x = m["cp"].detach().requires_grad_(True), m["data"].detach().requires_grad_(True)
                out, field = ops.bias_apply(c, x, tables, eps, True, 1.0)
                out.backward(m["gout"])
            finally:
                ops.BIAS_REDUCED = old
            assert maxdiff(out.detach().cpu(), r_out.detach()) <= 5e-6 and maxdiff(field.cpu(), r_field) <= 5e-6, name
            assert maxdiff(c.grad.cpu(), cpd.grad) <= 2e-5 * max(1.0, float(cpd.grad.abs().max())), name
            assert maxdiff(x.grad.cpu(), dd.grad) <= 1e-5, name
            got.append((out.detach(), field, c.grad, x.grad))
        # the reduced backward and the two launches: bit-identical, wherever the operands sit
        assert all(torch.equal(a, b) for a, b in zip(got[0], got[1])), name
        control = control or got[0]
        note("bias_apply", "%s/%s" % (sid(shape), name), got[0], control)


# ================================================================================================ A: the axpy family
@pytest.mark.parametrize("gate", [None, 1.0, float("nan")], ids=["nogate", "finite", "nan"])
@pytest.mark.parametrize("M", [16, 512, 65536, 385])
def test_a_axpy_family(M, gate):
    ops = _ops()
    N = 3
    base, x, old = rand((N, M), 71), rand((N, M), 72), rand((N, M), 73)
    gt = None if gate is None else torch.tensor(gate, device=DEV)
    keep = gate is not None and gate != gate
    r_axpy = base.double() + 0.3 * x.double()
    r_norm = old.double() if keep else base.double() + 0.7 * L.unit_normalize_ref(x)
    r_sign = old.double() if keep else base.double() + 0.7 * torch.sign(x.double())
    control = None
    for name, m in moves(dict(base=base.to(DEV), x=x.to(DEV), old=old.to(DEV))):
        o = m["old"] if gate is not None else None
        got = [ops.raw_axpy(m["base"], m["x"], 0.3), ops.raw_axpy(None, m["x"], -2.0),
               ops.normalized_axpy(m["base"], m["x"], 0.7, gate=gt, old=o), ops.sign_axpy(m["base"], m["x"], 0.7, gate=gt, old=o)]
        multi = ops.update_multi([(m["base"], m["x"], 0.7, 0, o), (m["base"], m["x"], 0.7, 1, o)], gate=gt)
        assert maxdiff(got[0].cpu(), r_axpy) < AXPY and maxdiff(got[1].cpu(), -2.0 * x.double()) < AXPY, name
        assert maxdiff(got[2].cpu(), r_norm) < AXPY and maxdiff(got[3].cpu(), r_sign) < AXPY, name
        assert maxdiff(multi[0].cpu(), r_norm) < AXPY and maxdiff(multi[1].cpu(), r_sign) < AXPY, name
        if keep:
            assert torch.equal(got[2], m["old"]) and torch.equal(multi[0], m["old"]) and torch.equal(multi[1], m["old"]), name
        got += list(multi)
        control = control or got
        note("axpy_family", "M%d/%s/%s" % (M, "nogate" if gate is None else str(gate), name), got, control)
        # one multiply-add per element, sign(x) exactly: no order to depend on
        assert torch.equal(got[0], control[0]) and torch.equal(got[1], control[1]) and torch.equal(got[3], control[3]), name


def test_a_update_multi_rows_inside_one_flat_buffer():
    """descriptors whose rows are views of one flat parameter bucket at 4-byte granularity"""
    ops = _ops()
    sizes = [(2, 385), (2, 16), (2, 511), (2, 512)]
    total = sum(a * b for a, b in sizes)
    flat_x, flat_b = rand((total + 8,), 74), rand((total + 8,), 75)
    fx, fb = flat_x.to(DEV), flat_b.to(DEV)
    items, refs, off = [], [], 1
    for i, (n, mm) in enumerate(sizes):
        xs, bs = fx[off:off + n * mm].view(n, mm), fb[off:off + n * mm].view(n, mm)
        items.append((bs, xs, 0.5, i % 2, None))
        xd, bd = flat_x[off:off + n * mm].view(n, mm).double(), flat_b[off:off + n * mm].view(n, mm).double()
        refs.append(bd + 0.5 * (torch.sign(xd) if i % 2 else L.unit_normalize_ref(xd)))
        off += n * mm
    assert len({it[1].data_ptr() % 16 for it in items}) > 1
    outs = ops.update_multi(items)
    for o, r, it in zip(outs, refs, items):
        assert maxdiff(o.cpu(), r) < AXPY
        one = ops.sign_axpy(it[0], it[1], 0.5) if it[3] else ops.normalized_axpy(it[0], it[1], 0.5)
        assert maxdiff(o, one) < AXPY
        note("update_multi_vs_single", "M%d" % it[1].shape[1], (o,), (one,))


# ================================================================================================ A: displacement measurements
@pytest.mark.parametrize("dims", [(64, 256), (9, 18, 64)], ids=sid)
def test_a_displacement_measurements(dims):
    ops = _ops()
    d = len(dims)
    phi = smooth_field(dims, 2.3, 51)
    dv = (phi.double() - L.identity_grid64(2, dims))
    want = max(float((dv[:, a] * (dims[d - 1 - a] - 1) / 2).abs().max()) for a in range(d))
    control = None
    for name, m in moves(dict(phi=phi.to(DEV))):
        got = ops.raw_max_displacement(m["phi"])
        via = torch.tensor([float(ops.grid_displacement(m["phi"])[0].values()[0])], device=DEV)
        assert abs(float(got) - want) < 1e-3, name           # test_displacement_measurements
        control = control or (got, via)
        assert torch.equal(got, control[0]) and torch.equal(via, control[1]) and torch.equal(got, via), name      # a maximum has no order


@pytest.mark.parametrize("cols", [2048, 4096])
def test_a_slot_rows_max(cols):
    ops = _ops()
    acc = torch.rand(5, cols, device=DEV)
    acc[3, 77] = float("nan")
    ref = acc.max(dim=1).values
    for name, m in moves(dict(slots=acc, out=torch.empty(5, device=DEV))):
        got = ops.raw_slot_rows_max(m["slots"], out=m["out"])
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[~torch.isnan(ref)], ref[~torch.isnan(ref)]), name
    for s in (acc.clone(), L.offset_copy(acc, 1), L.offset_copy(acc, 2)):      # reset: the accumulator is zeroed behind the read
        got = ops.raw_slot_rows_max(s, reset=True)
        assert torch.equal(got[~torch.isnan(ref)], ref[~torch.isnan(ref)]) and float(s.abs().max()) == 0.0


# ================================================================================================ A: Jacobian and differences
@pytest.mark.parametrize("positions,clamp", [(False, False), (True, True)], ids=["displacement", "clamped_positions"])
@pytest.mark.parametrize("dims", [(40, 130), (6, 10, 70)], ids=sid)
def test_a_jacobian(dims, positions, clamp):
    """bounds: tests/test_jacobian3d_gpu (4 x the error of the fp32 twin of the closed form, at least 1e-6)"""
    ops = _ops()
    d = len(dims)
    field = smooth_field(dims, 1.5, 31) * 1.05 if positions else 0.3 * rand((2, d) + dims, 32)
    gout = rand((2, 1) + dims, 33)
    f64 = field.double().requires_grad_(True)
    det64 = JF.jacobian_det64(f64, positions, clamp)
    det64.backward(gout.double())
    f32 = field.clone().requires_grad_(True)
    det32 = JF.jacobian_det32(f32, positions, clamp)
    det32.backward(gout)
    e32v, e32g = maxdiff(det32.detach(), det64.detach()), maxdiff(f32.grad, f64.grad)
    control = None
    for name, m in moves(dict(field=field.to(DEV), gout=gout.to(DEV))):
        f = m["field"].detach().requires_grad_(True)
        det = ops.jacobian_det(f, positions, clamp)
        det.backward(m["gout"])
        st = ops.jacobian_stats(m["field"].detach(), positions, clamp)
        assert maxdiff(det.detach().cpu(), det64.detach()) <= max(1e-6, 4 * e32v), name
        assert maxdiff(f.grad.cpu(), f64.grad) <= max(1e-6, 4 * e32g), name
        flat = det.detach().flatten(1)
        assert torch.equal(st.neg, (flat < 0).sum(1)) and torch.equal(st.nonpos, (~(flat > 0)).sum(1)), name
        img = m["field"].detach()
        diffs = ops.image_diff2d(img) if d == 2 else ops.image_diff3d(img)
        got = (det.detach(), f.grad, st.neg, st.nonpos, st.min, st.max) + tuple(diffs)
        control = control or got
        # per-voxel stencils and gather-form backwards (documented reproducible): no sum crosses a lane
        assert note("jacobian", "%s/%s/%s" % (sid(dims), "pos" if positions else "disp", name), got, control), name


# ================================================================================================ B: non-contiguous operands
def _variants(t):
    return [("contiguous", t)] + L.strided_variants(t)


def _grad_forms(out):
    """[(name, fn(out) -> starts the backward)]: the incoming gradient as a transposed-back tensor, an expanded scalar, and the
    zero-interleaved gradient of a step-2 slice"""
    w = rand(tuple(out.shape), 91).to(out.device)
    wt = w.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not wt.is_contiguous()
    return [("contiguous", lambda o: o.backward(w), w.cpu()),
            ("transposed", lambda o: o.backward(wt), w.cpu()),
            ("expanded", lambda o: o.sum().backward(), torch.ones_like(w).cpu()),
            ("expanded_tensor", lambda o: o.backward(L.expanded_grad(o.shape, o.device)), torch.ones_like(w).cpu()),
            ("step2", lambda o: o[..., ::2].sum().backward(), _step2_ones(w).cpu())]


def _step2_ones(w):
    g = torch.zeros_like(w)
    g[..., ::2] = 1
    return g


@pytest.mark.parametrize("dims,mode", [((24, 40), "bilinear"), ((24, 40), "bicubic"), ((6, 10, 72), "bilinear")],
                         ids=["24x40-bilinear", "24x40-bicubic", "6x10x72-bilinear"])
def test_b_grid_sample_non_contiguous(dims, mode):
    ops = _ops()
    d = len(dims)
    C = 4      # (C = 1, 4: the channel counts whose backward formulations are reproducible run to run)
    inp = rand((2, C) + dims, 42)
    grid = (ident(2, dims) * 1.02 + 0.02 * rand((2, d) + dims, 41)).contiguous()
    gb = G_BICUBIC if mode == "bicubic" else G_SAMPLER

    def run(a, g, start):
        a, g = a.detach().requires_grad_(True), g.detach().requires_grad_(True)
        out = ops.grid_sample(a, g, mode, "zeros")
        start(out)
        return out.detach(), a.grad, g.grad

    # Which backward route a contiguous and a strided grid take.  ops.last_bwd_route() is a note per THREAD and autograd runs the
    # backward on its own, so the launcher is called here directly with what ops.grid_sample passes it: the bound measured on
    # a contiguous grid, none (halo 0) for a strided one, whose displacement is not measured.  (Bicubic has one kernel.)
    if mode == "bilinear":
        measured = float(ops.raw_max_displacement(grid.to(DEV)).item())
        for what, halo in (("contiguous", ops._warp_halo_of(measured, d)), ("strided", 0)):
            ops.raw_grid_sample_bwd(rand((2, C) + dims, 43).to(DEV), inp.to(DEV), grid.to(DEV), 0, 0, False, True, True, halo)
            note_route("b_grid_sample_bilinear", "%s/grid_%s/halo%d" % (sid(dims), what, halo), ops.last_bwd_route())

    probe = ops.grid_sample(inp.to(DEV), grid.to(DEV), mode, "zeros")
    for gname, start, w in _grad_forms(probe):
        ref = L.grid_sample_ref(inp, grid, w, mode=mode)
        control = run(inp.to(DEV), grid.to(DEV), lambda o, w=w: o.backward(w.to(DEV)))
        for iname, a in _variants(inp.to(DEV)):
            for qname, g in _variants(grid.to(DEV)):
                if gname != "contiguous" and (iname != "contiguous" or qname != "contiguous"):
                    continue      # (one thing at a time)
                got = run(a, g, start)
                tag = (gname, iname, qname)
                assert maxdiff(got[0].cpu(), ref[0]) < TOL, tag
                assert maxdiff(got[1].cpu(), ref[1]) < gbound(ref[1]), tag
                assert maxdiff(got[2].cpu(), ref[2]) < gbound(ref[2], gb), tag
                assert torch.equal(got[0], control[0]), tag
                if qname == "contiguous" and mode == "bilinear":      # the copy takes the kernels of the control: same bits
                    assert torch.equal(got[1], control[1]) and torch.equal(got[2], control[2]), tag
                else:      # no displacement measurement for a strided grid: another backward route (recorded above)
                    note("b_grid_sample_%s" % mode, "%s/grad_%s/inp_%s/grid_%s" % (sid(dims), gname, iname, qname), got[1:3], control[1:3])


@pytest.mark.parametrize("dims,C", [((40, 64), 1), ((20, 24, 16), 2)], ids=lambda v: sid(v) if isinstance(v, tuple) else "C%d" % v)
def test_b_affine_warp_non_contiguous(dims, C):
    ops = _ops()
    d = len(dims)
    theta, inp = _theta(d, False), rand((2, C) + dims, 22)

    def run(a, t, start):
        a, t = a.detach().requires_grad_(True), t.detach().requires_grad_(True)
        out = ops.affine_warp(a, t)
        start(out)
        return out.detach(), a.grad, t.grad

    probe = ops.affine_warp(inp.to(DEV), theta.to(DEV))
    th = theta.to(DEV)
    th_t = th.transpose(1, 2).contiguous().transpose(1, 2)
    assert not th_t.is_contiguous()
    for gname, start, w in _grad_forms(probe):
        ref = L.affine_warp_ref(inp, theta, w)
        control = run(inp.to(DEV), th, lambda o, w=w: o.backward(w.to(DEV)))
        for iname, a in _variants(inp.to(DEV)):
            for tname, t in (("contiguous", th), ("transposed", th_t)):
                if gname != "contiguous" and (iname != "contiguous" or tname != "contiguous"):
                    continue
                got = run(a, t, start)
                tag = (gname, iname, tname)
                assert maxdiff(got[0].cpu(), ref[0]) < TOL and maxdiff(got[1].cpu(), ref[1]) < TOL * max(1.0, float(ref[1].abs().max())), tag
                assert maxdiff(got[2].cpu(), ref[2]) / float(ref[2].abs().max()) < G_THETA[0], tag
                assert all(torch.equal(x, y) for x, y in zip(got, control)), tag      # _dev copies: the control's kernels


@pytest.mark.parametrize("dims", [(33, 80), (12, 20), (35, 20, 80)], ids=sid)
def test_b_gauss_smooth_non_contiguous(dims):
    ops = _ops()
    d = len(dims)
    x = rand((2, d) + dims, 64)
    w9 = list(ops._GAUSS9)
    probe = ops.gauss_smooth(x.to(DEV))
    for gname, start, w in _grad_forms(probe):
        ref, ref_g = L.gauss_ref(x, w9), L.gauss_ref(w, w9)
        control = None
        for xname, v in _variants(x.to(DEV)):
            if gname != "contiguous" and xname != "contiguous":
                continue
            a = v.detach().requires_grad_(True)
            out = ops.gauss_smooth(a)
            if control is None:
                out.backward(w.to(DEV))      # the control: contiguous input, the same gradient as a contiguous tensor
            else:
                start(out)
            got = (out.detach(), a.grad)
            assert maxdiff(got[0].cpu(), ref) < GAUSS[0] and maxdiff(got[1].cpu(), ref_g) < GAUSS[0] * max(1.0, float(ref_g.abs().max())), (gname, xname)
            assert all(torch.equal(p, q) for p, q in zip(got, control or got)), (gname, xname)
            control = control or got
        a = x.to(DEV).requires_grad_(True)
        start(ops.gauss_smooth(a))
        assert torch.equal(a.grad, control[1]), gname


@pytest.mark.parametrize("low,full", [((3, 5), (24, 40)), ((4, 5, 10), (32, 40, 80))], ids=lambda v: sid(v))
def test_b_upsample_field_non_contiguous(low, full):
    from advchain_amd import bands
    ops = _ops()
    d = len(low)
    coef = rand((2, d) + low, 51)
    tabs = bands.upsample_tables(low, full, DEV)
    probe = ops.upsample_field(coef.to(DEV), tabs, 0.125)
    for gname, start, w in _grad_forms(probe):
        up, adj = L.interp_ref(coef, full, w.double() * 0.125)
        ref = L.identity_grid64(2, full) + 0.125 * up
        control = None
        for cname, v in _variants(coef.to(DEV)):
            if gname != "contiguous" and cname != "contiguous":
                continue
            a = v.detach().requires_grad_(True)
            out = ops.upsample_field(a, tabs, 0.125)
            start(out)
            got = (out.detach(), a.grad)
            assert maxdiff(got[0].cpu(), ref) < TP[0], (gname, cname)
            assert maxdiff(got[1].cpu(), adj) / float(adj.abs().max()) < TP[1], (gname, cname)
            control = control or got
            assert all(torch.equal(p, q) for p, q in zip(got, control)), (gname, cname)


def test_b_axpy_non_contiguous():
    ops = _ops()
    x, y = rand((2, 3, 9, 16), 73), rand((2, 3, 9, 16), 74)
    probe = ops.axpy(x.to(DEV), y.to(DEV), 0.5)
    for gname, start, w in _grad_forms(probe):
        for xname, xv in _variants(x.to(DEV)):
            for yname, yv in _variants(y.to(DEV)):
                if gname != "contiguous" and (xname != "contiguous" or yname != "contiguous"):
                    continue
                a, b = xv.detach().requires_grad_(True), yv.detach().requires_grad_(True)
                out = ops.axpy(a, b, 0.5)
                start(out)
                tag = (gname, xname, yname)
                assert maxdiff(out.detach().cpu(), x.double() + 0.5 * y.double()) < AXPY, tag
                assert maxdiff(a.grad.cpu(), w) < AXPY and maxdiff(b.grad.cpu(), 0.5 * w.double()) < AXPY, tag


@pytest.mark.parametrize("dims", [(40, 130), (6, 10, 70)], ids=sid)
def test_b_jacobian_det_non_contiguous(dims):
    ops = _ops()
    d = len(dims)
    field = 0.3 * rand((2, d) + dims, 32)
    probe = ops.jacobian_det(field.to(DEV))
    for gname, start, w in _grad_forms(probe):
        f64 = field.double().requires_grad_(True)
        det64 = JF.jacobian_det64(f64)
        det64.backward(w.double())
        f32 = field.clone().requires_grad_(True)
        det32 = JF.jacobian_det32(f32)
        det32.backward(w)
        e32v, e32g = maxdiff(det32.detach(), det64.detach()), maxdiff(f32.grad, f64.grad)
        control = None
        for fname, v in _variants(field.to(DEV)):
            if gname != "contiguous" and fname != "contiguous":
                continue
            f = v.detach().requires_grad_(True)
            det = ops.jacobian_det(f)
            start(det)
            got = (det.detach(), f.grad)
            assert maxdiff(got[0].cpu(), det64.detach()) <= max(1e-6, 4 * e32v), (gname, fname)
            assert maxdiff(got[1].cpu(), f64.grad) <= max(1e-6, 4 * e32g), (gname, fname)
            control = control or got
            assert torch.equal(got[0], control[0]), (gname, fname)
        f = field.to(DEV).requires_grad_(True)
        ops.jacobian_det(f).backward(w.to(DEV))
        assert torch.equal(f.grad, control[1]), gname      # _dev copies the strided gradient: the kernels of the contiguous one


@pytest.mark.parametrize("shape,spacing", [BIAS_SHAPES[0], BIAS_SHAPES[3]], ids=[BIAS_IDS[0], BIAS_IDS[3]])
def test_b_bias_apply_non_contiguous(shape, spacing):
    from tests import cpu_backend
    from tests.test_bias_rows_gpu import _case, _geometry
    ops = _ops()
    tables, _ = _geometry(shape, spacing)
    cp, data, gout, eps = _case(shape, spacing, True, 1.0)
    probe = ops.bias_apply(cp, data, tables, eps, True, 1.0)[0]
    for gname, start, w in _grad_forms(probe):
        cpd, dd = cp.cpu().double().requires_grad_(True), data.cpu().double().requires_grad_(True)
        r_out, r_field = cpu_backend.bias_apply(cpd, dd, tables, eps, True, 1.0)
        r_out.backward(w.double())
        control = None
        for cname, cv in _variants(cp):
            for dname, dv in _variants(data):
                if gname != "contiguous" and (cname != "contiguous" or dname != "contiguous"):
                    continue
                c, x = cv.detach().requires_grad_(True), dv.detach().requires_grad_(True)
                out, field = ops.bias_apply(c, x, tables, eps, True, 1.0)
                start(out)
                tag = (gname, cname, dname)
                assert maxdiff(out.detach().cpu(), r_out.detach()) <= 5e-6 and maxdiff(field.cpu(), r_field) <= 5e-6, tag
                assert maxdiff(c.grad.cpu(), cpd.grad) <= 2e-5 * max(1.0, float(cpd.grad.abs().max())), tag
                assert maxdiff(x.grad.cpu(), dd.grad) <= 1e-5, tag
                got = (out.detach(), field, c.grad, x.grad)
                control = control or got
                assert all(torch.equal(p, q) for p, q in zip(got, control)), tag


@pytest.mark.parametrize("dims,vs", [((32, 48), [4, 6]), ((16, 20, 24), [4, 5, 6])], ids=lambda v: sid(v))
def test_b_demons_field_non_contiguous(dims, vs):
    """ops.demons_field / demons_field_pair: a strided velocity and strided incoming gradients against the contiguous run (bits)
    and against autograd through the oracle's DemonsCompose (fp32: it builds float32 windows and grids internally; bound 1e-4
    relative, test_demons_field_backward_across_the_gather_threshold)"""
    from advchain_amd import bands
    from oracle import advchain_oracle as O
    ops = _ops()
    d = len(dims)
    vel = O.unit_normalize(rand((2, d) + tuple(vs), 71))
    tables = bands.upsample_tables(list(vs), list(dims), torch.device(DEV))
    probe = ops.demons_field(vel.to(DEV), 1.5, tables, d == 3)
    for gname, start, w in _grad_forms(probe):
        pc = vel.clone().requires_grad_(True)
        want = O.demons_compose(1.5 * pc, dims, final_clamp=False)
        want.backward(w)
        control = None
        for vname, v in _variants(vel.to(DEV)):
            if gname != "contiguous" and vname != "contiguous":
                continue
            a = v.detach().requires_grad_(True)
            q = ops.demons_field(a, 1.5, tables, d == 3)
            start(q)
            b = v.detach().requires_grad_(True)
            qp, qm = ops.demons_field_pair(b, 1.5, tables, d == 3)
            start(qp)
            tag = (gname, vname)
            assert maxdiff(q.detach().cpu(), want.detach()) < TOL, tag
            assert maxdiff(a.grad.cpu(), pc.grad) / float(pc.grad.abs().max()) < 1e-4, tag
            assert torch.equal(qp.detach(), q.detach()), tag      # test_demons_field_pair_is_the_two_single_fields
            assert maxdiff(b.grad, a.grad) <= 2e-6 * float(a.grad.abs().max()), tag
            control = control or (q.detach(), a.grad)
            assert torch.equal(q.detach(), control[0]), tag
            note("b_demons_field", "%s/grad_%s/vel_%s" % (sid(dims), gname, vname), (a.grad,), control[1:])


# ================================================================================================ C: batch independence
def _batch(shape, seed, spike=None):
    """five distinct entries; entry `spike` 1e4 times larger than the rest"""
    t = rand((5,) + tuple(shape), seed)
    if spike is not None:
        t[spike] *= 1e4
    return t


def _entries(run, tensors, picks=(0, 3)):
    """run(*tensors) on the batch of 5 and on each picked entry alone (N = 1): [(n, batch result[n], single result)]"""
    full = run(*[t.to(DEV) for t in tensors])
    out = []
    for n in picks:
        one = run(*[t[n:n + 1].contiguous().to(DEV) for t in tensors])
        out.append((n, [None if r is None else r[n:n + 1] for r in full], one))
    return out


def _assert_entries(entry, case, rows, exact=True, refs=None):
    for n, batch, one in rows:
        for i, (a, b) in enumerate(zip(batch, one)):
            if a is None:
                continue
            same = note("c_" + entry, "%s/entry%d/result%d" % (case, n, i), (a,), (b,))
            if exact:
                assert same, (entry, case, n, i, maxdiff(a, b))


C_DIMS = [(40, 72), (6, 10, 72)]


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("field", [("vox", 0.5, 1), ("vox", 3.3, 4), ("vox", 9.0, 12)], ids=lambda f: "%s%g" % (f[0], f[1]))
@pytest.mark.parametrize("dims", C_DIMS, ids=sid)
def test_c_grid_sample_entries_do_not_depend_on_the_batch(dims, field, deterministic):
    """every backward formulation the product's rule picks (exact gather / march / whole-row / owner-computes scatter, window
    scatter) and the tile kernels with a hint; one entry's gradient is 1e4 times the others' (a batch-wide fixed-point scale
    would cost the small entries their low bits).  The float-atomic window scatter (3D 9 voxels, default mode) sums in arrival
    order: held to the float64 bound only."""
    ops = _ops()
    d = len(dims)
    C = 4
    grid = smooth_field(dims, field[1], 61, 5)
    inp, gout = _batch((C,) + dims, 42), _batch((C,) + dims, 43, spike=1)
    measured = float(ops.raw_max_displacement(grid.to(DEV)).item())
    policy = ops._warp_halo_of(measured, d)
    ref = L.grid_sample_ref(inp, grid, gout)
    was = ops.is_deterministic()
    ops.set_deterministic(deterministic)
    try:
        for halo in dict.fromkeys([policy, abs(policy), 0]):
            routes = []

            def run(a, g, w):
                out = ops.raw_grid_sample_fwd(a, g, 0, 0, False)
                gin, gg = ops.raw_grid_sample_bwd(w, a, g, 0, 0, False, True, True, halo)
                routes.append(ops.last_bwd_route())
                return out, gin, gg
            rows = _entries(run, (inp, grid, gout))
            # by design not reproducible, and so not comparable bit for bit: the float-atomic flush of the window scatter, and
            # the overflow list of the tile kernels (samples displaced beyond the tile halo -- the hint, 2 voxels / 16 pixels
            # without one, at most 4 voxels / 24 pixels -- are drained with global float atomics).  Everything else is exact
            reach = min(halo if halo > 0 else (2 if d == 3 else 16), 4 if d == 3 else 24)
            exact = halo < 0 or (set(routes) <= {"tiled", "gather", "march", "rows", "window_int64", "window_staged"}
                                 and ("tiled" not in routes or measured < reach - 0.001))
            case = "%s/%s%g/halo%d/%s" % (sid(dims), field[0], field[1], halo, "det" if deterministic else "default")
            note_route("c_grid_sample", case, "/".join(dict.fromkeys(routes)))
            _assert_entries("grid_sample", case, rows, exact=exact)
            for n, batch, one in rows:
                for got in (batch, one):
                    assert maxdiff(got[0].cpu(), ref[0][n:n + 1]) < TOL, (case, n)
                    assert maxdiff(got[1].cpu(), ref[1][n:n + 1]) < gbound(ref[1][n:n + 1]), (case, n)
                    assert maxdiff(got[2].cpu(), ref[2][n:n + 1]) < gbound(ref[2][n:n + 1]), (case, n)
    finally:
        ops.set_deterministic(was)


def _compose_route(d, h):
    """the formulation advchain_compose_self_bwd takes for a bound h (compose_self_bwd_impl, sampler.hip; shapes the gather form
    and the window scatter take)"""
    if d == 2:
        return "rows" if h <= -2 else ("gather" if 1 <= abs(h) <= 4 else "window")
    return "march" if h <= -2 else ("gather" if abs(h) == 1 else ("window" if abs(h) >= 2 else "tiled"))


@pytest.mark.parametrize("amp", [0.3, 1.4, 2.6])
@pytest.mark.parametrize("dims", C_DIMS, ids=sid)
def test_c_compose_self_entries_do_not_depend_on_the_batch(dims, amp):
    ops = _ops()
    d = len(dims)
    phi = smooth_field(dims, amp, 11, 5)
    gout = _batch((d,) + dims, 12, spike=1)
    measured = float(ops.raw_max_displacement(phi.to(DEV)).item())
    halo = ops.squaring_halo(measured, d)
    ref_out, ref_g = L.compose_self_ref(phi, gout)
    for h in dict.fromkeys([halo, abs(halo), 0]):
        def run(p, w):
            ws = ops._scatter_workspace(p.shape[0], dims, DEV)
            return ops.raw_compose_self_fwd(p), ops.raw_compose_self_bwd(w, p, ws, chain=False, halo=h)
        rows = _entries(run, (phi, gout))
        # Which formulation compose_self_bwd_impl (sampler.hip) takes for this bound, and whether its sums have an order:
        # exact bounds (negative) -- whole rows, gather form, march -- none.  A hint the gather form takes (1 in 3D, 1..4 in 2D)
        # with every sample inside it: nothing reaches the overflow list, none.  No bound in 3D: the tile kernel (halo 2), 64-bit
        # integer LDS sums, none while every sample stays inside the halo -- this is the SELF instantiation of k_scatter_rows,
        # whose whole-batch scale this test caught (3.1e-5 at amp 0.3).  Everything else -- a hint the samples exceed (overflow
        # list: float atomics), the window scatter (3D hints of 2 and more, 2D without a bound or above 4: float-atomic flush)
        # -- depends on arrival order by design: the float64 bound, difference noted
        route = _compose_route(d, h)
        exact = h < 0 or (route == "gather" and measured < h - 0.001) or (route == "tiled" and measured < 2 - 0.001)
        note_route("c_compose_self", "%s/amp%g/halo%d" % (sid(dims), amp, h), "%s, %s" % (route, "bit-equal asserted" if exact else "float64 bound"))
        _assert_entries("compose_self", "%s/amp%g/halo%d" % (sid(dims), amp, h), rows, exact=exact)
        for n, batch, one in rows:
            for got in (batch, one):
                assert maxdiff(got[0].cpu(), ref_out[n:n + 1]) < TOL, (h, n)
                assert maxdiff(got[1].cpu(), ref_g[n:n + 1]) < gbound(ref_g[n:n + 1]), (h, n)


@pytest.mark.parametrize("dims", [(256, 64), (6, 9, 80)], ids=sid)
def test_c_expo_chain_entries_do_not_depend_on_the_batch(dims):
    """n = 4 fixed; 2D: 16 fields fuse (256 windows), one field alone takes the per-squaring launches (16 windows)"""
    ops = _ops()
    d, n = len(dims), 4
    N = 16 if d == 2 else 5
    phi0 = drift_field(dims, 0.005, 0.04, 21, N)
    gk = rand((N, d) + dims, 22)
    gk[1] *= 1e4
    hints = [1 | (1 << 8)] * n

    def run(p, w):
        m = dict(phi0=p, fields=torch.empty((n - 1,) + tuple(p.shape), device=DEV), pos=torch.empty_like(p), gk=w,
                 g0=torch.empty_like(p), scratch=torch.empty_like(p))
        _chain_fwd(ops, m, n, hints, d == 2)
        _chain_bwd(ops, m, n, [-1] * n)
        return m["fields"], m["pos"], m["g0"]
    fields, pos, g0 = run(phi0.to(DEV), gk.to(DEV))
    for e in (0, 3):
        f1, p1, g1 = run(phi0[e:e + 1].contiguous().to(DEV), gk[e:e + 1].contiguous().to(DEV))
        assert torch.equal(fields[:, e:e + 1], f1) and torch.equal(pos[e:e + 1], p1), e
        assert note("c_expo_chain", "%s/entry%d" % (sid(dims), e), (g0[e:e + 1],), (g1,)), e


@pytest.mark.parametrize("theta_grad", [False, True], ids=["gin_only", "gin_gtheta"])
@pytest.mark.parametrize("dims,C", [((70, 48), 4), ((24, 40, 32), 4)], ids=lambda v: sid(v) if isinstance(v, tuple) else "C%d" % v)
def test_c_affine_warp_entries_do_not_depend_on_the_batch(dims, C, theta_grad):
    ops = _ops()
    d = len(dims)
    theta = (torch.eye(d, d + 1).repeat(5, 1, 1) + 0.2 * rand((5, d, d + 1), 21)).contiguous()
    inp, gout = _batch((C,) + dims, 22), _batch((C,) + dims, 23, spike=1)

    def run(a, t, w):
        a, t = a.requires_grad_(True), t.requires_grad_(theta_grad)
        out = ops.affine_warp(a, t)
        out.backward(w)
        return out.detach(), a.grad, t.grad
    _assert_entries("affine_warp", "%s/%s" % (sid(dims), "gth" if theta_grad else "gin"), _entries(run, (inp, theta, gout)))


@pytest.mark.parametrize("pre,post", GAUSS_JOBS)
@pytest.mark.parametrize("dims", [(33, 80), (35, 20, 80)], ids=sid)
def test_c_raw_gauss_entries_do_not_depend_on_the_batch(dims, pre, post):
    ops = _ops()
    d = len(dims)
    x = (_batch((d,) + dims, 64) * 0.5 + (ident(5, dims) if pre == 2 else 0)).contiguous()
    aux = (ident(5, dims) * 1.05 + 0.1 * _batch((d,) + dims, 65)).contiguous()

    def run(v, a):
        return (ops.raw_gauss(v, d, pre=pre, post=post, scale=1.5, aux=a if post == 2 else None),)
    _assert_entries("raw_gauss", "%s/pre%d_post%d" % (sid(dims), pre, post), _entries(run, (x, aux)))


@pytest.mark.parametrize("low,full", [((3, 5), (24, 40)), ((4, 5, 10), (32, 40, 80))], ids=lambda v: sid(v))
def test_c_tp_interp_entries_do_not_depend_on_the_batch(low, full):
    """tp_interp packs four planes a workgroup: N = 1 (2 or 3 planes) and N = 5 (10 or 15) both leave a partial group"""
    from advchain_amd import bands
    ops = _ops()
    d = len(low)
    tabs = bands.upsample_tables(low, full, DEV)
    coef, gfull = _batch((d,) + low, 51), _batch((d,) + full, 52, spike=1)

    def run(c, g):
        return ops.raw_tp_interp(c, tabs, d, add_identity=True, scale=0.125), ops.raw_tp_adjoint(g, tabs, scale=0.25)
    _assert_entries("tp_interp", sid(full), _entries(run, (coef, gfull)))


@pytest.mark.parametrize("shape,spacing", [BIAS_SHAPES[0], BIAS_SHAPES[3]], ids=[BIAS_IDS[0], BIAS_IDS[3]])
def test_c_bias_apply_entries_do_not_depend_on_the_batch(shape, spacing):
    from advchain_amd.augmentor import AdvBias
    ops = _ops()
    res = {}
    g = torch.Generator().manual_seed(99)
    cp5 = data5 = gout5 = None
    for N in (5, 1):
        cfg = dict(epsilon=0.3, control_point_spacing=list(spacing), downscale=2, data_size=[N] + list(shape[1:]),
                   interpolation_order=3, init_mode="random", space="log")
        t = AdvBias(len(shape) - 2, cfg, device=torch.device(DEV))
        t.init_parameters()
        if cp5 is None:
            cp5 = (torch.randn(tuple(t.param.shape), generator=g) * 0.4).float()
            data5 = torch.rand((5,) + tuple(shape[1:]), generator=g) + 0.5
            gout5 = torch.randn((5,) + tuple(shape[1:]), generator=g)
            gout5[1] *= 1e4
        res[N] = t._tables

    def run_with(tables, cp, data, gout):
        c, x = cp.to(DEV).requires_grad_(True), data.to(DEV).requires_grad_(True)
        out, field = ops.bias_apply(c, x, tables, 0.2, True, 1.0)
        out.backward(gout.to(DEV))
        return out.detach(), field, c.grad, x.grad
    full = run_with(res[5], cp5, data5, gout5)
    for n in (0, 3):
        one = run_with(res[1], cp5[n:n + 1].contiguous(), data5[n:n + 1].contiguous(), gout5[n:n + 1].contiguous())
        for i, (a, b) in enumerate(zip(full, one)):
            assert note("c_bias_apply", "%s/entry%d/result%d" % (sid(shape), n, i), (a[n:n + 1],), (b,)), (n, i)


@pytest.mark.parametrize("M", [512, 385])
def test_c_normalized_updates_entries_do_not_depend_on_the_batch(M):
    ops = _ops()
    base, x = _batch((M,), 71), _batch((M,), 72, spike=1)

    def run(b, v):
        multi = ops.update_multi([(b, v, 0.7, 0, None), (b, v, 0.7, 1, None)])
        return ops.normalized_axpy(b, v, 0.7), multi[0], multi[1]
    rows = _entries(run, (base, x))
    _assert_entries("normalized_updates", "M%d" % M, rows)
    for n, batch, one in rows:
        ref = base[n:n + 1].double() + 0.7 * L.unit_normalize_ref(x[n:n + 1])
        assert maxdiff(batch[0].cpu(), ref) < AXPY and maxdiff(batch[1].cpu(), ref) < AXPY, n


@pytest.mark.parametrize("dims", [(40, 132), (6, 10, 72)], ids=sid)
def test_c_jacobian_det_entries_do_not_depend_on_the_batch(dims):
    ops = _ops()
    d = len(dims)
    field, gout = 0.3 * _batch((d,) + dims, 32), _batch((1,) + dims, 33, spike=1)

    def run(f, w):
        f = f.requires_grad_(True)
        det = ops.jacobian_det(f)
        det.backward(w)
        st = ops.jacobian_stats(f.detach())
        return det.detach(), f.grad, st.neg, st.nonpos, st.min, st.max
    _assert_entries("jacobian_det", sid(dims), _entries(run, (field, gout)))
