"""The fixed-point scatters of the sampler backward against float64 autograd on the CPU, at high dynamic range.

Every scatter formulation of the warp backward (grid_sample and the self-composition of the squaring chain) adds
INTEGERS: a deposit is w * grad_out * 2^b / gmax, gmax the largest |grad_out| of the route's scale domain (common.h:
FixScale), and a cell goes back to float times gmax / 2^b.  A domain that misses a depositing sample wraps the int32 sum; a
domain wider than necessary costs the small gradients their precision; a factor 2^b / gmax that overflows fp32 at tiny
gradients turns the whole result into garbage.  The tests below pin each route's contract.

Routes, how a call reaches them, the kernels a rocprofv3 kernel trace of this module shows for them, and the scale domain
(b = bits below the domain's maximum):
  march    3D, halo = -H (H = 2..4; 5..8 one launch per channel): k_march_rowmax(64) + k_scatter_march3d (C = 3 self, C = 4
           warps), k_scatter_march3d_wide (C = 1 warps of rows <= 64, row maxima in its prologue), k_scatter_march3d_flat
           (self, rows of 68..80).  Domain: the rows the workgroup visits, halo rows and halo planes included.
           b = 23 / 22 / 21 for H = 2 / 3 / 4, 18 for H = 5..8.
  rows2d   2D, halo = -H (3..16, squarings ..32): k_march_rowmax + k_scatter_rows2d.  Domain: the rows visited.
           b = 25 / 24 / 22 / 20 / 18 for H <= 2 / 4 / 8 / 16 / 32.  In advchain_expo_chain_bwd consecutive launches hand
           the row maxima of their output to the next one (no k_march_rowmax between them).
  tiled    3D, halo = 0 (and 2D warps the window scatter does not take, C = 3): k_scatter_prepare + k_scatter_rows
           (+ k_scatter_overflow).  Domain: the samples of the workgroup's source region, tile + halo (until round 24 the WHOLE
           grad_out tensor, every batch entry: tests/test_layout_gpu.py part C found an entry's bits depending on its
           neighbours).  b = 30, 64-bit LDS cells.  A1 / A2 below still hold it to the bounds of the wider domain; A5 is bitwise.
  window   3D halo >= 2, every 2D halo the other routes decline: k_scatter_window2d / k_scatter_window3d.  Domain: the
           tile's own samples.  b = 20; tiles flush with float atomics, so results are not bitwise reproducible.
  det      the window route under ops.set_deterministic(True): k_det_absmax + k_scatter_window* + k_det_convert.  Domain:
           the batch entry.  b = 40, 64-bit global cells.
  affine   ops.affine_warp backward, theta gradient off / on: k_affine_box_gin.  Domain: the tile's sample box (with the
           theta gradient: the output tiles covering it, reach two tiles).  b = 30 - log2(corners a cell can receive).
  gather   |disp| < 1 voxel, halo = -1: k_adjoint_gather* / k_adjoint_march*; floats, no scale (control group).

Contract, asserted per route (tolerances add the fp32 floor of the sampling arithmetic: positions and weights are fp32,
the reference is float64, 2e-5 of the largest reference value, 5e-5 for the affine positions through theta; fields keep
their sampling positions off the grid lines, where the fp32 and float64 positions could pick different cells):
  A1  no wraparound: per batch entry, max|got - ref| <= 2^-(b-6) * max|grad_out of that entry|.
  A2  the scale is local: cells farther than the route's reach (its row block + 2H + 2 rows) from every spike keep
      2e-5 * |ref| + 2^-(b-4) * (the local max).  The tiled route (domain "tensor" below, from when its scale was the
      whole tensor's maximum): A1 against the tensor's maximum instead.  The det route's domain is the entry: A1.
  A3  zeros: where no non-zero sample reaches a cell the reference is exactly 0 and so is the result; an all-zero entry
      gives exact zeros, never NaN.
  A4  scale invariance: got(2^k g) == 2^k got(g) bit for bit for k = +-60 (the window route: to A1, its flush order
      varies); for k = -90, -100, -112, +100 the result is finite and meets A1 against 2^k ref.
  A5  entries are independent: entry 0's result is bitwise unchanged when entry 1 is 2^20 or 2^-20 times larger
      (window: to A1 against entry 0's own maximum; tiled: A1 against the tensor max, and bitwise as well since its scale
      is the workgroup's own -- also tests/test_layout_gpu.py part C).
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rand
from tests.test_ops_gpu import _smooth_field

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32 = 2e-5                     # fp32 floor of the sampling arithmetic against a float64 reference (relative)
SWEEP = (-112, -100, -90, -60, 0, 60, 100)


def _ops():
    from advchain_amd import ops
    return ops


def _sheared(dims, amp, seed, shear):
    """identity + a smooth field of ~amp voxels + a y displacement of `shear` voxels that varies along x: samples of the
    rows either side of a workgroup's own rows land in them.  No sampling position lies within 2e-4 voxels of a grid
    line: there the derivative of the interpolation w.r.t. the position jumps, and the fp32 position of the kernels
    (rounded to ~1e-5 voxels) and the float64 one of the reference could fall on different sides of the kink."""
    phi = _smooth_field(dims, amp, seed).double()
    d = len(dims)
    W, Hy = dims[-1], dims[-2]
    x = torch.linspace(-1.0, 1.0, W, dtype=torch.float64).view(*([1] * (d - 1)), W)
    phi[:, 1] += (shear * 2.0 / (Hy - 1)) * x
    return _off_kinks(phi)


def _off_kinks(phi):
    """phi with every sampling position at least 2e-4 voxels away from a grid line (float32)"""
    phi = phi.double().clone()
    dims = tuple(phi.shape[2:])
    d = len(dims)
    for a in range(d):
        S = dims[d - 1 - a]
        u = (phi[:, a] + 1.0) * 0.5 * (S - 1)
        r = torch.round(u)
        near = (u - r).abs() < 2e-4
        u = torch.where(near, r + torch.where(u >= r, 2e-4, -2e-4), u)
        phi[:, a] = u / (S - 1) * 2.0 - 1.0
    return phi.float().contiguous()


def _rows2d_ty(C, W, H):
    """owned rows of a k_scatter_rows2d workgroup (rows2d_tile in scatter_march.hip)"""
    nseg = (W + 63) // 64
    ty = 32 if H >= 8 else 16
    while ty > 4 and (C * ty * W * 4 > 49152 or ty * nseg > 64):
        ty //= 2
    return ty


def _march_bits(H):
    return 23 if H <= 2 else 22 if H == 3 else 21 if H == 4 else 18


def _rows2d_bits(H):
    return 25 if H <= 2 else 24 if H <= 4 else 22 if H <= 8 else 20 if H <= 16 else 18


class Route(object):
    """One backward formulation: `run(g)` on the GPU, `ref(g)` in float64 on the CPU (both linear in g)."""

    def __init__(self, name, kind, dims, halo, bits, amp=0.0, shear=0.0, C=None, ty=8, reach=None, det=False,
                 chain=None, domain="local", theta_grad=False, bitwise=True, pad="zeros", N=2, fp=FP32):
        self.name, self.kind, self.dims, self.halo, self.bits = name, kind, tuple(dims), halo, bits
        self.amp, self.shear, self.det, self.chain, self.domain = amp, shear, det, chain, domain
        self.theta_grad, self.bitwise, self.pad, self.N, self.ty, self.fp = theta_grad, bitwise, pad, N, ty, fp
        d = len(dims)
        self.C = d if kind == "self" else C
        H = abs(halo) if halo else max(1, int(math.ceil(amp + shear)))
        self.reach = reach if reach is not None else ty + 2 * H + 2
        self._setup = None

    def __repr__(self):
        return self.name

    def shape(self):
        return (self.N, self.C) + self.dims

    def setup(self):
        if self._setup is not None:
            return self._setup
        ops = _ops()
        d = len(self.dims)
        s = {}
        if self.kind in ("self", "warp"):
            phi = _sheared(self.dims, self.amp, 61, self.shear)
            bound = min([-h for h in (self.halo, self.chain) if h is not None and h < 0] or [0])
            if bound:              # an exact bound must hold: the measured displacement sits below it
                measured = float(ops.raw_max_displacement(phi.to(DEV)).item())
                assert measured < bound - 0.001, (self.name, measured)
            s["phi"] = phi
            if self.kind == "warp":
                s["inp"] = rand(self.shape(), 63)
        else:   # affine
            g = torch.Generator().manual_seed(11)
            s["inp"] = torch.rand(self.shape(), generator=g)
            s["theta"] = torch.eye(d, d + 1).repeat(self.N, 1, 1) + 0.01 * torch.randn(self.N, d, d + 1, generator=g)
        self._setup = s
        return s

    # ---- GPU
    def run(self, g):
        ops = _ops()
        s = self.setup()
        old = ops.is_deterministic()
        ops.set_deterministic(self.det)
        try:
            if self.kind == "affine":
                xg = s["inp"].to(DEV).requires_grad_(True)
                tg = s["theta"].to(DEV).requires_grad_(self.theta_grad)
                ops.affine_warp(xg, tg, padding_mode=self.pad).backward(g.to(DEV))
                out = xg.grad
            elif self.kind == "warp":
                out = ops.raw_grid_sample_bwd(g.to(DEV), s["inp"].to(DEV), s["phi"].to(DEV), 0, ops.pad_code(self.pad),
                                              False, True, False, self.halo)[0]
            else:
                pd = s["phi"].to(DEV)
                ws = ops._scatter_workspace(self.N, self.dims, DEV)
                if self.chain is None:
                    out = ops.raw_compose_self_bwd(g.to(DEV), pd, ws, chain=False, halo=self.halo)
                else:           # a first launch (halo self.chain), then this route's launch chained after it
                    first = ops.raw_compose_self_bwd(g.to(DEV), pd, ws, chain=False, halo=self.chain)
                    out = ops.raw_compose_self_bwd(first, pd, ws, chain=True, halo=self.halo)
            torch.cuda.synchronize()
            return out.cpu()
        finally:
            ops.set_deterministic(old)

    # ---- float64 reference
    def ref(self, g):
        s = self.setup()
        g = g.double()
        if self.kind == "affine":
            x = s["inp"].double().requires_grad_(True)
            grid = F.affine_grid(s["theta"].double(), list(x.shape), align_corners=True)
            F.grid_sample(x, grid, padding_mode=self.pad, align_corners=True).backward(g)
            return x.grad
        if self.kind == "warp":
            x = s["inp"].double().requires_grad_(True)
            d = len(self.dims)
            F.grid_sample(x, s["phi"].double().permute(0, *range(2, d + 2), 1), padding_mode=self.pad,
                          align_corners=True).backward(g)
            return x.grad
        from oracle import advchain_oracle as O
        steps = 1 if self.chain is None else 2
        for _ in range(steps):
            p = s["phi"].double().clone().requires_grad_(True)
            O.compose_fields(p, p).backward(g)
            g = p.grad
        return g

    def quantum(self):
        return 2.0 ** -(self.bits - 6)


H3 = 2     # (the tiled route's 3D tile halo)
ROUTES = [
    # march: every kernel form; rows 40 (k_scatter_march3d), 96 (x segments), 72 (flat), C = 1 warps (wide), H = 6 (per channel)
    Route("march_self_h2", "self", (6, 112, 40), -2, _march_bits(2), amp=0.9, shear=0.9),
    Route("march_self_h3_seg", "self", (5, 112, 96), -3, _march_bits(3), amp=1.2, shear=1.4),
    Route("march_self_h4_flat", "self", (6, 112, 72), -4, _march_bits(4), amp=1.6, shear=1.9),
    Route("march_self_h6", "self", (6, 112, 40), -6, _march_bits(6), amp=2.5, shear=3.0),
    Route("march_wide_c1_h3", "warp", (6, 144, 40), -3, _march_bits(3), amp=1.2, shear=1.4, C=1, ty=16),
    Route("march_warp_c4_h2", "warp", (5, 112, 40), -2, _march_bits(2), amp=0.9, shear=0.9, C=4, pad="border"),
    # rows2d: self H = 4 / 12 and image warps C = 1 / 4
    Route("rows2d_self_h4", "self", (120, 100), -4, _rows2d_bits(4), amp=1.5, shear=2.0, ty=_rows2d_ty(2, 100, 4)),
    Route("rows2d_self_h12", "self", (200, 130), -12, _rows2d_bits(12), amp=5.0, shear=6.0, ty=_rows2d_ty(2, 130, 12)),
    Route("rows2d_warp_c1_h6", "warp", (140, 90), -6, _rows2d_bits(6), amp=2.4, shear=3.0, C=1, ty=_rows2d_ty(1, 90, 6)),
    Route("rows2d_warp_c4_h3", "warp", (130, 72), -3, _rows2d_bits(3), amp=1.1, shear=1.4, C=4, ty=_rows2d_ty(4, 72, 3),
          pad="border"),
    # tiled (held to the bound of a whole-tensor scale, see the docstring); chained after a tiled, a march and a window launch
    Route("tiled_self_3d", "self", (6, 40, 40), 0, 30, amp=0.9, shear=0.6, domain="tensor"),
    Route("tiled_warp_3d_c2", "warp", (6, 40, 40), 0, 30, amp=0.9, shear=0.6, C=2, domain="tensor"),
    Route("tiled_warp_2d_c3", "warp", (40, 72), 0, 30, amp=2.0, shear=1.5, C=3, domain="tensor"),
    Route("tiled_after_tiled", "self", (6, 40, 40), 0, 30, amp=0.9, shear=0.6, chain=0, domain="tensor"),
    Route("tiled_after_march", "self", (6, 40, 40), 0, 23, amp=0.9, shear=0.6, chain=-2, domain="tensor"),
    Route("tiled_after_window", "self", (6, 40, 40), 0, 20, amp=0.9, shear=0.6, chain=4, domain="tensor", bitwise=False),
    # window: per-tile scale, float-atomic flush
    Route("window_self_3d", "self", (8, 96, 40), 8, 20, amp=2.5, shear=2.0, bitwise=False),
    Route("window_warp_3d_c4", "warp", (6, 96, 40), 8, 20, amp=2.0, shear=2.0, C=4, bitwise=False),
    Route("window_self_2d", "self", (256, 96), 8, 20, amp=3.0, shear=3.0, ty=32, bitwise=False),
    Route("window_warp_2d_c2", "warp", (256, 96), 0, 20, amp=3.0, shear=3.0, C=2, ty=32, bitwise=False),
    # det: the window route's 64-bit twin, per-entry scale
    Route("det_self_3d", "self", (8, 64, 40), 8, 40, amp=2.5, shear=2.0, det=True, domain="entry"),
    Route("det_warp_2d_c1", "warp", (160, 96), 8, 40, amp=3.0, shear=3.0, C=1, det=True, domain="entry"),
    # affine box (the corner count of a cell costs up to ~4 bits of the 2^30; positions come through theta in fp32: a wider
    # fp32 floor).  With the theta gradient the scale is the maximum of the 32 x 32 (3D: 16 x 16 x 8) tiles that cover the
    # sample box: a reach of two tiles
    Route("affine_2d", "affine", (160, 96), 0, 26, C=4, reach=48, fp=5e-5),
    Route("affine_2d_theta", "affine", (224, 96), 0, 26, C=4, reach=72, theta_grad=True, fp=5e-5),
    Route("affine_3d_theta", "affine", (12, 128, 32), 0, 24, C=1, reach=40, theta_grad=True, fp=5e-5),
    # gather forms: floats (control group)
    Route("gather_self_2d", "self", (64, 80), -1, 24, amp=0.4, shear=0.4),
    Route("gather_warp_3d_c1", "warp", (6, 64, 40), -1, 24, amp=0.4, shear=0.4, C=1),
]
BY_NAME = {r.name: r for r in ROUTES}


# ---------------------------------------------------------------------------------------------------------------
# grad_out patterns
def _spike_cells(route):
    """(y, x) of the spikes: the last / first own row of two neighbouring workgroups (rows ty - 1, ty); the first row of the
    last-but-one row block, ONLY a halo row for the block above it, whose own rows hold no spike (the sheared field
    carries its samples into that block's rows); the last row (partial block); x: tile corners (63 / 64), the partial
    last row segment, the edges; 3D: on planes 0, the middle (a z-halo plane of a chunk) and the last."""
    S1, W = route.dims[-2], route.dims[-1]
    ty = route.ty
    nb = (S1 + ty - 1) // ty
    ys = [ty - 1, ty, (nb - 2) * ty, S1 - 1]
    xs = [0, min(W - 1, 63), min(W - 1, 64), W - 1, W // 3]
    return ys, xs


def spikes(route, b, seed=5):
    g = b * torch.rand(route.shape(), generator=torch.Generator().manual_seed(seed))
    ys, xs = _spike_cells(route)
    d = len(route.dims)
    zs = [0, route.dims[0] // 2, route.dims[0] - 1] if d == 3 else [None]
    sign = 1.0
    for n in range(route.N):
        for c in range(route.C):
            for y in ys:
                for x in xs:
                    for z in zs:
                        idx = (n, c, y, x) if z is None else (n, c, z, y, x)
                        g[idx] = sign
                        sign = -sign
    return g, ys


def _far_rows(route, ys):
    S1 = route.dims[-2]
    far = torch.tensor([all(abs(y - s) > route.reach for s in ys) for y in range(S1)])
    return far


def _check_a1(route, got, ref, g, what):
    """A1 per batch entry (got, ref and g in the same units; ref float64)."""
    for n in range(route.N):
        gmax = float(g[n].abs().max()) if route.domain != "tensor" else float(g.abs().max())
        rmax = float(ref[n].abs().max())
        err = float((got[n].double() - ref[n]).abs().max())
        tol = route.quantum() * gmax + route.fp * rmax
        if route.chain is not None:      # two launches: the intermediate's maximum scales the first one's quantum
            tol += 2.0 ** -(route.bits - 6) * 4.0 * gmax
        assert err <= tol, (route.name, what, n, err, tol, gmax)


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1e-3, 1e-6])
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_spikes_over_background(route, b):
    """+-1 spikes at workgroup / tile / segment boundaries over a background of b * rand: A1 everywhere; A2 on the rows
    out of every spike's reach (their results must keep the background's own precision)."""
    g, ys = spikes(route, b)
    got, ref = route.run(g), route.ref(g)
    assert torch.isfinite(got).all(), route.name
    _check_a1(route, got, ref, g, "spikes")
    if route.domain != "local":
        return
    far = _far_rows(route, ys)
    assert int(far.sum()) >= 8, (route.name, int(far.sum()))       # the geometry leaves rows to look at
    sel = (Ellipsis, far, slice(None))
    gf, rf, of = g[sel], ref[sel], got[sel].double()
    for n in range(route.N):
        lmax = b
        err = (of[n] - rf[n]).abs()
        tol = route.fp * (rf[n].abs() + lmax) + 2.0 ** -(route.bits - 4) * lmax
        worst = float((err - tol).max())
        assert worst <= 0, (route.name, n, float(err.max()), float(rf[n].abs().max()), worst)
        assert float(gf[n].abs().max()) <= b


@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_exact_zeros(route):
    """A3: whole rows / planes of zeros next to non-zero ones, an all-zero batch entry, a single non-zero voxel."""
    d = len(route.dims)
    S1 = route.dims[-2]
    g = rand(route.shape(), 7)
    g[:, :, ..., : S1 // 3, :] = 0.0         # a band of zero rows (planes in 3D: the leading third of the z range too)
    if d == 3:
        g[:, :, : max(1, route.dims[0] // 3)] = 0.0
    g[1] = 0.0                               # an all-zero entry
    got, ref = route.run(g), route.ref(g)
    assert torch.isfinite(got).all(), route.name
    assert bool((got[1] == 0).all()), route.name
    zero = ref == 0
    assert int(zero[0].sum()) > 0
    assert bool((got[zero] == 0).all()), (route.name, int((got[zero] != 0).sum()))
    _check_a1(route, got, ref, g, "zero bands")
    # one non-zero voxel in the whole tensor
    g1 = torch.zeros(route.shape())
    g1[(0, route.C - 1) + tuple(s // 2 for s in route.dims)] = 0.75
    got1, ref1 = route.run(g1), route.ref(g1)
    z1 = ref1 == 0
    assert bool((got1[z1] == 0).all()), (route.name, int((got1[z1] != 0).sum()))
    _check_a1(route, got1, ref1, g1, "single voxel")


@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_magnitude_sweep(route):
    """A4: the same rand gradient times 2^k.  k = +-60: the result scales by exactly 2^k (power-of-two scaling is exact in
    fp32 and cancels out of the fixed-point scale); the extremes stay finite and meet A1 against 2^k ref."""
    g = rand(route.shape(), 9)
    ref = route.ref(g)
    base = route.run(g)
    _check_a1(route, base, ref, g, "k=0")
    for k in SWEEP:
        if k == 0:
            continue
        gk = g * 2.0 ** k
        got = route.run(gk)
        assert torch.isfinite(got).all(), (route.name, k, int((~torch.isfinite(got)).sum()))
        unscaled = got.double() * 2.0 ** -k
        if abs(k) == 60 and route.bitwise:
            assert torch.equal(got, base * 2.0 ** k), (route.name, k, float((unscaled - base.double()).abs().max()))
        _check_a1(route, unscaled, ref, g, "k=%d" % k)


@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_entry_contrast(route):
    """A5: entry 1 at 2^20 and 2^-20 times entry 0's magnitude leaves entry 0's result alone."""
    g = rand(route.shape(), 13)
    base = route.run(g)
    ref0 = route.ref(g)
    for k in (20, -20):
        gc = g.clone()
        gc[1] *= 2.0 ** k
        got = route.run(gc)
        assert torch.isfinite(got).all(), (route.name, k)
        if route.domain == "tensor":
            # (the bound of a scale shared by the entries, which the tiled route had until round 24; its per-region scale meets it)
            _check_a1(route, got, ref0 * torch.tensor([1.0, 2.0 ** k], dtype=torch.float64).view(-1, *([1] * (got.dim() - 1))),
                      gc, "contrast %d" % k)
            if route.bitwise:      # ... and, its scale being the workgroup's own since round 24, entry 0 keeps its bits
                assert torch.equal(got[0], base[0]), (route.name, k, float((got[0] - base[0]).abs().max()))
        elif route.bitwise:
            assert torch.equal(got[0], base[0]), (route.name, k, float((got[0] - base[0]).abs().max()))
        else:
            err = float((got[0].double() - ref0[0]).abs().max())
            tol = route.quantum() * float(g[0].abs().max()) + route.fp * float(ref0[0].abs().max())
            assert err <= tol, (route.name, k, err, tol)


# ---------------------------------------------------------------------------------------------------------------
# full-size geometry: cfg-3's 3D volume on the march scatter, cfg-2's 2D image on the whole-row scatter
@pytest.mark.parametrize("route", [
    Route("march_self_cfg3", "self", (128, 128, 64), -2, _march_bits(2), amp=0.9, shear=0.9),
    Route("rows2d_self_cfg2", "self", (256, 256), -8, _rows2d_bits(8), amp=2.5, shear=4.5, ty=_rows2d_ty(2, 256, 8)),
], ids=repr)
def test_full_size_geometry(route):
    g, ys = spikes(route, 1e-6)
    got, ref = route.run(g), route.ref(g)
    _check_a1(route, got, ref, g, "spikes")
    far = _far_rows(route, ys)
    sel = (Ellipsis, far, slice(None))
    for n in range(route.N):
        err = (got[sel][n].double() - ref[sel][n]).abs()
        tol = FP32 * (ref[sel][n].abs() + 1e-6) + 2.0 ** -(route.bits - 4) * 1e-6
        assert float((err - tol).max()) <= 0, (route.name, n, float(err.max()))
    tiny = route.run(g * 2.0 ** -112)
    assert torch.isfinite(tiny).all()
    _check_a1(route, tiny.double() * 2.0 ** 112, ref, g, "k=-112")


# ---------------------------------------------------------------------------------------------------------------
# the whole-row handover of advchain_expo_chain_bwd
def _expo_chain(dims, amp, shear, n):
    ops = _ops()
    phi0 = _sheared(dims, amp, 95, shear).to(DEV)
    fields = [phi0]
    for _ in range(n - 1):     # (the squarings, moved off the kinks as well: the backward takes any fields)
        fields.append(_off_kinks(ops.raw_compose_self_fwd(fields[-1]).cpu()).to(DEV))
    disp = [float(ops.raw_max_displacement(f).item()) for f in fields]
    halos = [ops.squaring_halo(disp[m], 2) for m in range(n - 1, -1, -1)]
    return fields, halos


def _chain_bwd(fields, halos, gpos):
    from advchain_amd import _lib
    ops = _ops()
    N, dims, n = fields[0].shape[0], tuple(fields[0].shape[2:]), len(fields)
    lib = _lib.load()
    stack = torch.stack(fields[1:]).contiguous() if n > 1 else None
    out, scratch = torch.empty_like(gpos), torch.empty_like(gpos)
    ws = ops._scatter_workspace(N, dims, DEV)
    _lib.check(lib.advchain_expo_chain_bwd(ops._ptr(gpos), ops._ptr(fields[0]), ops._ptr(stack), ops._ptr(out), ops._ptr(scratch),
                                           ops._ptr(ws), (ctypes.c_int32 * n)(*halos), N, 2, _lib.dims_array(dims), n,
                                           ops._stream()), "expo_chain_bwd")
    per_step, g = None, gpos
    for i, phi in enumerate(reversed(fields)):
        g = ops.raw_compose_self_bwd(g, phi, ws, chain=i > 0, halo=halos[i])
    per_step = g
    torch.cuda.synchronize()
    return out.cpu(), per_step.cpu()


@pytest.mark.parametrize("b", [1e-3, 1e-6])
def test_rows2d_handover_in_the_squaring_chain(b):
    """Consecutive k_scatter_rows2d launches of advchain_expo_chain_bwd take the row maxima their predecessor left behind
    instead of a k_march_rowmax pass: with spikes over a small background (rows whose maxima differ by 10^6) the chain
    must equal the per-step calls bit for bit, meet A1 against the float64 chain, and scale exactly by 2^+-60."""
    from oracle import advchain_oracle as O
    dims, n = (120, 96), 3
    fields, halos = _expo_chain(dims, 1.2, 1.4, n)
    assert all(h <= -3 for h in halos), halos          # every step on the whole-row scatter: a handover at each join
    route = Route("rows2d_chain", "self", dims, halos[0], min(_rows2d_bits(-h) for h in halos), ty=16)
    g, _ = spikes(route, b)
    got, per_step = _chain_bwd(fields, halos, g.to(DEV))
    assert torch.equal(got, per_step), float((got - per_step).abs().max())
    ref = g.double()
    for f in reversed(fields):
        p = f.cpu().double().requires_grad_(True)
        O.compose_fields(p, p).backward(ref)
        ref = p.grad
    gm = [float(g[i].abs().max()) for i in range(2)]
    for i in range(2):
        err = float((got[i].double() - ref[i]).abs().max())
        tol = n * 2.0 ** -(route.bits - 6) * 8.0 * gm[i] + FP32 * float(ref[i].abs().max())
        assert err <= tol, (i, err, tol)
    for k in (60, -60, -112):
        gk, _ = _chain_bwd(fields, halos, (g * 2.0 ** k).to(DEV))
        assert torch.isfinite(gk).all(), k
        if abs(k) == 60:
            assert torch.equal(gk, got * 2.0 ** k), k
