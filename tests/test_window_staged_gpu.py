"""Staged form of the deterministic 2D window scatter (scatter_window.hip: the stage instantiation of k_scatter_window2d and
k_window_merge2d; include/advchain_hip.h: advchain_grid_sample_bwd_staged).

In deterministic mode the window scatter used to clear an int64 image of grad_in, take a maximum of grad_out per batch entry,
flush its LDS windows with 64-bit integer atomics and convert the image (the "int64 twin").  The staged form stores every tile's
window and a header instead, and a merge kernel sums the staged cells per grad_in pixel in registers.  What must hold:
  * grad_in and grad_grid are BIT FOR BIT those of the int64 twin (ops.WINDOW_STAGED = False gives the twin in the same
    process), for smooth fields, for fields whose windows outgrow the LDS budget (capped windows: the merge kernel rebuilds the
    corners the stage kernel left out) and for tiles that reach nothing; both are autograd's through F.grid_sample to the
    tolerance of the existing window-scatter tests;
  * repeats are equal, a batch entry does not depend on the rest of the batch, a non-finite grad_out is not dropped;
  * a solver call gives the same bits with either form, launch by launch and replayed from a hipGraph.
Every case uses the hint halo = 16 (the whole-row scatter and the gather form decline) and asserts through
advchain_last_bwd_route that the staged form / the twin really ran.
"""
import contextlib
import io
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import maxdiff, rand
from tests.test_ops_gpu import _smooth_field

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HALO = 16
PADS = (("zeros", True), ("zeros", False), ("border", False))      # (padding, clamp_grid)
CELLS_PER_CHANNEL = {1: 8192, 2: 4096, 4: 3072}                   # the LDS budget of a window (scatter_window.hip)


@pytest.fixture
def det():
    from advchain_amd import ops
    ops.set_deterministic(True)
    was = ops.WINDOW_STAGED
    try:
        yield ops
    finally:
        ops.WINDOW_STAGED = was
        ops.set_deterministic(False)


def _bwd(ops, staged, args, need_ggrid=True):
    """raw_grid_sample_bwd in the staged form or as the int64 twin; asserts which of the two ran"""
    ops.WINDOW_STAGED = staged
    try:
        gin, ggrid = ops.raw_grid_sample_bwd(*args, True, need_ggrid, HALO)
        assert ops.last_bwd_route() == ("window_staged" if staged else "window_int64"), ops.last_bwd_route()
    finally:
        ops.WINDOW_STAGED = True
    return gin, ggrid


def _bits(x):
    return x.view(torch.int32)


def _field3(dims, amp_px, seed):
    """three batch entries of identity + a smooth displacement of up to ~amp_px pixels"""
    return torch.cat([_smooth_field(dims, amp_px, seed), _smooth_field(dims, amp_px, seed + 1)[:1]]).contiguous()


def _autograd(inp, grid, wv, pad, clamp):
    a, g = inp.clone().requires_grad_(True), grid.clone().requires_grad_(True)
    gp = torch.clamp(g, -1, 1) if clamp else g
    (F.grid_sample(a, gp.permute(0, 2, 3, 1), padding_mode=pad, align_corners=True) * wv).sum().backward()
    return a.grad, g.grad


def _check_against_twin_and_autograd(ops, inp, grid, wv, pad, clamp, what):
    ref_in, ref_grid = _autograd(inp, grid, wv, pad, clamp)
    args = (wv.to(DEV), inp.to(DEV), grid.to(DEV), 0, ops.pad_code(pad), clamp)
    gin, ggrid = _bwd(ops, True, args)
    tin, tgrid = _bwd(ops, False, args)
    assert torch.equal(gin, tin) and torch.equal(ggrid, tgrid), what
    assert maxdiff(gin.cpu(), ref_in) < 5e-5 * max(1.0, float(ref_in.abs().max())), what
    assert maxdiff(ggrid.cpu(), ref_grid) < 5e-5 * max(1.0, float(ref_grid.abs().max())), what
    only, none = _bwd(ops, True, args, need_ggrid=False)
    tonly, _ = _bwd(ops, False, args, need_ggrid=False)
    assert none is None and torch.equal(only, tonly) and torch.equal(only, gin), what


@pytest.mark.parametrize("dims", [(64, 96), (100, 72), (33, 40)])
@pytest.mark.parametrize("amp_px", [20.0, 45.0])
def test_staged_form_equals_the_int64_twin_bit_for_bit(det, dims, amp_px):
    """Smooth fields of 20 / 45 px, N = 3, C = 1, 2, 4, zeros padding with and without a clamped grid and border padding, with
    and without grad_grid; (100, 72) and (33, 40) have partial tiles."""
    ops = det
    grid = (_field3(dims, amp_px, 41) * 1.02).contiguous()
    for C in (1, 2, 4):
        inp, wv = rand((3, C) + dims, 43 + C), rand((3, C) + dims, 53 + C)
        for pad, clamp in PADS:
            _check_against_twin_and_autograd(ops, inp, grid, wv, pad, clamp, (C, pad, clamp))


def _boxes(grid, pad, clamp):
    """CPU model of the box rule of k_scatter_window2d: per batch entry and 32 x 32 tile of samples, (ww, wh) of the bounding box
    of the valid corners (0 where a tile has none)."""
    N, _, H, W = grid.shape
    g = torch.clamp(grid, -1, 1) if clamp else grid
    x = ((g[:, 0] + 1) * 0.5) * (W - 1)
    y = ((g[:, 1] + 1) * 0.5) * (H - 1)
    if pad == "border":
        x, y = x.clamp(0, W - 1), y.clamp(0, H - 1)
    ix, iy = torch.floor(x).long(), torch.floor(y).long()
    big = 1 << 30

    def span(i, S):
        v0, v1 = (i >= 0) & (i < S), (i + 1 >= 0) & (i + 1 < S)
        lo = torch.where(v0, i, torch.where(v1, i + 1, torch.full_like(i, big)))
        hi = torch.where(v1, i + 1, torch.where(v0, i, torch.full_like(i, -big)))
        return lo, hi
    xlo, xhi = span(ix, W)
    ylo, yhi = span(iy, H)
    out = []
    for n in range(N):
        for ty in range(0, H, 32):
            for tx in range(0, W, 32):
                s = (n, slice(ty, ty + 32), slice(tx, tx + 32))
                ww = max(int(xhi[s].max()) - int(xlo[s].min()) + 1, 0)
                wh = max(int(yhi[s].max()) - int(ylo[s].min()) + 1, 0)
                out.append((ww, wh))
    return out


def _capped(boxes, C):
    cells = CELLS_PER_CHANNEL[C]
    return [ww > 128 or (ww > 0 and wh > cells // min(ww, 128)) for ww, wh in boxes]


def _magnifying_grid(dims, N):
    """sampling position = centre + 5 (pixel - centre) + 3 px (sin(x / 17), cos(y / 13)): most tiles of samples land outside
    the image, the ones around the centre stretch over 160 x 160 pixels -- more than a window holds"""
    H, W = dims
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cy, cx = (H - 1) / 2, (W - 1) / 2
    px = cx + 5 * (xs - cx) + 3 * torch.sin(xs / 17)
    py = cy + 5 * (ys - cy) + 3 * torch.cos(ys / 13)
    g = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1])
    return torch.stack([g * (1 + 0.003 * n) for n in range(N)]).contiguous()


@pytest.mark.parametrize("pad", ["zeros", "border"])
def test_capped_windows_and_empty_tiles(det, pad):
    """(100, 200), a five-fold magnification: 1 (C = 1) or 2 (C = 2, 4) of the 28 tiles of an entry have a box beyond the LDS
    budget -- the corners outside the capped window are the merge kernel's -- and, with zeros padding, 26 tiles have no valid
    corner at all (border padding: none, every sample is clamped onto the image)."""
    ops = det
    dims, N = (100, 200), 2
    grid = _magnifying_grid(dims, N)
    boxes = _boxes(grid, pad, False)
    if pad == "zeros":
        assert any(ww * wh == 0 for ww, wh in boxes)
    for C in (1, 2, 4):
        assert any(_capped(boxes, C)), C
        inp, wv = rand((N, C) + dims, 83 + C), rand((N, C) + dims, 93 + C)
        _check_against_twin_and_autograd(ops, inp, grid, wv, pad, False, (C, pad))


def test_every_tile_capped_on_a_random_grid(det):
    """A uniformly random grid at (64, 96): the box of every tile is the whole image.  For C = 2 and C = 4 that is more than a
    window holds (4096 / 96 = 42 and 3072 / 96 = 32 rows of 64), so every tile is capped and every rectangle of the merge kernel
    walks every tile's samples again; for C = 1 the image fits (8192 / 96 = 85 rows) and the case runs the plain staged path."""
    ops = det
    dims, N = (64, 96), 2
    grid = (torch.rand((N, 2) + dims, generator=torch.Generator().manual_seed(7)) * 2 - 1).contiguous()
    for pad, clamp in (("zeros", False), ("border", False)):
        boxes = _boxes(grid, pad, clamp)
        for C in (1, 2, 4):
            assert all(_capped(boxes, C)) == (C != 1), (C, pad)
            inp, wv = rand((N, C) + dims, 23 + C), rand((N, C) + dims, 33 + C)
            _check_against_twin_and_autograd(ops, inp, grid, wv, pad, clamp, (C, pad))


@pytest.mark.parametrize("C", [1, 4])
def test_repeats_are_equal_and_an_entry_does_not_depend_on_the_batch(det, C):
    ops = det
    dims = (100, 72)
    grid = (_field3(dims, 30.0, 61) * 1.02).contiguous().to(DEV)
    inp, wv = rand((3, C) + dims, 63 + C).to(DEV), rand((3, C) + dims, 73 + C).to(DEV)
    args = (wv, inp, grid, 0, 0, True)
    gin, ggrid = _bwd(ops, True, args)
    for _ in range(3):
        again, gg2 = _bwd(ops, True, args)
        assert torch.equal(gin, again) and torch.equal(ggrid, gg2)
    one = tuple(t[1:2].contiguous() for t in (wv, inp, grid)) + (0, 0, True)
    alone, gg_alone = _bwd(ops, True, one)
    assert torch.equal(gin[1:2], alone) and torch.equal(ggrid[1:2], gg_alone)
    big = wv.clone()
    big[0] *= 1e6                      # the scale is the ENTRY's maximum: entry 1 does not see entry 0's
    scaled, _ = _bwd(ops, True, (big, inp, grid, 0, 0, True))
    assert torch.equal(scaled[1:2], alone)


@pytest.mark.parametrize("C", [1, 4])
def test_non_finite_grad_out_is_not_dropped(det, C):
    """A NaN in entry 0 and an inf in entry 1: their outputs are the twin's bit patterns (NaN / inf, nothing finite made up);
    entry 2 is what it is without them."""
    ops = det
    dims = (64, 96)
    grid = (_field3(dims, 25.0, 81) * 1.02).contiguous().to(DEV)
    inp, wv = rand((3, C) + dims, 83 + C).to(DEV), rand((3, C) + dims, 93 + C).to(DEV)
    clean, _ = _bwd(ops, True, (wv, inp, grid, 0, 0, True))
    assert bool(torch.isfinite(clean).all())
    bad = wv.clone()
    bad[0, 0, 40, 50] = float("nan")
    bad[1, C - 1, 7, 90] = float("inf")
    args = (bad, inp, grid, 0, 0, True)
    gin, ggrid = _bwd(ops, True, args)
    tin, tgrid = _bwd(ops, False, args)
    assert torch.equal(_bits(gin), _bits(tin)) and torch.equal(_bits(ggrid), _bits(tgrid))
    assert not bool(torch.isfinite(gin[0]).any()) and not bool(torch.isfinite(gin[1]).any())
    assert torch.equal(gin[2], clean[2])


SOLVER_DIMS = (64, 64)        # the smallest size at which a later ascent step of this chain leaves the whole-row scatter (32, 48: never)


def _solver_outputs(ops, monkeypatch, staged, hip_graph):
    """what cfg-2's chain at 2 x 1 x SOLVER_DIMS leaves behind after its last call from fixed seeds, and the routes its image-warp
    backwards took (a replayed loop: three recorded calls, the capture, two replays)"""
    import bench
    routes = []
    real = ops.raw_grid_sample_bwd

    def noting(*a, **k):
        out = real(*a, **k)
        routes.append(ops.last_bwd_route())
        return out
    monkeypatch.setattr(ops, "raw_grid_sample_bwd", noting)
    ops.WINDOW_STAGED = staged
    try:
        batch = 2
        wl = dict(bench.WORKLOADS["cfg2"], dims=SOLVER_DIMS, batch=batch)
        solver = bench.build_solver(wl, DEV, None, hip_graph=hip_graph)
        solver.deterministic = True
        torch.manual_seed(11)
        data = torch.rand(batch, 1, *wl["dims"], device=DEV)
        model = bench.make_model(2).to(DEV)
        for rep in range(6 if hip_graph else 1):
            torch.manual_seed(13)
            with contextlib.redirect_stdout(io.StringIO()):
                loss = solver.adversarial_training(data=data, model=model, **bench.solver_kwargs(wl, DEV))
            assert math.isfinite(float(loss.detach()))
        outs = ([solver.adv_data.detach().clone(), solver.warped_back_adv_output.detach().clone()]
                + [t.param.detach().clone() for t in solver.chain_of_transforms])
    finally:
        ops.WINDOW_STAGED = True
        monkeypatch.setattr(ops, "raw_grid_sample_bwd", real)
    return solver, outs, routes


def test_solver_call_gives_the_same_bits_with_either_form(det, monkeypatch):
    """cfg-2's chain (noise, bias, morph, affine; five ascent steps) at 2 x 1 x 64 x 64: its last ascent steps warp by more
    than 16 px and take the window scatter.  Staged form against int64 twin from the same seeds: parameters, adversarial data and
    warped-back prediction equal bit for bit -- launch by launch, and with the ascent loop replayed from a hipGraph (the staging
    buffer is a torch.empty inside the captured region, nothing is read back; a replay follows its frozen launch plan, whose
    margins may pick other kernels than a launch-by-launch call does, so replay is compared with replay)."""
    ops = det
    _, staged, routes = _solver_outputs(ops, monkeypatch, True, False)
    assert "window_staged" in routes and "window_int64" not in routes, routes
    _, twin, routes_twin = _solver_outputs(ops, monkeypatch, False, False)
    assert "window_int64" in routes_twin and "window_staged" not in routes_twin, routes_twin
    for a, b in zip(staged, twin):
        assert torch.equal(a, b)
    solver, replayed, routes_graph = _solver_outputs(ops, monkeypatch, True, True)
    assert "window_staged" in routes_graph and "window_int64" not in routes_graph, routes_graph
    st = solver.graph_stats
    assert st["violations"] == 0 and st["replays"] >= 1 and st["refused"] == 0, st
    solver_twin, replayed_twin, _ = _solver_outputs(ops, monkeypatch, False, True)
    assert solver_twin.graph_stats["violations"] == 0 and solver_twin.graph_stats["replays"] >= 1, solver_twin.graph_stats
    for a, b in zip(replayed, replayed_twin):
        assert torch.equal(a, b)
    for a in replayed + staged:
        assert bool(torch.isfinite(a).all())
