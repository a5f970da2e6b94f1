"""Layouts that a solver-path operator must not care about, and the float64 references the layout tests hold it to.

Layouts: a contiguous tensor whose first element sits 4, 8 or 12 bytes into its storage (`offset_copy`: what a flat parameter
bucket, an arena allocator or a batch slice of odd-sized images hands out), and the non-contiguous forms autograd and slicing
produce (`strided_variants`, `expanded_grad`).

References, written plainly on the CPU in float64: F.grid_sample / F.affine_grid with align_corners=True on the planar grid
layout of tests/test_ops_gpu.to_planar, with autograd through them; a dense separable 9-tap convolution with zero padding for
the Gaussian (`gauss_ref`, with the prologues / epilogues of advchain_gauss_axis); F.interpolate for the upsampling tables; the
dense band matrices for the bias field (tests/cpu_backend.bias_apply); oracle.advchain_oracle.compose_fields and
unit_normalize on .double() inputs (both only call torch functions on their arguments, so they run in double as they are).

oracle.advchain_oracle.gaussian_smooth and identity_grid cannot run in double: the first builds a float32 window and hands it to
a convolution with the input (a dtype error for double input), the second returns float32.  The Gaussian reference here is
therefore the separable form below; the identity grid is built in double by `identity_grid64`.

Importing this module needs no GPU."""
import torch
import torch.nn.functional as F

from oracle import advchain_oracle as O


# ------------------------------------------------------------------------------------------------ layouts
def offset_copy(t, k=1):
    """The values of `t`, contiguous, k elements (k = 1, 2, 3: 4, 8, 12 bytes for float32) into a fresh storage."""
    assert k in (1, 2, 3) and t.element_size() == 4
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    view = buf[k:k + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
    return view


def strided_variants(t):
    """[(name, view)]: the values of `t` (at least 2 dims, the last two larger than 1) as non-contiguous tensors."""
    out = [("transposed", t.transpose(-1, -2).contiguous().transpose(-1, -2))]
    if t.dim() >= 3:
        C = t.shape[1]
        big = torch.empty((t.shape[0], C + 2) + tuple(t.shape[2:]), device=t.device, dtype=t.dtype)
        big[:, 1:1 + C] = t
        out.append(("channel_slice", big[:, 1:1 + C]))
    wide = torch.empty(tuple(t.shape[:-1]) + (2 * t.shape[-1],), device=t.device, dtype=t.dtype)
    wide[..., ::2] = t
    out.append(("step2", wide[..., ::2]))
    for name, v in out:
        assert not v.is_contiguous(), name
        assert torch.equal(v, t), name
    return out


def expanded_grad(shape, device):
    """What out.sum().backward() hands a backward: a scalar one expanded to the shape (every stride 0)."""
    g = torch.ones((), device=device).expand(tuple(shape))
    assert not g.is_contiguous() or g.numel() <= 1
    return g


# ------------------------------------------------------------------------------------------------ float64 references
def to_planar(grid_last):
    d = grid_last.shape[-1]
    return grid_last.permute(0, d + 1, *range(1, d + 1)).contiguous()


def planar_to_last(grid):
    d = grid.shape[1]
    return grid.permute(0, *range(2, 2 + d), 1)


def identity_grid64(n, dims):
    """O.identity_grid in double (channel order x, y[, z] <-> last .. first axis)."""
    axes = [torch.linspace(-1, 1, s, dtype=torch.float64) for s in dims]
    mesh = torch.meshgrid(axes, indexing="ij")
    return torch.stack(list(reversed(mesh)), 0).unsqueeze(0).repeat(n, *([1] * (len(dims) + 1))).contiguous()


def grid_sample_ref(inp, grid, gout=None, mode="bilinear", pad="zeros", clamp=False):
    """(out, grad_in, grad_grid) of F.grid_sample(inp, grid^T, align_corners=True) in double; grid planar (N,d,...)."""
    a = inp.detach().cpu().double().requires_grad_(True)
    g = grid.detach().cpu().double().requires_grad_(True)
    gp = torch.clamp(g, -1, 1) if clamp else g
    out = F.grid_sample(a, planar_to_last(gp), mode=mode, padding_mode=pad, align_corners=True)
    if gout is None:
        return out.detach(), None, None
    out.backward(gout.detach().cpu().double().expand_as(out))
    return out.detach(), a.grad, g.grad


def compose_self_ref(phi, gout=None):
    """(phi o phi, grad_phi) through O.compose_fields in double."""
    p = phi.detach().cpu().double().requires_grad_(True)
    out = O.compose_fields(p, p)
    if gout is None:
        return out.detach(), None
    out.backward(gout.detach().cpu().double())
    return out.detach(), p.grad


def chain_ref(phi0, n, gpos=None):
    """n squarings of phi0 in double: ([phi_1..phi_{n-1}], pos = (phi_n - phi_0) + identity, and what advchain_expo_chain_bwd
    returns for grad_pos = gpos: the gradient through the n squarings, d phi_n / d phi_0 applied to gpos -- the direct
    `- phi_0` term of pos is the caller's, as in advchain_demons_compose_pair_bwd)."""
    p0 = phi0.detach().cpu().double().requires_grad_(True)
    phis, phi = [], p0
    for _ in range(n):
        phi = O.compose_fields(phi, phi)
        phis.append(phi)
    pos = (phi - p0) + identity_grid64(p0.shape[0], p0.shape[2:])
    grad = None
    if gpos is not None:
        phi.backward(gpos.detach().cpu().double())
        grad = p0.grad
    return [f.detach() for f in phis[:-1]], pos.detach(), grad


def affine_warp_ref(inp, theta, gout=None, mode="bilinear", pad="zeros"):
    """(out, grad_in, grad_theta) of F.grid_sample(inp, F.affine_grid(theta)) with align_corners=True, in double."""
    a = inp.detach().cpu().double().requires_grad_(True)
    t = theta.detach().cpu().double().requires_grad_(True)
    out = F.grid_sample(a, F.affine_grid(t, a.size(), align_corners=True), mode=mode, padding_mode=pad, align_corners=True)
    if gout is None:
        return out.detach(), None, None
    out.backward(gout.detach().cpu().double().expand_as(out))
    return out.detach(), a.grad, t.grad


def _conv_axis(x, w, dim):
    """sum_k w[k] x[i + k - R] along `dim`, zero beyond the ends (the border rule of oracle.gaussian_smooth)."""
    R = len(w) // 2
    n = x.shape[dim]
    pad = [0, 0] * (x.dim() - 1 - dim) + [R, R]
    xp = F.pad(x, pad)
    out = torch.zeros_like(x)
    for k in range(len(w)):
        out = out + float(w[k]) * xp.narrow(dim, k, n)
    return out


def gauss_ref(x, weights, pre=0, post=0, scale=1.0, aux=None):
    """Separable Gaussian over every spatial axis of x (N, C, ...) in double with the prologues / epilogues of
    advchain_gauss_axis: pre 1: x * scale; pre 2: border_identity(x) - identity (the identity sampled with border padding at x is
    clamp(x, -1, 1)); post 1: + identity; post 2: * slope(aux), the derivative of that clamp at the positions `aux`."""
    x = x.detach().cpu().double()
    nd = x.dim() - 2
    ident = identity_grid64(x.shape[0], x.shape[2:])
    if pre == 1:
        x = x * scale
    elif pre == 2:
        x = torch.clamp(x, -1, 1) - ident
    for dim in range(2, 2 + nd):
        x = _conv_axis(x, weights, dim)
    if post == 1:
        x = x + ident
    elif post == 2:
        x = x * border_identity_slope(aux)
    return x


def border_identity_slope(pos):
    """d F.grid_sample(identity, pos, border)[c] / d pos[c]: 1 inside (-1, 1), 0 beyond -- as float32 autograd gives it.  The
    slope is the difference of two neighbouring identity coordinates (each rounded to 2^-24) times (S - 1) / 2: 1 to within
    (S - 1) 2^-24, 4e-6 for rows of 256, which is the reference's own rounding (the kernels repeat its arithmetic) and more
    than the Gaussian's bound; so this one factor is taken in the reference's precision, everything else in double."""
    p = pos.detach().cpu().float().requires_grad_(True)
    O.compose_fields(O.identity_grid(p.shape[0], p.shape[2:]), p).sum().backward()
    return p.grad.double()


def interp_ref(coef, full, gfull=None):
    """(F.interpolate(coef, full, align_corners=False), its adjoint applied to gfull) in double: the upsampling tables of
    advchain_amd.bands.upsample_tables."""
    c = coef.detach().cpu().double().requires_grad_(True)
    out = F.interpolate(c, size=tuple(full), mode="bilinear" if len(full) == 2 else "trilinear", align_corners=False)
    if gfull is None:
        return out.detach(), None
    out.backward(gfull.detach().cpu().double())
    return out.detach(), c.grad


def unit_normalize_ref(x):
    return O.unit_normalize(x.detach().cpu().double())
