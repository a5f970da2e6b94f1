"""Closed forms of the finite differences and the Jacobian determinant of 2D and 3D fields, in plain torch: slicing stencils
and the explicit determinant.  Test infrastructure: the float64 evaluation is what the HIP kernels are held to, the fp32 twin
(the same expressions on float32 tensors) measures what fp32 arithmetic itself costs and is the baseline a user could write
today.  Runs on CPU or GPU tensors; differentiable by autograd.

Conventions (those of the kernels): a field is (N, d, S0[, S1], S2)... channel c is the component along the spatial axis
counted from the LAST one (channel 0 = x = last axis).  The stencil along an axis: v[1] - v[0] at the first element,
v[-1] - v[-2] at the last, 0.5 (v[i+1] - v[i-1]) inside.  Displacement mode: J_ij = delta_ij + D_j f_i.  Positions mode: the
field is a sampling grid in normalised [-1, 1] coordinates (align_corners=True), J_ij = ((S_i - 1) / 2) D_j q_i, optionally
clamped to [-1, 1] first (torch.clamp: the gradient passes where -1 <= q <= 1)."""
import torch


def diff_axis(v, dim):
    """The stencil along `dim` (at least 2 elements)."""
    n = v.shape[dim]
    if n < 2:
        raise IndexError("index 1 is out of bounds for dimension %d with size %d" % (dim, n))
    parts = [v.narrow(dim, 1, 1) - v.narrow(dim, 0, 1)]
    if n > 2:
        parts.append(0.5 * (v.narrow(dim, 2, n - 2) - v.narrow(dim, 0, n - 2)))
    parts.append(v.narrow(dim, n - 1, 1) - v.narrow(dim, n - 2, 1))
    return torch.cat(parts, dim)


def image_diff(x):
    """(dx, dy[, dz]) of a (N, C, spatial...) batch: x along the last axis."""
    return tuple(diff_axis(x, x.dim() - 1 - j) for j in range(x.dim() - 2))


def _det(field, positions, clamp):
    nd = field.dim() - 2
    assert field.shape[1] == nd and nd in (2, 3)
    q = field.clamp(-1, 1) if clamp else field
    J = [[None] * nd for _ in range(nd)]
    for i in range(nd):
        comp = q[:, i]                                   # (N, spatial...)
        s = (field.shape[-1 - i] - 1) / 2.0              # component i runs along the axis -1 - i
        for j in range(nd):
            d = diff_axis(comp, comp.dim() - 1 - j)
            J[i][j] = s * d if positions else (1.0 + d if i == j else d)
    if nd == 2:
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
    else:
        det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
               + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
    return det.unsqueeze(1)


def jacobian_det64(field, positions=False, clamp=False):
    """The float64 closed form; `field` of any float dtype (converted first, so the rounding of the INPUT is not counted)."""
    return _det(field.double(), positions, clamp)


def jacobian_det32(field, positions=False, clamp=False):
    """The fp32 twin: the same expressions in float32."""
    return _det(field.float(), positions, clamp)


def stats_of(det):
    """(neg, nonpos, min, max) per batch entry of a determinant map; NaN counts as nonpos and is ignored by the extrema."""
    flat = det.flatten(1)
    num = ~torch.isnan(flat)
    inf = torch.full_like(flat, float("inf"))
    return ((flat < 0).sum(1), (~(flat > 0)).sum(1), torch.where(num, flat, inf).amin(1), torch.where(num, flat, -inf).amax(1))
