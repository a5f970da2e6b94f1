"""Closed forms of the supervised losses of advchain/common/loss.py (contour_loss, cross_entropy_2D), written from their
specification rather than from the reference's code, in any dtype / on any device torch runs (tests only).

contour_loss: the reference's filters sum over the class axis, so with S the object classes,
    u = sum_{c in S} input_c - sum_{c in S} T_c,   w = mean of m^2 over the first min(|S|, mask channels) mask channels,
    2D: 1/2 [mean(w (Sx*u)^2) + mean(w (Sy*u)^2)],   3D: 1/3 [2 mean(w (A*u)^2) + mean(w (B*u)^2)],
zero padding, means over N * voxels.
cross_entropy_2D: -sum w_y log p_y (labels, -100 ignored) or -sum_c w_c t_c log p_c (soft), w = weight / sum(weight) * K,
divided by N*H*W when size_average."""
import torch
import torch.nn.functional as F

_H = [1.0, 2.0, 1.0]
_HP = [1.0, 0.0, -1.0]


def _stencils(nd, dtype, device):
    h = torch.tensor(_H, dtype=dtype, device=device)
    hp = torch.tensor(_HP, dtype=dtype, device=device)
    if nd == 2:
        A = h[:, None] * hp[None, :]                       # Sobel-x [[1,0,-1],[2,0,-2],[1,0,-1]]
        B = hp[:, None] * h[None, :]                       # Sobel-y
    else:
        A = h[:, None, None] * hp[None, :, None] * h[None, None, :]
        B = h[:, None, None] * h[None, :, None] * hp[None, None, :]
    return A[None, None], B[None, None]


def _correlate(u, k):
    """3^d cross-correlation with zero padding as a sum of shifted copies (no convolution backend: any dtype, any device)."""
    sp = u.shape[2:]
    up = F.pad(u, (1, 1) * len(sp))
    out = torch.zeros_like(u)
    for idx in torch.cartesian_prod(*[torch.arange(3)] * len(sp)).tolist():
        idx = [idx] if isinstance(idx, int) else idx
        wv = float(k[tuple(idx)])
        if wv != 0.0:
            out = out + wv * up[(slice(None), slice(None)) + tuple(slice(i, i + n) for i, n in zip(idx, sp))]
    return out


def contour_closed(x, target, ignore_background=True, one_hot_target=True, mask=None):
    """Value of contour_loss in x's dtype (differentiable w.r.t. x and a float target)."""
    N, K = x.shape[:2]
    sp = tuple(x.shape[2:])
    nd = len(sp)
    c0 = 1 if ignore_background else 0
    oc = K - c0
    if one_hot_target:
        T = F.one_hot(target.long().reshape((N,) + sp), K).movedim(-1, 1).to(x.dtype)
    else:
        T = target.to(x.dtype)
    u = (x[:, c0:].sum(1) - T[:, c0:].sum(1))[:, None]
    if mask is None:
        w = torch.ones_like(u)
    else:
        mc = min(oc, mask.shape[1])
        w = (mask[:, :mc].to(x.dtype) ** 2).mean(1, keepdim=True)
    A, B = _stencils(nd, x.dtype, x.device)
    a = _correlate(u, A[0, 0])
    b = _correlate(u, B[0, 0])
    if nd == 2:
        return 0.5 * ((w * a * a).mean() + (w * b * b).mean())
    return (2.0 * (w * a * a).mean() + (w * b * b).mean()) / 3.0


def ce_closed(x, target, weight=None, size_average=True):
    """Value of cross_entropy_2D in x's dtype (differentiable w.r.t. x and a soft target)."""
    N, K, H, W = x.shape
    lp = F.log_softmax(x, dim=1)
    if weight is None:
        w = torch.ones(K, dtype=x.dtype, device=x.device)
    else:
        w = torch.as_tensor(weight).to(device=x.device, dtype=x.dtype).reshape(-1)
        w = w / w.sum() * K
    if target.dim() == 3:
        ign = target == -100
        y = torch.where(ign, torch.zeros_like(target), target)
        per = -w[y] * lp.gather(1, y[:, None])[:, 0]
        per = torch.where(ign, torch.zeros_like(per), per)
        total = per.sum()
    else:
        total = -(w[None, :, None, None] * target.to(x.dtype) * lp).sum()
    return total / (N * H * W) if size_average else total
