"""Closed forms of the soft Dice loss, of its gradient coefficients and of the fused Dice + cross entropy of common.loss
(dice_loss, dice_ce_loss, cross_entropy_3D), written from their specification, in any dtype / on any device torch runs (tests
only).  With p = softmax(x) over the K planes, t the one-hot labels or a soft target, sums over the counted voxels of entry n
(label -100: not counted; batch_dice: over n as well, N -> 1):

    I_nk = sum p_k t_k,  P_nk = sum p_k,  T_nk = sum t_k,  D_nk = P_nk + T_nk + smooth,  dice_nk = (2 I_nk + smooth) / D_nk
    omega_k = w_k / sum of the counted w_j  (class 0 not counted with ignore_background),  loss = 1 - 1/N sum_nk omega_k dice_nk
    dL/dp_k(v) = A_nk t_k(v) + B_nk,  dL/dt_k(v) = A_nk p_k(v) + B_nk,  A_nk = -2 c omega_k / D_nk,
    B_nk = c omega_k (2 I_nk + smooth) / D_nk^2,  c = 1/N (1 for batch_dice)."""
import torch
import torch.nn.functional as F

from tests.seg_loss_forms import ce_closed


def targets_and_mask(x, target):
    """(t, m): the target as (N,K,dims) maps in x's dtype and the (N,1,dims) mask of the counted voxels."""
    K = x.shape[1]
    if target.dim() == x.dim() - 1:
        ign = target == -100
        y = torch.where(ign, torch.zeros_like(target), target)
        t = F.one_hot(y, K).movedim(-1, 1).to(x.dtype)
        return t, (~ign)[:, None].to(x.dtype)
    return target.to(x.dtype), torch.ones_like(x[:, :1])


def omega_of(K, weight, ignore_background, dtype, device):
    w = torch.ones(K, dtype=dtype, device=device) if weight is None else \
        torch.as_tensor(weight).to(device=device, dtype=dtype).reshape(-1).clone()
    if ignore_background:
        w[0] = 0.0
    return w / w.sum()


def dice_sums(p, t, m, batch_dice):
    """I, P, T of shape (rows, K): rows = N, or 1 for batch_dice."""
    axes = tuple(range(2, p.dim()))
    I, P, T = (p * t * m).sum(axes), (p * m).sum(axes), (t * m).sum(axes)
    if batch_dice:
        I, P, T = I.sum(0, keepdim=True), P.sum(0, keepdim=True), T.sum(0, keepdim=True)
    return I, P, T


def dice_from_maps(p, t, m, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5):
    """The loss as a function of the probability maps p and the target maps t (differentiable w.r.t. both)."""
    I, P, T = dice_sums(p, t, m, batch_dice)
    dice = (2.0 * I + smooth) / (P + T + smooth)
    omega = omega_of(p.shape[1], weight, ignore_background, p.dtype, p.device)
    return 1.0 - (dice * omega[None]).sum() / dice.shape[0]


def dice_closed(x, target, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5):
    """Value of dice_loss in x's dtype (differentiable w.r.t. x and a soft target)."""
    t, m = targets_and_mask(x, target)
    return dice_from_maps(torch.softmax(x, 1), t, m, weight, ignore_background, batch_dice, smooth)


def dice_coefficients(p, t, m, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5):
    """(A, B) of shape (rows, K): dL/dp_k(v) = A t_k(v) + B at a counted voxel, dL/dt_k(v) = A p_k(v) + B."""
    I, P, T = dice_sums(p, t, m, batch_dice)
    D = P + T + smooth
    c = 1.0 / I.shape[0]
    omega = omega_of(p.shape[1], weight, ignore_background, p.dtype, p.device)[None]
    return -2.0 * c * omega / D, c * omega * (2.0 * I + smooth) / (D * D)


def ce_closed_nd(x, target, weight=None, size_average=True):
    """ce_closed for 2D and 3D input: the cross entropy only sees planes of voxels."""
    if x.dim() == 4:
        return ce_closed(x, target, weight, size_average)
    N, K, D, H, W = x.shape
    tgt = target.reshape(N, D, H * W) if target.dim() == 4 else target.reshape(N, K, D, H * W)
    return ce_closed(x.reshape(N, K, D, H * W), tgt, weight, size_average)


def dice_ce_closed(x, target, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5, dice_weight=1.0,
                   ce_weight=1.0):
    """Value of dice_ce_loss: its own expression (one softmax, one log), not the sum of the two closed forms above."""
    t, m = targets_and_mask(x, target)
    K = x.shape[1]
    lp = F.log_softmax(x, 1)
    p = lp.exp()
    dice = dice_from_maps(p, t, m, weight, ignore_background, batch_dice, smooth)
    w = torch.ones(K, dtype=x.dtype, device=x.device) if weight is None else \
        torch.as_tensor(weight).to(device=x.device, dtype=x.dtype).reshape(-1)
    w = w / w.sum() * K
    w = w.reshape((1, K) + (1,) * (x.dim() - 2))
    ce = -(w * t * m * lp).sum() / (x.numel() // K)
    return ce_weight * ce + dice_weight * dice


def dice_loop(x, target, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5):
    """The same loss by plain Python loops over entries and classes (float arithmetic on flattened tensors)."""
    N, K = x.shape[:2]
    p = torch.softmax(x, 1).reshape(N, K, -1)
    labels = target.dim() == x.dim() - 1
    tgt = target.reshape(N, -1) if labels else target.reshape(N, K, -1)
    w = [1.0] * K if weight is None else [float(a) for a in torch.as_tensor(weight).reshape(-1)]
    first = 1 if ignore_background else 0
    wsum = sum(w[first:])
    rows = [list(range(N))] if batch_dice else [[n] for n in range(N)]
    total = 0.0
    for row in rows:
        for k in range(first, K):
            I = P = T = 0.0
            for n in row:
                if labels:
                    keep = tgt[n] != -100
                    tk = (tgt[n] == k).to(x.dtype)[keep]
                    pk = p[n, k][keep]
                else:
                    tk, pk = tgt[n, k], p[n, k]
                I += float((pk * tk).sum())
                P += float(pk.sum())
                T += float(tk.sum())
            total += w[k] / wsum * (2.0 * I + smooth) / (P + T + smooth)
    return 1.0 - total / len(rows)
