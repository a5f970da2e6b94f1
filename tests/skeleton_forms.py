"""The definitions behind common.loss.soft_skeletonize / cldice_loss, in any dtype on any device torch runs (tests only).

Stacked forms: E (minimum over a voxel and its in-image face neighbours) and D (maximum over the in-image 3x3(x3) box) as
torch.min / torch.max over dim 0 of a stack of shifted copies padded with +inf / -inf.  Both return the FIRST extremum of the
stack, so autograd realises the tie rule of the kernels: centre, then axis by axis, minus before plus (E); centre, then raster
order of the box (D).  relu'(0) = 0 is torch's own.

Published forms: the max_pool composition of Shit et al. (clDice, CVPR 2021): soft_erode / soft_dilate / soft_skel / soft_cldice.
"""
import itertools

import torch
import torch.nn.functional as F


def _shifted(x, offset, fill):
    """y(v) = x(v + offset) where that is inside the image, `fill` elsewhere; x is (N,C,dims)."""
    nd = x.dim() - 2
    pad = []
    for _ in range(nd):
        pad += [1, 1]
    xp = F.pad(x, pad, value=fill)
    index = [slice(None), slice(None)] + [slice(1 + o, 1 + o + s) for o, s in zip(offset, x.shape[2:])]
    return xp[tuple(index)]


def cross_offsets(nd):
    offs = [(0,) * nd]
    for a in range(nd):
        for s in (-1, 1):
            offs.append(tuple(s if i == a else 0 for i in range(nd)))
    return offs


def box_offsets(nd):
    return [(0,) * nd] + list(itertools.product((-1, 0, 1), repeat=nd))


def erode_stack(x):
    return torch.stack([_shifted(x, o, float("inf")) for o in cross_offsets(x.dim() - 2)])


def dilate_stack(x):
    return torch.stack([_shifted(x, o, float("-inf")) for o in box_offsets(x.dim() - 2)])


def erode(x):
    return erode_stack(x).min(dim=0).values


def dilate(x):
    return dilate_stack(x).max(dim=0).values


def soft_skeleton_stacked(x, iterations):
    skel = torch.relu(x - dilate(erode(x)))
    for _ in range(iterations):
        x = erode(x)
        delta = torch.relu(x - dilate(erode(x)))
        skel = skel + torch.relu(delta - skel * delta)
    return skel


# ---- the published composition ---------------------------------------------------------------------------------------------
def soft_erode(img):
    if img.dim() == 4:
        p1 = -F.max_pool2d(-img, (3, 1), (1, 1), (1, 0))
        p2 = -F.max_pool2d(-img, (1, 3), (1, 1), (0, 1))
        return torch.min(p1, p2)
    p1 = -F.max_pool3d(-img, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    p2 = -F.max_pool3d(-img, (1, 3, 1), (1, 1, 1), (0, 1, 0))
    p3 = -F.max_pool3d(-img, (1, 1, 3), (1, 1, 1), (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def soft_dilate(img):
    if img.dim() == 4:
        return F.max_pool2d(img, (3, 3), (1, 1), (1, 1))
    return F.max_pool3d(img, (3, 3, 3), (1, 1, 1), (1, 1, 1))


def soft_open(img):
    return soft_dilate(soft_erode(img))


def soft_skel(img, iter_):
    img1 = soft_open(img)
    skel = F.relu(img - img1)
    for _ in range(iter_):
        img = soft_erode(img)
        img1 = soft_open(img)
        delta = F.relu(img - img1)
        skel = skel + F.relu(delta - skel * delta)
    return skel


def soft_cldice_published(y_true, y_pred, iter_=3, smooth=1.0):
    """y_true, y_pred: (N,K,dims) one-hot / probabilities; the foreground channels pooled over batch and classes."""
    skel_pred = soft_skel(y_pred, iter_)
    skel_true = soft_skel(y_true, iter_)
    tprec = (torch.sum(torch.multiply(skel_pred, y_true)[:, 1:, ...]) + smooth) / (torch.sum(skel_pred[:, 1:, ...]) + smooth)
    tsens = (torch.sum(torch.multiply(skel_true, y_pred)[:, 1:, ...]) + smooth) / (torch.sum(skel_true[:, 1:, ...]) + smooth)
    return 1.0 - 2.0 * (tprec * tsens) / (tprec + tsens)


# ---- the loss as common.loss.cldice_loss defines it ---------------------------------------------------------------------
def one_hot_no_class(labels, K, dtype):
    """(N,dims) int64 -> (N,K,dims); a label outside [0, K) is in no class."""
    return torch.stack([(labels == k) for k in range(K)], dim=1).to(dtype)


def cldice_closed(logits, target, iterations=3, weight=None, ignore_background=True, batch=False, smooth=1.0):
    p = torch.softmax(logits, 1)
    N, K = p.shape[:2]
    if target.dim() == logits.dim() - 1:
        t = one_hot_no_class(target, K, p.dtype)
        m = (target != -100).to(p.dtype).unsqueeze(1)
    else:
        t = target.detach().to(p.dtype)
        m = torch.ones_like(p[:, :1])
    sp = soft_skeleton_stacked(p, iterations)
    st = soft_skeleton_stacked(t, iterations)
    axes = tuple(range(2, p.dim()))
    sums = [(m * sp * t).sum(axes), (m * sp).sum(axes), (m * st * p).sum(axes), (m * st).sum(axes)]      # (N,K) each
    if batch:
        sums = [s.sum(0, keepdim=True) for s in sums]
    tprec = (sums[0] + smooth) / (sums[1] + smooth)
    tsens = (sums[2] + smooth) / (sums[3] + smooth)
    cl = 2 * tprec * tsens / (tprec + tsens)
    w = torch.ones(K, dtype=p.dtype, device=p.device) if weight is None else torch.as_tensor(weight, dtype=p.dtype, device=p.device)
    first = 1 if ignore_background else 0
    omega = w[first:] / w[first:].sum()
    return 1 - (cl[:, first:] * omega).sum() / cl.shape[0]


# ---- how far the selections of a map are from flipping -------------------------------------------------------------------
def _nonzero_min(a):
    a = a[torch.isfinite(a) & (a != 0)]
    return float(a.abs().min()) if a.numel() else float("inf")


def selection_margin(p, iterations):
    """Over all levels of the skeleton of p: the smaller of the smallest nonzero gap between a window's extremum and any other
    value of the window, and the smallest nonzero |relu argument|."""
    margin = float("inf")

    def opened(x):
        nonlocal margin
        es = erode_stack(x)
        e = es.min(dim=0).values
        margin = min(margin, _nonzero_min(es - e))
        ds = dilate_stack(e)
        o = ds.max(dim=0).values
        margin = min(margin, _nonzero_min(o - ds))
        return e, o

    x = p
    e, o = opened(x)
    margin = min(margin, _nonzero_min(x - o))
    skel = torch.relu(x - o)
    for _ in range(iterations):
        x = e
        e, o = opened(x)
        margin = min(margin, _nonzero_min(x - o))
        delta = torch.relu(x - o)
        arg = delta - skel * delta
        margin = min(margin, _nonzero_min(arg))
        skel = skel + torch.relu(arg)
    return margin


def margin_logits(shape, seed):
    """float64 logits log(q) whose softmax has well separated values: each foreground plane of q is a random permutation of
    (i + 0.5) / V * 0.9 / (K - 1), q_0 the rest."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    N, K = shape[:2]
    V = 1
    for s in shape[2:]:
        V *= s
    q = torch.empty((N, K, V), dtype=torch.float64)
    base = (torch.arange(V, dtype=torch.float64) + 0.5) / V * 0.9 / (K - 1)
    for n in range(N):
        for k in range(1, K):
            q[n, k] = base[torch.randperm(V, generator=g)]
    q[:, 0] = 1 - q[:, 1:].sum(1)
    return torch.log(q).reshape(shape)
