"""Reference forms of common.metrics.confusion_matrix / overlap_metrics / overlap_scores in numpy, and the label maps and logits of
tests/test_confusion_cpu.py and tests/test_confusion_gpu.py.

The counts are np.add.at on a (K + 1, K + 1) table, labels outside [0, K) mapped to the extra index K, ignore_index applied first
(on the target only).  The scores are float64 quotients of the integers cast to fp32 once.  The argmax is torch.argmax on the CPU
tensor (for bf16: on the CPU bf16 tensor itself)."""
import collections

import numpy as np
import torch

from tests.surface_forms import label_pair

ConfusionForm = collections.namedtuple("ConfusionForm", ["matrix", "pred_only", "target_only", "counted"])
OverlapForm = collections.namedtuple("OverlapForm", ["overlap", "counted", "dice", "iou", "precision", "recall", "specificity"])
SCORES = ["dice", "iou", "precision", "recall", "specificity"]


def table_form(pred, target, K, ignore_index=None):
    """pred, target (N, dims) int64 -> ((N, K + 1, K + 1) int64 table [n, t, p] with index K for "no class", counted (N,))."""
    p = torch.as_tensor(pred).cpu().numpy().reshape(pred.shape[0], -1)
    y = torch.as_tensor(target).cpu().numpy().reshape(target.shape[0], -1)
    N = p.shape[0]
    table = np.zeros((N, K + 1, K + 1), dtype=np.int64)
    counted = np.zeros((N,), dtype=np.int64)
    for n in range(N):
        keep = np.ones(y[n].shape, dtype=bool) if ignore_index is None else y[n] != ignore_index
        pn, yn = p[n][keep], y[n][keep]
        pi = np.where((pn >= 0) & (pn < K), pn, K)
        yi = np.where((yn >= 0) & (yn < K), yn, K)
        np.add.at(table[n], (yi, pi), 1)
        counted[n] = keep.sum()
    return table, counted


def confusion_form(pred, target, K, ignore_index=None, reduce_batch=False):
    table, counted = table_form(pred, target, K, ignore_index)
    if reduce_batch:
        table, counted = table.sum(0), counted.sum(0)
    return ConfusionForm(torch.from_numpy(np.ascontiguousarray(table[..., :K, :K])),
                         torch.from_numpy(np.ascontiguousarray(table[..., K, :K])),
                         torch.from_numpy(np.ascontiguousarray(table[..., :K, K])), torch.as_tensor(counted))


def _quotient(num, den):
    num, den = num.astype(np.float64), den.astype(np.float64)
    out = np.full(num.shape, np.nan, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return torch.from_numpy(out.astype(np.float32))


def scores_form(overlap, counted):
    """overlap (..., K, 3), counted (...) int64 torch -> the five fp32 scores (..., K) in the order of SCORES."""
    o, c = overlap.numpy(), counted.numpy()
    a, b, tp = o[..., 0], o[..., 1], o[..., 2]
    fp, fn = a - tp, b - tp
    tn = c[..., None] - tp - fp - fn
    return [_quotient(2 * tp, a + b), _quotient(tp, a + b - tp), _quotient(tp, a), _quotient(tp, b), _quotient(tn, tn + fp)]


def overlap_form(pred, target, K, ignore_index=None, reduce_batch=False):
    """Without the table (K may be large): |A|, |B|, |A n B| as bincounts of the counted in-range labels."""
    p = torch.as_tensor(pred).cpu().numpy().reshape(pred.shape[0], -1)
    y = torch.as_tensor(target).cpu().numpy().reshape(target.shape[0], -1)
    N = p.shape[0]
    overlap = np.zeros((N, K, 3), dtype=np.int64)
    counted = np.zeros((N,), dtype=np.int64)
    for n in range(N):
        keep = np.ones(y[n].shape, dtype=bool) if ignore_index is None else y[n] != ignore_index
        in_p, in_y = keep & (p[n] >= 0) & (p[n] < K), keep & (y[n] >= 0) & (y[n] < K)
        overlap[n, :, 0] = np.bincount(p[n][in_p], minlength=K)
        overlap[n, :, 1] = np.bincount(y[n][in_y], minlength=K)
        overlap[n, :, 2] = np.bincount(p[n][in_p & in_y & (p[n] == y[n])], minlength=K)
        counted[n] = keep.sum()
    if reduce_batch:
        overlap, counted = overlap.sum(0), counted.sum(0)
    overlap, counted = torch.from_numpy(overlap), torch.as_tensor(counted)
    return OverlapForm(overlap, counted, *scores_form(overlap, counted))


def argmax_form(logits):
    """torch.argmax over the class axis of the CPU tensor, in its own dtype."""
    return torch.argmax(logits.detach().cpu(), dim=1)


# ---- label maps ---------------------------------------------------------------------------------------------------------------

def blobs(K, shape, seed=0):
    """Classes 1 .. K - 1 (class 0 alone for K == 1) as balls around 16 seeded centres per entry on background 0; a voxel takes
    the class of the nearest centre that covers it.  Integer arithmetic on torch's seeded CPU generator."""
    g = torch.Generator().manual_seed(77 * K + seed)
    dims = shape[1:]
    grids = torch.meshgrid(*[torch.arange(s) for s in dims], indexing="ij")
    out = torch.zeros(shape, dtype=torch.int64)
    widest = max(2, max(dims) // 6)
    for n in range(shape[0]):
        centres = [torch.randint(0, s, (16,), generator=g) for s in dims]
        radius = torch.randint(1, widest + 1, (16,), generator=g)
        cls = torch.randint(1, K, (16,), generator=g) if K > 1 else torch.zeros(16, dtype=torch.int64)
        view = (16,) + (1,) * len(dims)
        d2 = sum((gr.unsqueeze(0) - c.view(view)) ** 2 for gr, c in zip(grids, centres))
        d2 = torch.where(d2 <= (radius ** 2).view(view), d2, torch.full_like(d2, 2 ** 40))
        best, who = d2.min(0)
        out[n] = torch.where(best < 2 ** 40, cls[who], torch.zeros_like(who))
    return out


def label_patterns(K, shape, seed=0):
    """{name: (pred, target)} int64 (N, dims): the patterns of tests/test_confusion_gpu.py."""
    g = torch.Generator().manual_seed(1234 + seed)
    one = torch.full(shape, K - 1, dtype=torch.int64)
    bp, bt = label_pair(K, shape, seed=K)                 # both with 5 % at -100 and one voxel at K + 3
    clean_t = blobs(K, shape, seed)
    clean_p = torch.roll(clean_t, 1, dims=-1)
    return {
        "one_class": (one, one.clone()),
        "uniform": (torch.randint(0, K, shape, generator=g), torch.randint(0, K, shape, generator=g)),
        "blobs": (clean_p, clean_t),
        "blocks_pred": (bp, clean_t),
        "blocks_target": (clean_p, bt),
        "blocks_both": (bp, bt),
        "all_ignored": (clean_p, torch.full(shape, -100, dtype=torch.int64)),
    }


# ---- logits -------------------------------------------------------------------------------------------------------------------

def logits_patterns(K, shape, dtype, seed=0):
    """{name: logits (N, K, dims) of `dtype` on the CPU}.  gaussian; half_integers: multiples of 0.5 in [-1.5, 1.5], exact in bf16,
    so that most voxels tie; specials: gaussian with NaN, +inf, -inf planted and one voxel of all -inf."""
    g = torch.Generator().manual_seed(4321 + seed + 17 * K)
    full = (shape[0], K) + tuple(shape[1:])
    gauss = torch.randn(full, generator=g)
    half = torch.randint(-3, 4, full, generator=g).float() * 0.5
    special = torch.randn(full, generator=g)
    flat = special.view(shape[0], K, -1)
    V = flat.shape[2]
    for i, value in enumerate([float("nan"), float("inf"), -float("inf"), float("nan"), float("inf")]):
        idx = torch.randint(0, V, (max(1, V // 16),), generator=g)
        cls = torch.randint(0, K, idx.shape, generator=g)
        flat[i % shape[0], cls, idx] = value
    flat[0, :, V // 2] = -float("inf")                    # an all -inf voxel: class 0
    flat[-1, :, V - 1] = float("nan")                     # all NaN: the first one, class 0
    if K > 1:
        flat[0, K - 1, 0] = float("nan")                  # a NaN behind a +inf: the NaN wins
        flat[0, 0, 0] = float("inf")
    return {"gaussian": gauss.to(dtype), "half_integers": half.to(dtype), "specials": special.to(dtype)}
