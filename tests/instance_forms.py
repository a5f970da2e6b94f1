"""Brute-force form of common.metrics.instance_metrics, written from its definitions in plain numpy with Python integers on the CPU
(tests only), and the label pairs of tests/test_instances_gpu.py.

    components:  those of components_forms (connected_components with num_classes = K); the class of one is its voxels' label
    pair:        a component a of pred and b of target of the same entry and class; I = |a n b|, U = |a| + |b| - I
    overlap:     I >= 1
    match:       float(I) > iou_threshold * float(U)
    iou_fixed:   the sum over the matches of (I << 32) // U

One entry at a time: the roots of both maps, then numpy.unique over the (root in pred, root in target) of the voxels that carry
the same label and a root in both maps lists every overlapping pair with its I."""
import collections
import itertools

import numpy as np
import torch

from tests.components_forms import _roots_of_entry

InstanceBrute = collections.namedtuple("InstanceBrute", ["components", "matched", "overlapping", "iou_fixed", "precision", "recall",
                                                         "f1", "sq", "pq", "pred_status", "target_status", "pairs", "half_pairs",
                                                         "most_partners"])
INTEGERS = ("components", "matched", "overlapping", "iou_fixed")
QUOTIENTS = ("precision", "recall", "f1", "sq", "pq")


def roots_of(labels, connectivity, background, num_classes):
    """(N, dims) int64 numpy: the root of every voxel (the smallest linear index of its component within the entry), -1 elsewhere."""
    x = torch.as_tensor(labels).cpu().numpy()
    return np.stack([_roots_of_entry(x[n], connectivity, background, num_classes) for n in range(x.shape[0])])


def _quotient(num, den):
    return np.float32(float(num) / float(den)) if den else np.float32("nan")


def instance_brute(pred, target, num_classes, iou_threshold=0.5, connectivity=1, background=0, roots=None):
    """InstanceBrute of numpy arrays.  Beyond the fields of InstanceMetrics: `pairs` (N, K), the overlapping pairs; `half_pairs`
    (N, K), those with 2 I == U; `most_partners`, the largest number of matches any single component has (at most 1 by the
    definitions).  `roots`: (roots_of(pred, ...), roots_of(target, ...)) if already there."""
    p = torch.as_tensor(pred).cpu().numpy()
    t = torch.as_tensor(target).cpu().numpy()
    K, N = int(num_classes), p.shape[0]
    rp_all, rt_all = roots if roots is not None else (roots_of(p, connectivity, background, K), roots_of(t, connectivity, background, K))
    ints = {name: np.zeros((N, K, 2) if name in ("components", "overlapping") else (N, K), dtype=np.int64) for name in INTEGERS}
    pairs = np.zeros((N, K), dtype=np.int64)
    half_pairs = np.zeros((N, K), dtype=np.int64)
    status = [np.zeros(p.shape, dtype=np.uint8), np.zeros(p.shape, dtype=np.uint8)]
    iou_fixed = [[0] * K for _ in range(N)]                                   # Python integers
    most_partners = 0
    for n in range(N):
        rp, rt = rp_all[n].reshape(-1), rt_all[n].reshape(-1)
        lp, lt = p[n].reshape(-1), t[n].reshape(-1)
        size_p = np.bincount(rp[rp >= 0], minlength=rp.size)
        size_t = np.bincount(rt[rt >= 0], minlength=rt.size)
        for which, (r, lab) in enumerate(((rp, lp), (rt, lt))):
            for root in np.unique(r[r >= 0]).tolist():
                ints["components"][n, lab[root], which] += 1
        both = (rp >= 0) & (rt >= 0) & (lp == lt)
        state = [dict(), dict()]                                               # root -> [overlaps, matches]
        if both.any():
            keys, counts = np.unique(np.stack([rp[both], rt[both]], axis=1), axis=0, return_counts=True)
            for (a, b), I in zip(keys.tolist(), counts.tolist()):
                k = int(lp[a])
                assert k == int(lt[b]) and 0 <= k < K and k != background
                U = int(size_p[a]) + int(size_t[b]) - I
                match = float(I) > iou_threshold * float(U)
                pairs[n, k] += 1
                half_pairs[n, k] += 2 * I == U
                for which, root in ((0, a), (1, b)):
                    s = state[which].setdefault(root, [0, 0])
                    if s[0] == 0:
                        ints["overlapping"][n, k, which] += 1
                    s[0] += 1
                    s[1] += match
                if match:
                    ints["matched"][n, k] += 1
                    iou_fixed[n][k] += (I << 32) // U
        for which, r in enumerate((rp, rt)):
            flat = status[which][n].reshape(-1)
            flat[r >= 0] = 3
            for root, (overlaps, matches) in state[which].items():
                most_partners = max(most_partners, matches)
                flat[r == root] = 1 if matches else 2
    ints["iou_fixed"] = np.array(iou_fixed, dtype=np.int64)
    q = {name: np.zeros((N, K), dtype=np.float32) for name in QUOTIENTS}
    for n, k in itertools.product(range(N), range(K)):
        nP, nT = (int(c) for c in ints["components"][n, k])
        TP = int(ints["matched"][n, k])
        S = float(iou_fixed[n][k]) * 2.0 ** -32
        q["precision"][n, k] = _quotient(TP, nP)
        q["recall"][n, k] = _quotient(TP, nT)
        q["f1"][n, k] = _quotient(2 * TP, nP + nT)
        q["sq"][n, k] = _quotient(S, TP)
        q["pq"][n, k] = _quotient(2.0 * S, nP + nT)
    return InstanceBrute(*([ints[name] for name in INTEGERS] + [q[name] for name in QUOTIENTS] + status
                           + [pairs, half_pairs, most_partners]))


# ---- the label pairs of tests/test_instances_gpu.py --------------------------------------------------------------------------

CELL = 8


def _cells(dims):
    """The cells of CELL voxels per axis (the last one of an axis may be shorter; an axis below CELL is one cell)."""
    per_axis = [[(o, min(CELL, s - o)) for o in range(0, s, CELL)] for s in dims]
    return itertools.product(*per_axis)


def _fill(m, lo, size, value):
    at = tuple(slice(max(0, a), max(0, min(a + s, d))) for a, s, d in zip(lo, size, m.shape))
    m[at] = value


def lesion_pairs(shape, K, seed):
    """(pred, target) int64 (N, dims) of the classes 1 .. K-1 on background 0.  Every cell draws one of: nothing (2 in 10); a box
    of 1-4 voxels per axis in target and the box shifted by -1..1 and resized by -1..1 per axis in pred, in one case in ten with
    another class in pred (5 in 10); a box in one map only (1 in 10); a split (2 in 10): a box 5 long on the last axis in one
    map and the same box with its fourth plane cleared in the other, so one component overlaps a piece of 3 (IoU 0.6) and a piece
    of 1.  On top, 1 % of the voxels of each map are -100 and one voxel is K + 3."""
    rng = np.random.RandomState(seed)
    pred = np.zeros(shape, dtype=np.int64)
    target = np.zeros(shape, dtype=np.int64)
    for n in range(shape[0]):
        for cell in _cells(shape[1:]):
            origin, extent = [c[0] for c in cell], [c[1] for c in cell]
            kind = rng.randint(10)
            k = 1 + rng.randint(max(K - 1, 1))
            size = [min(1 + rng.randint(4), max(1, e - 2)) for e in extent]
            lo = [o + (1 + rng.randint(e - s - 1) if e - s - 1 >= 1 else 0) for o, e, s in zip(origin, extent, size)]
            shift = [rng.randint(-1, 2) for _ in extent]
            resize = [rng.randint(-1, 2) for _ in extent]
            wrong = rng.randint(10) == 0
            first = rng.randint(2)
            maps = (pred[n], target[n]) if first else (target[n], pred[n])
            if kind < 2:
                continue
            if kind >= 8 and extent[-1] >= 5:                                   # split
                size[-1] = 5
                size[:-1] = [min(s, 2) for s in size[:-1]]
                lo[-1] = origin[-1] + rng.randint(extent[-1] - 5 + 1)
                _fill(maps[0], lo, size, k)
                _fill(maps[1], lo, size, k)
                _fill(maps[1], lo[:-1] + [lo[-1] + 3], size[:-1] + [1], 0)
            elif kind == 7:                                                     # one map only
                _fill(maps[0], lo, size, k)
            else:                                                               # a box and its shifted, resized copy
                _fill(target[n], lo, size, k)
                other = k if not wrong or K < 3 else 1 + (k % (K - 1))
                _fill(pred[n], [a + d for a, d in zip(lo, shift)], [max(1, s + d) for s, d in zip(size, resize)], other)
    for m in (pred, target):
        m[rng.rand(*shape) < 0.01] = -100
        m.reshape(-1)[rng.randint(m.size)] = K + 3
    return torch.from_numpy(pred), torch.from_numpy(target)


def flipped(x, share, seed):
    """x (values in {0, 1}) with `share` of its voxels flipped."""
    g = torch.Generator().manual_seed(seed)
    flip = torch.rand(x.shape, generator=g) < share
    return torch.where(flip, 1 - x, x)


def alternating(shape):
    """Classes 1 and 2 alternating along every axis: at connectivity 1 every voxel is a component of its own."""
    grids = torch.meshgrid(*[torch.arange(s) for s in shape[1:]], indexing="ij")
    return (1 + sum(grids) % 2).long().unsqueeze(0).repeat(shape[0], *([1] * (len(shape) - 1))).contiguous()
