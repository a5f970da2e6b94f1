"""Brute-force surface distance metrics of common.metrics (surface_distance_metrics, hausdorff_distance, average_surface_distance),
written from their definitions in plain torch / numpy on the CPU (tests only).

    A = {v: pred[n,v] == k}, B = {v: target[n,v] == k};  a label outside [0, K) belongs to no class
    dS = the voxels of S with a face neighbour outside S (a position outside the image is outside S): a padded-neighbour test
    direction 0 = {min_{b in dB} |S (a - b)| : a in dA},  direction 1 = {min_{a in dA} |S (b - a)| : b in dB}: all pairs between
                  the two border sets only, int64 squares with unit spacing, float64 with a sampling
    per direction max, mean and numpy.percentile(., q) (the default "linear" rule)
    hausdorff = max of the maxima, hausdorff_percentile = max of the percentiles, assd = (sum0 + sum1) / (m0 + m1)
    both borders empty: NaN;  one empty: +inf;  dice = 2 |A n B| / (|A| + |B|), NaN when both are empty."""
import collections

import numpy as np
import torch

FIELDS = ["hausdorff", "hausdorff_percentile", "assd", "directed", "surface_voxels", "max_squared", "overlap", "dice"]
Reference = collections.namedtuple("Reference", FIELDS)


def border(member):
    """bool (dims) -> bool (dims): the members with a face neighbour that is no member or outside the image."""
    nd = member.dim()
    padded = torch.zeros([s + 2 for s in member.shape], dtype=torch.bool)
    inner = tuple(slice(1, -1) for _ in range(nd))
    padded[inner] = member
    surrounded = torch.ones_like(member)
    for a in range(nd):
        for shift in (0, 2):
            at = tuple(slice(shift, shift + member.shape[b]) if b == a else slice(1, -1) for b in range(nd))
            surrounded &= padded[at]
    return member & ~surrounded


def _nearest(a, b, sampling):
    """Per row of a (m, nd) int64 the squared distance to the nearest row of b: int64 (unit spacing) or float64."""
    out = []
    s = None if sampling is None else torch.tensor([float(v) for v in sampling], dtype=torch.float64)
    for i0 in range(0, a.shape[0], 512):
        delta = a[i0:i0 + 512, None, :] - b[None, :, :]
        if s is None:
            out.append((delta * delta).sum(-1).min(1).values)
        else:
            sd = delta.double() * s
            out.append((sd * sd).sum(-1).min(1).values)
    return torch.cat(out)


def directed_squares(pred, target, K, sampling=None):
    """{(n, k): (squares of direction 0, squares of direction 1, |A|, |B|, |A n B|)}; squares are None where the OTHER border is
    empty and of length 0 where the own border is."""
    pred, target = torch.as_tensor(pred).cpu(), torch.as_tensor(target).cpu()
    out = {}
    for n in range(pred.shape[0]):
        for k in range(K):
            A, B = pred[n] == k, target[n] == k
            a, b = torch.nonzero(border(A)), torch.nonzero(border(B))
            d0 = _nearest(a, b, sampling) if b.shape[0] and a.shape[0] else (None if a.shape[0] else torch.zeros(0))
            d1 = _nearest(b, a, sampling) if b.shape[0] and a.shape[0] else (None if b.shape[0] else torch.zeros(0))
            out[(n, k)] = (d0, d1, a.shape[0], b.shape[0], int(A.sum()), int(B.sum()), int((A & B).sum()))
    return out


def metrics_of(squares, N, K, q):
    """The float64 / int64 Reference from directed_squares()."""
    r = Reference(torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, K, dtype=torch.float64), torch.zeros(N, K, dtype=torch.float64),
                  torch.zeros(N, K, 2, 3, dtype=torch.float64), torch.zeros(N, K, 2, dtype=torch.int64),
                  torch.zeros(N, K, 2, dtype=torch.float64), torch.zeros(N, K, 3, dtype=torch.int64),
                  torch.zeros(N, K, dtype=torch.float64))
    for (n, k), (d0, d1, m0, m1, a, b, ab) in squares.items():
        r.surface_voxels[n, k] = torch.tensor([m0, m1])
        r.overlap[n, k] = torch.tensor([a, b, ab])
        r.dice[n, k] = 2.0 * ab / (a + b) if a + b else float("nan")
        if m0 == 0 or m1 == 0:
            fill = float("nan") if m0 == 0 and m1 == 0 else float("inf")
            for f in (r.hausdorff, r.hausdorff_percentile, r.assd, r.directed, r.max_squared):
                f[n, k] = fill
            continue
        total = 0.0
        for d, sq in enumerate((d0, d1)):
            dist = sq.double().sqrt().numpy()
            r.max_squared[n, k, d] = float(sq.max())
            r.directed[n, k, d] = torch.tensor([float(dist.max()), float(np.percentile(dist, q)), float(dist.mean())], dtype=torch.float64)
            total += float(dist.sum())
        r.hausdorff[n, k] = r.directed[n, k, :, 0].max()
        r.hausdorff_percentile[n, k] = r.directed[n, k, :, 1].max()
        r.assd[n, k] = total / (m0 + m1)
    return r


def surface_brute(pred, target, K, sampling=None, q=95.0):
    pred = torch.as_tensor(pred)
    return metrics_of(directed_squares(pred, target, K, sampling), pred.shape[0], K, q)


# ---- the cases of tests/test_surface_gpu.py ------------------------------------------------------------------------------------

# (K, (N, dims)): the smallest shapes at which each pass can go wrong
CASES = [(1, (2, 5, 7)),               # smaller than a wave
         (4, (3, 36, 57)),             # tails in both axes
         (20, (1, 70, 130)),           # rows longer than a wave
         (2, (1, 600, 9)),             # a column longer than an LDS tile; squared distances above 2^16: the third radix digit
         (4, (2, 6, 10, 70)),          # 3D
         (70, (1, 33, 9, 5)),          # the longest axis outermost; more classes than one histogram group
         (300, (1, 12, 70))]           # more classes than one group of counters and of fp64 accumulators
FAR_SHAPE = (1, 4200, 4)               # squared distances above 2^24: the fourth digit, and inexact in an fp32 copy
PERCENTILES = [0.0, 37.5, 50.0, 95.0, 100.0]


def case_id(case):
    return "K%d-%s" % (case[0], "x".join(map(str, case[1])))


def label_pair(K, shape, seed=0):
    """(pred, target) int64 (N, dims).  target: random blocks (4 voxels wide) of the classes 0 .. K-2 (from 3 classes on; both
    classes for K == 2; class 0 and no class for K == 1), 5 % of the voxels at -100 and one at K + 3.  pred: target rolled by a few
    voxels, 1 % of the voxels relabelled at random (far outliers), other voxels at -100 and another at K + 3.  From 4 classes on
    class K-1 is absent from both maps and class K-2 from pred only."""
    g = torch.Generator().manual_seed(seed)
    used = K if K <= 2 else K - 1
    y = torch.randint(0, max(used, 2), (shape[0],) + tuple((s + 3) // 4 for s in shape[1:]), generator=g)
    for a in range(1, len(shape)):
        y = y.repeat_interleave(4, dim=a).narrow(a, 0, shape[a])
    y = y.contiguous()
    if K == 1:
        y[y == 1] = -100
    if K >= 4:
        y[(-1,) + (slice(-4, None),) * (len(shape) - 1)] = K - 2            # (whatever the blocks drew, class K-2 is in target)
    p = torch.roll(y, shifts=tuple([1, 2, 1][:len(shape) - 1]), dims=tuple(range(1, len(shape))))
    noise = torch.rand(shape, generator=g) < 0.01
    p[noise] = torch.randint(0, used, (int(noise.sum()),), generator=g)
    if K >= 4:
        p[p == K - 2] = 0
    y[torch.rand(shape, generator=g) < 0.05] = -100
    p[torch.rand(shape, generator=g) < 0.05] = -100
    y.reshape(shape[0], -1)[0, 5] = K + 3
    p.reshape(shape[0], -1)[0, 3] = K + 3
    return p, y


def column_pair():
    """label_pair(2, (1, 600, 9)) with class 1 confined to the upper half of both maps, but for one voxel of pred near the bottom:
    squared distances above 2^16."""
    p, y = label_pair(2, (1, 600, 9), seed=2)
    p[0, 300:][p[0, 300:] == 1] = 0
    y[0, 300:][y[0, 300:] == 1] = 0
    p[0, 590, 4] = 1
    return p, y


def pair_of(K, shape):
    """The label maps of a case of CASES, or of (2, FAR_SHAPE)."""
    if shape == FAR_SHAPE:
        return far_pair()
    if shape == (1, 600, 9):
        return column_pair()
    return label_pair(K, shape, seed=K)


def far_pair():
    """FAR_SHAPE, K = 2, every voxel without a class but a few: class 0 is a blob at the top of target and at the bottom of pred
    (distances of about 4190: squares above 2^24), class 1 two blobs near the top, one row apart."""
    p = torch.full(FAR_SHAPE, -100, dtype=torch.int64)
    y = torch.full(FAR_SHAPE, -100, dtype=torch.int64)
    y[0, 1:3, 1:3] = 0
    p[0, 4195:4198, 1:3] = 0
    y[0, 10, 0:3] = 1
    p[0, 11, 1:4] = 1
    return p, y


def speck_pair(shape):
    """K = 2 on (1, H, W): class 1 is a blob near the top of both maps, and in pred one more voxel near the bottom; every other
    voxel has no class.  The borders of class 1 coincide except for that speck: direction 0 is m - 1 zeros and one far distance."""
    H, W = shape[1:]
    y = torch.full(shape, -100, dtype=torch.int64)
    y[0, 2:5, 0:min(3, W)] = 1
    p = y.clone()
    p[0, H - 2, min(2, W - 1)] = 1
    return p, y
