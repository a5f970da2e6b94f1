"""Brute-force forms of common.postprocess.erosion / dilation / opening / closing, written from their definitions in plain numpy
(tests only; no scipy, no distance transform), and the label maps of tests/test_morph_gpu.py.

    ball       B = {o : sum_a (s_a o_a)^2 <= radius^2}; with unit spacing the integer test |o|^2 <= floor(radius^2)
    border     a position outside the image is nothing: no member of any class (dilation), no obstacle (erosion)
    class voxel  a label k in [0, K) other than `background`; labels outside [0, K) are copied and count as "another label"

Every function enumerates the offsets of the ball and shifts whole arrays by them: O(|B|) array operations, nothing cleverer."""
import itertools
import math

import numpy as np
import torch


def ball_offsets(radius, shape, sampling=None):
    """[(offset tuple, squared length)] of the ball, restricted to the offsets that can connect two voxels of `shape` (dims)."""
    nd = len(shape)
    if sampling is None:
        r2 = float(radius) * float(radius)
        r2 = 2 ** 30 - 1 if r2 >= 2 ** 30 - 1 else math.floor(r2)
        s = (1,) * nd
    else:
        r2 = float(radius) * float(radius)
        s = tuple(float(v) for v in sampling)
    reach = [min(int(math.floor(min(float(radius), 1e9) / s[a])) + 1, shape[a] - 1) for a in range(nd)]
    out = []
    for o in itertools.product(*[range(-m, m + 1) for m in reach]):
        d2 = sum((s[a] * o[a]) ** 2 for a in range(nd))
        if d2 <= r2:
            out.append((o, d2))
    return out


def smallest_relative_gap(radius, shape, sampling):
    """min |d2 - radius^2| / radius^2 over ALL offsets that fit in `shape`: how far the ball's membership is from a flip."""
    r2 = float(radius) ** 2
    gaps = [abs(sum((float(sampling[a]) * o[a]) ** 2 for a in range(len(shape))) - r2) / r2
            for o in itertools.product(*[range(0, m) for m in shape])]
    return min(gaps)


def _windows(shape, o):
    """(here, there): slices with x[there] = the voxels at v + o for the v of x[here] that have v + o inside the image."""
    here = tuple(slice(max(0, -c), shape[a] - max(0, c)) for a, c in enumerate(o))
    there = tuple(slice(max(0, c), shape[a] - max(0, -c)) for a, c in enumerate(o))
    return here, there


def _set_erosion(member, offsets):
    """{v in member : every in-image v + o is in member}"""
    keep = member.copy()
    for o, _ in offsets:
        here, there = _windows(member.shape, o)
        keep[here] &= member[there]
    return keep


def _set_dilation(member, offsets):
    """{v in the image : some v + o is in member} (the ball is symmetric)"""
    out = np.zeros_like(member)
    for o, _ in offsets:
        here, there = _windows(member.shape, o)
        out[here] |= member[there]
    return out


def _classes(K, background):
    return [k for k in range(K) if k != background]


def _per_entry(fn, labels):
    x = torch.as_tensor(labels).cpu().numpy()
    return torch.from_numpy(np.stack([fn(e) for e in x]))


def erosion_brute(labels, radius, K, sampling=None, background=0):
    def one(x):
        offsets = ball_offsets(radius, x.shape, sampling)
        same = np.ones(x.shape, dtype=bool)                     # every in-image v + o carries labels[v]
        for o, _ in offsets:
            here, there = _windows(x.shape, o)
            same[here] &= x[here] == x[there]
        is_class = (x >= 0) & (x < K) & (x != background)
        out = x.copy()
        out[is_class & ~same] = background
        return out
    return _per_entry(one, labels)


def dilation_brute(labels, radius, K, sampling=None, background=0):
    def one(x):
        offsets = ball_offsets(radius, x.shape, sampling)
        is_class = (x >= 0) & (x < K) & (x != background)
        best_d = np.full(x.shape, np.inf)
        best_c = np.full(x.shape, -1, dtype=np.int64)
        for o, d2 in offsets:
            here, there = _windows(x.shape, o)
            cand = is_class[there]
            c = x[there]
            better = cand & ((d2 < best_d[here]) | ((d2 == best_d[here]) & (c < best_c[here])))
            best_d[here] = np.where(better, d2, best_d[here])
            best_c[here] = np.where(better, c, best_c[here])
        out = x.copy()
        grow = (x == background) & (best_c >= 0)
        out[grow] = best_c[grow]
        return out
    return _per_entry(one, labels)


def opening_brute(labels, radius, K, sampling=None, background=0):
    def one(x):
        offsets = ball_offsets(radius, x.shape, sampling)
        out = x.copy()
        for k in _classes(K, background):
            member = x == k
            if not member.any():
                continue
            opened = _set_dilation(_set_erosion(member, offsets), offsets)
            assert not (opened & ~member).any()                 # anti-extensive
            out[member & ~opened] = background
        return out
    return _per_entry(one, labels)


def closing_brute(labels, radius, K, sampling=None, background=0):
    def one(x):
        offsets = ball_offsets(radius, x.shape, sampling)
        claims = np.zeros(x.shape, dtype=np.int64)
        who = np.full(x.shape, -1, dtype=np.int64)
        for k in _classes(K, background):
            member = x == k
            if not member.any():
                continue
            closed = _set_erosion(_set_dilation(member, offsets), offsets)
            assert not (member & ~closed).any()                 # extensive
            claims += closed
            who[closed] = k
        out = x.copy()
        take = (x == background) & (claims == 1)
        out[take] = who[take]
        return out
    return _per_entry(one, labels)


BRUTE = {"erosion": erosion_brute, "dilation": dilation_brute, "opening": opening_brute, "closing": closing_brute}


# ---- the label maps of tests/test_morph_gpu.py --------------------------------------------------------------------------------

def blobs(K, shape, seed=0):
    """Classes 1 .. K - 1 as overlapping balls of integer radii around seeded centres on background 0 (integer arithmetic and
    torch's seeded CPU generator: the same map on every machine).  A voxel takes the class of the nearest centre that covers it."""
    g = torch.Generator().manual_seed(1000 * K + seed)
    dims = shape[1:]
    voxels = 1
    for s in dims:
        voxels *= s
    m = max(8, 2 * (K - 1), voxels // 120)
    widest = 2 + max(1, min(5, min([s for s in dims if s > 1] or [1]) // 3))
    grids = torch.meshgrid(*[torch.arange(s) for s in dims], indexing="ij")
    out = torch.zeros(shape, dtype=torch.int64)
    for n in range(shape[0]):
        best = torch.full(dims, 2 ** 40, dtype=torch.int64)
        for i in range(m):
            centre = [int(torch.randint(0, s, (1,), generator=g)) for s in dims]
            r = int(torch.randint(2, widest + 1, (1,), generator=g))
            d2 = sum((gr - c) ** 2 for gr, c in zip(grids, centre))
            take = (d2 <= r * r) & (d2 < best)
            best = torch.where(take, d2, best)
            out[n][take] = 1 + i % (K - 1)
    return out


def percolation(shape, p=0.59, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < p).long()


def with_odd_labels(x, K, seed=5):
    """The map with -100 and K + 3 voxels scattered over it (about 2 % each): inside classes, beside them and in the background."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(x.shape, generator=g)
    out = x.clone()
    out[u < 0.02] = -100
    out[u > 0.98] = K + 3
    return out


def gap_between_two_classes(shape):
    """Class 1 | one background voxel | class 2 along the last axis, everywhere else background far away: (map, the gap's index)."""
    x = torch.zeros(shape, dtype=torch.int64)
    mid = tuple(s // 2 for s in shape[1:])
    lead = (0,) + mid[:-1]
    x[lead + (slice(mid[-1] - 4, mid[-1]),)] = 1
    x[lead + (slice(mid[-1] + 1, mid[-1] + 5),)] = 2
    return x, lead + (mid[-1],)


def tie_at_25(shape):
    """A background voxel at squared distance 25 from class 3 along the last axis, (0, 5), and from class 1 diagonally, (3, 4):
    (map, the voxel's index).  Everything else is background."""
    x = torch.zeros(shape, dtype=torch.int64)
    mid = tuple(s // 2 for s in shape[1:])
    at = (0,) + mid
    x[(0,) + mid[:-1] + (mid[-1] + 5,)] = 3
    x[(0,) + mid[:-2] + (mid[-2] + 3, mid[-1] - 4)] = 1
    return x, at


def two_discs_and_a_bridge(shape):
    """Two discs (balls in 3D) of class 1 of radius 4 joined by a bridge one voxel wide along the last axis: (map, bridge mask)."""
    dims = shape[1:]
    grids = torch.meshgrid(*[torch.arange(s) for s in dims], indexing="ij")
    mid = [s // 2 for s in dims]
    x = torch.zeros(shape, dtype=torch.int64)
    bridge = torch.zeros(shape, dtype=torch.bool)
    left, right = mid[-1] - 9, mid[-1] + 9
    for c in (left, right):
        d2 = sum((g - m) ** 2 for g, m in zip(grids[:-1], mid[:-1])) + (grids[-1] - c) ** 2
        x[0][d2 <= 16] = 1
    line = (0,) + tuple(mid[:-1]) + (slice(left + 5, right - 4),)
    bridge[line] = True
    x[line] = 1
    return x, bridge


def class_on_the_border(shape):
    """A block of class 1 that fills the low corner of the image: it touches the border on every axis."""
    x = torch.zeros(shape, dtype=torch.int64)
    x[(slice(None),) + tuple(slice(0, max(1, s // 2)) for s in shape[1:])] = 1
    return x


def seam_probe(shape, axis, seam, distance):
    """All class 1 but one voxel of class 2 at coordinate `seam` - 1 of spatial axis `axis` (the last voxel in front of the seam),
    the other coordinates in the middle; the class-1 voxel at `seam` - 1 + distance lies across the seam at exactly that distance:
    (map, its index)."""
    x = torch.ones(shape, dtype=torch.int64)
    mid = [s // 2 for s in shape[1:]]
    other = list(mid)
    other[axis] = seam - 1
    x[(0,) + tuple(other)] = 2
    probe = list(mid)
    probe[axis] = seam - 1 + distance
    assert probe[axis] < shape[1 + axis]
    return x, (0,) + tuple(probe)
