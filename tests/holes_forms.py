"""Brute-force form of common.postprocess.fill_holes / find_holes, written from the definitions in plain numpy / torch on the CPU
(tests only, independent of scipy), and the constructed label maps of tests/test_holes_gpu.py.

    background component: a component (components_forms.components_brute) of the mask ``labels == background``
    touches the border:   one of its voxels has a coordinate 0 or size - 1 on a spatial axis
    enclosing labels:     the labels of the voxels adjacent (same connectivity) to one of its voxels that are not background
    hole:                 does not touch the border, exactly one enclosing label k, 0 <= k < K, at most max_size voxels

One entry at a time: the (component, neighbouring label) pairs are listed per offset of the whole neighbourhood and collected
into one set of labels per component; then every component is judged on its own."""
import itertools

import numpy as np
import torch

from tests.components_forms import _corner, components_brute, serpentine

FILLED, BORDER, MIXED, TOO_LARGE = "filled", "border", "mixed", "too large"


def offsets_all_around(ndim, connectivity):
    return [d for d in itertools.product((-1, 0, 1), repeat=ndim) if 1 <= sum(1 for c in d if c) <= connectivity]


def classify_background(labels, K, connectivity=1, background=0, max_size=None):
    """Per entry a list of (member mask, kind, k, size) for every background component, in the order of the first voxel.  kind:
    BORDER, MIXED (two enclosing labels, or one outside [0, K)), TOO_LARGE or FILLED; k is the enclosing class or None."""
    x = torch.as_tensor(labels).cpu()
    comp, count, sizes = components_brute((x == background).long(), connectivity)
    x = x.numpy()
    nd = x.ndim - 1
    out = []
    for n in range(x.shape[0]):
        c = comp[n].numpy()
        m = int(count[n])
        on_border = set()
        for axis in range(nd):
            for face in (0, c.shape[axis] - 1):
                on_border.update(np.unique(np.take(c, face, axis=axis)).tolist())
        enclosing = {i: set() for i in range(1, m + 1)}
        for d in offsets_all_around(nd, connectivity):
            here = tuple(slice(max(0, -e), c.shape[a] - max(0, e)) for a, e in enumerate(d))
            there = tuple(slice(max(0, e), c.shape[a] - max(0, -e)) for a, e in enumerate(d))
            sel = (c[here] > 0) & (x[n][there] != background)
            for i, y in set(zip(c[here][sel].tolist(), x[n][there][sel].tolist())):
                enclosing[i].add(y)
        entry = []
        for i in range(1, m + 1):
            member = c == i
            size = int(member.sum())
            k = next(iter(enclosing[i])) if len(enclosing[i]) == 1 else None
            if i in on_border:
                kind = BORDER
            elif k is None or not 0 <= k < K:
                kind = MIXED
            elif max_size is not None and size > max_size:
                kind = TOO_LARGE
            else:
                kind = FILLED
            entry.append((member, kind, k, size))
        out.append(entry)
    return out


def fill_holes_brute(labels, K, connectivity=1, background=0, max_size=None):
    """(out int64 (N, dims), fill int64 (N, dims), count int64 (N, K), voxels int64 (N, K)) as torch CPU tensors."""
    x = torch.as_tensor(labels).cpu()
    out = x.clone().numpy()
    fill = np.full(out.shape, -1, dtype=np.int64)
    count = np.zeros((out.shape[0], K), dtype=np.int64)
    voxels = np.zeros((out.shape[0], K), dtype=np.int64)
    for n, entry in enumerate(classify_background(x, K, connectivity, background, max_size)):
        for member, kind, k, size in entry:
            if kind == FILLED:
                out[n][member] = k
                fill[n][member] = k
                count[n, k] += 1
                voxels[n, k] += size
    return torch.from_numpy(out), torch.from_numpy(fill), torch.from_numpy(count), torch.from_numpy(voxels)


def kinds(labels, K, connectivity=1, background=0, max_size=None):
    """{kind: number of background components of that kind}, over all entries."""
    out = {FILLED: 0, BORDER: 0, MIXED: 0, TOO_LARGE: 0}
    for entry in classify_background(labels, K, connectivity, background, max_size):
        for _, kind, _, _ in entry:
            out[kind] += 1
    return out


# ---- the constructed maps of tests/test_holes_gpu.py: (N, dims) with at least 9 voxels along every spatial axis -------------------

def _inner(m, margin):
    """The view of m without `margin` voxels at both ends of every spatial axis."""
    return m[(slice(None),) + (slice(margin, -margin),) * (m.dim() - 1)]


def hollow_box(shape):
    """A box of class 1 with a wall one voxel thick, one voxel away from the border; the cavity is one hole, the outer shell of
    the entry a background component that touches the border."""
    m = torch.zeros(shape, dtype=torch.int64)
    _inner(m, 1)[...] = 1
    _inner(m, 2)[...] = 0
    return m


def cavity_voxels(shape):
    out = 1
    for s in shape[1:]:
        out *= s - 4
    return out


def box_with_island(shape):
    """The hollow box with an island of class 2 in its cavity (two enclosing labels: not filled) and a cavity inside the island
    (filled with 2)."""
    m = hollow_box(shape)
    _inner(m, 3)[...] = 2
    _inner(m, 4)[...] = 0
    return m


def leaky_box(shape, far=False):
    """The hollow box without the wall voxel at the corner (1, .., 1), or with far=True at (size - 2, ..): the cavity reaches the
    outside only diagonally on every axis, i.e. only at full connectivity."""
    m = hollow_box(shape)
    m[(slice(None),) + tuple((s - 2 if far else 1) for s in shape[1:])] = 0
    return m


def border_contact(shape, tile, axis, low):
    """All of class 1 but a cavity at the first tile corner and a tunnel one voxel wide from it along spatial axis `axis` to the
    border (coordinate 0 with low, else size - 1): the cavity's only contact with the border is the last voxel of the tunnel."""
    m = torch.ones(shape, dtype=torch.int64)
    c = _corner(shape, tile)
    m[(slice(None),) + tuple(slice(ci - 1, ci + 1) for ci in c)] = 0
    at = [slice(ci, ci + 1) for ci in c]
    at[axis] = slice(0, c[axis]) if low else slice(c[axis], shape[1 + axis])
    m[(slice(None),) + tuple(at)] = 0
    return m


def serpentine_hole(shape, odd_voxel=False):
    """components_forms.serpentine as background inside a frame of class 1 one voxel thick: one long thin hole through every tile.
    odd_voxel: one voxel of the frame that is a face neighbour of the hole is of class 2."""
    m = torch.ones(shape, dtype=torch.int64)
    inner = (shape[0],) + tuple(s - 2 for s in shape[1:])
    _inner(m, 1)[...] = 1 - serpentine(inner)
    if odd_voxel:
        m[(slice(None), shape[1] - 1) + tuple(s - 2 for s in shape[2:])] = 2
    return m


def poisoned_hole(shape, tile, diagonal):
    """All of class 1 but a cavity of two voxels per axis across the first tile corner, and one voxel of -100: a face neighbour
    of the cavity, or with diagonal=True the voxel that touches the cavity's first corner on every axis only."""
    m = torch.ones(shape, dtype=torch.int64)
    c = _corner(shape, tile)
    m[(slice(None),) + tuple(slice(ci - 1, ci + 1) for ci in c)] = 0
    if diagonal:
        m[(slice(None),) + tuple(ci - 2 for ci in c)] = -100
    else:
        m[(slice(None),) + tuple(ci - 2 if a == len(c) - 1 else ci for a, ci in enumerate(c))] = -100
    return m


def two_sizes(shape, tile, m_voxels):
    """All of class 1 but two holes in rows along the last axis across the first tile corner: one of m_voxels, one of
    m_voxels + 1 voxels."""
    m = torch.ones(shape, dtype=torch.int64)
    c = _corner(shape, tile)
    lo = c[-1] - m_voxels // 2
    m[(slice(None),) + tuple(c[:-1]) + (slice(lo, lo + m_voxels),)] = 0
    m[(slice(None),) + tuple(ci - 2 for ci in c[:-1]) + (slice(lo, lo + m_voxels + 1),)] = 0
    return m


def mixed_entries(shape):
    """N = 3: a hollow box, an all-background entry, an entry without a background voxel.  The cavity of entry 0 lies over
    background of entry 1: nothing pairs up across entries."""
    one = (1,) + tuple(shape[1:])
    return torch.cat([hollow_box(one), torch.zeros(one, dtype=torch.int64), torch.ones(one, dtype=torch.int64)])
