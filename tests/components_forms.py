"""Brute-force forms of common.postprocess (connected_components, keep_largest_component, remove_small_components), written from
their definitions in plain numpy / torch on the CPU (tests only), and the label maps of tests/test_components_gpu.py.

    adjacent:   offsets differ by at most 1 on every axis and on at most `connectivity` axes
    foreground: not `background` and, with num_classes = K, inside [0, K)
    connected:  adjacent, the same label, and that label is foreground
    numbering:  the components of an entry are numbered from 1 in the order of their smallest linear index (C order)

One entry at a time: the connected pairs are listed per offset, then a union-find in a Python loop over those pairs hangs the
larger root below the smaller one, so a root is the smallest linear index of its component."""
import itertools

import numpy as np
import torch

from tests.surface_forms import label_pair


def offsets_in_front(ndim, connectivity):
    """The offsets of half of the neighbourhood: the neighbours in front of a voxel in C order."""
    out = []
    for d in itertools.product((-1, 0, 1), repeat=ndim):
        if 1 <= sum(1 for c in d if c) <= connectivity and d < (0,) * ndim:
            out.append(d)
    return out


def foreground_of(x, background, num_classes):
    fg = x != background
    if num_classes is not None:
        fg &= (x >= 0) & (x < num_classes)
    return fg


def _roots_of_entry(x, connectivity, background, num_classes):
    """x (dims) int64 numpy -> (root per voxel: the smallest linear index of its component, -1 on background)."""
    nd = x.ndim
    fg = foreground_of(x, background, num_classes)
    index = np.arange(x.size).reshape(x.shape)
    parent = list(range(x.size))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for d in offsets_in_front(nd, connectivity):
        here = tuple(slice(max(0, -c), x.shape[a] - max(0, c)) for a, c in enumerate(d))
        there = tuple(slice(max(0, c), x.shape[a] - max(0, -c)) for a, c in enumerate(d))
        joined = fg[here] & fg[there] & (x[here] == x[there])
        for a, b in zip(index[here][joined].tolist(), index[there][joined].tolist()):
            ra, rb = find(a), find(b)
            if ra < rb:
                parent[rb] = ra
            elif rb < ra:
                parent[ra] = rb
    roots = np.array([find(i) for i in range(x.size)], dtype=np.int64).reshape(x.shape)
    roots[~fg] = -1
    return roots


def components_brute(labels, connectivity=1, background=0, num_classes=None):
    """(labels int32 (N, dims), count int64 (N,), sizes int32 (N, dims)) as torch CPU tensors."""
    x = torch.as_tensor(labels).cpu().numpy()
    out = np.zeros(x.shape, dtype=np.int32)
    sizes = np.zeros(x.shape, dtype=np.int32)
    count = np.zeros(x.shape[0], dtype=np.int64)
    for n in range(x.shape[0]):
        roots = _roots_of_entry(x[n], connectivity, background, num_classes)
        fg = roots >= 0
        uniq, inverse = np.unique(roots[fg], return_inverse=True)          # sorted: the order of the smallest linear index
        out[n][fg] = inverse.reshape(-1) + 1
        count[n] = uniq.size
        sizes[n][fg] = np.bincount(inverse.reshape(-1), minlength=uniq.size)[inverse.reshape(-1)]
    return torch.from_numpy(out), torch.from_numpy(count), torch.from_numpy(sizes)


def keep_largest_brute(labels, num_classes, connectivity=1, background=0, components=None):
    """The literal definition; `components`: components_brute(labels, connectivity, background, num_classes) if already there."""
    x = torch.as_tensor(labels).cpu()
    comp, _, _ = components if components is not None else components_brute(x, connectivity, background, num_classes)
    out = x.clone()
    for n in range(x.shape[0]):
        voxels = torch.bincount(comp[n].reshape(-1).long())
        for k in range(num_classes):
            if k == background:
                continue
            member = x[n] == k
            if not bool(member.any()):
                continue
            numbers = torch.unique(comp[n][member]).tolist()
            best = max(numbers, key=lambda c: (int(voxels[c]), -c))          # ties: the smaller number, i.e. the earlier first voxel
            out[n][member & (comp[n] != best)] = background
    return out


def remove_small_brute(labels, min_size, connectivity=1, background=0, num_classes=None, components=None):
    x = torch.as_tensor(labels).cpu()
    comp, _, sizes = components if components is not None else components_brute(x, connectivity, background, num_classes)
    out = x.clone()
    out[(comp > 0) & (sizes < min_size)] = background
    return out


# ---- the label maps of tests/test_components_gpu.py --------------------------------------------------------------------------

SHAPES = [(2, 5, 7),                   # smaller than a wave
          (3, 36, 57),                 # tails in both axes
          (1, 70, 130),                # rows longer than a wave
          (1, 600, 9), (1, 9, 600),    # one axis far longer than any tile: many seams along one direction
          (2, 6, 10, 70),              # 3D
          (1, 33, 9, 5),               # 3D with the longest axis outermost
          (1, 20, 20, 40)]             # 3D with several slabs


def two_tiles_and_one(tile):
    """(1, dims): exactly two tiles along every tiled axis plus a tail of one voxel."""
    return (1,) + tuple(2 * t + 1 for t in tile)


def shape_id(shape):
    return "x".join(map(str, shape))


def blocks(K, shape):
    """The target map of surface_forms.label_pair: random blocks, 5 % of the voxels at -100 and one at K + 3."""
    return label_pair(K, shape, seed=K)[1]


def percolation(shape, p=0.59, seed=1):
    """Bernoulli(p) of class 1 on class 0: near the site-percolation threshold of the square lattice, large tortuous clusters."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < p).long()


def three_classes(shape, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 3, shape, generator=g)


def _serpentine_2d(H, W):
    """Every second row full, the rows joined alternately at the right and the left end: one component."""
    m = torch.zeros(H, W, dtype=torch.int64)
    m[0::2] = 1
    for j, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if j % 2 == 0 else 0] = 1
    return m


def _serpentine(dims):
    if len(dims) == 2:
        return _serpentine_2d(*dims)
    D, H, W = dims
    m = torch.zeros(D, H, W, dtype=torch.int64)
    last = H - 1 if H % 2 == 1 else H - 2                                  # the last full row of a slice
    for z in range(0, D, 2):
        m[z] = _serpentine_2d(H, W)
    for j, z in enumerate(range(1, D - 1, 2)):                              # the slices in between: one voxel at alternating corners
        if j % 2 == 0:
            m[z, last, W - 1] = 1
        else:
            m[z, 0, 0] = 1
    return m


def serpentine(shape):
    return torch.stack([_serpentine(shape[1:]) for _ in range(shape[0])])


def double_serpentine(shape):
    """Two serpentines of the same class side by side, one background voxel apart along the last axis: two components."""
    dims, W = shape[1:], shape[-1]
    m = torch.zeros(shape, dtype=torch.int64)
    half = W // 2
    if half < 1 or W - half - 1 < 1:
        return serpentine(shape)
    m[..., :half] = torch.stack([_serpentine(dims[:-1] + (half,)) for _ in range(shape[0])])
    m[..., half + 1:] = torch.stack([_serpentine(dims[:-1] + (W - half - 1,)) for _ in range(shape[0])])
    return m


def u_shape(shape):
    """Two arms along the first spatial axis at opposite corners of the other axes, joined only at the far end."""
    m = torch.zeros(shape, dtype=torch.int64)
    if len(shape) == 3:
        m[:, :, 0] = 1
        m[:, :, -1] = 1
        m[:, -1, :] = 1
    else:
        m[:, :, 0, 0] = 1
        m[:, :, -1, -1] = 1
        m[:, -1, :, 0] = 1
        m[:, -1, -1, :] = 1
    return m


def checkerboard(shape):
    grids = torch.meshgrid(*[torch.arange(s) for s in shape[1:]], indexing="ij")
    return ((sum(grids) % 2) == 0).long().unsqueeze(0).repeat(shape[0], *([1] * (len(shape) - 1))).contiguous()


def _corner(shape, tile):
    """The first voxel behind the first tile corner, or the middle of an axis that has only one tile."""
    return tuple(t if s > t else max(1, s // 2) for s, t in zip(shape[1:], tile))


def crossing_lines(shape, tile):
    """A diagonal of class 1 and an anti-diagonal of class 2 in the last two axes (a space diagonal in 3D) that cross between
    the voxels at a tile corner: they share no voxel and never merge."""
    m = torch.zeros(shape, dtype=torch.int64)
    c = _corner(shape, tile)
    for t in range(-max(shape), max(shape)):
        lead = tuple(ci - 1 + t for ci in c[:-1])
        for x, k in ((c[-1] - 1 + t, 1), (c[-1] - t, 2)):
            at = lead + (x,)
            if all(0 <= a < s for a, s in zip(at, shape[1:])):
                m[(slice(None),) + at] = k
    return m


def corner_pairs(shape, tile):
    """{name: (map, connectivity from which the two voxels are one component)}: pairs of voxels of class 1 that touch only
    across a tile corner (2D), a tile edge or a tile corner (3D)."""
    c = _corner(shape, tile)
    out = {}
    if len(c) == 2:
        m = torch.zeros(shape, dtype=torch.int64)
        m[:, c[0] - 1, c[1] - 1] = 1
        m[:, c[0], c[1]] = 1
        out["corner"] = (m, 2)
        m = torch.zeros(shape, dtype=torch.int64)
        m[:, c[0] - 1, c[1]] = 1
        m[:, c[0], c[1] - 1] = 1
        out["anti-corner"] = (m, 2)
    else:
        for name, skip in (("edge-zy", 2), ("edge-zx", 1), ("edge-yx", 0)):
            m = torch.zeros(shape, dtype=torch.int64)
            a = [ci - 1 for ci in c]
            b = list(c)
            b[skip] = a[skip] = min(c[skip] + 1, shape[1 + skip] - 1)         # the same coordinate on the third axis
            m[(slice(None),) + tuple(a)] = 1
            m[(slice(None),) + tuple(b)] = 1
            out[name] = (m, 2)
        m = torch.zeros(shape, dtype=torch.int64)
        m[(slice(None),) + tuple(ci - 1 for ci in c)] = 1
        m[(slice(None),) + tuple(c)] = 1
        out["corner"] = (m, 3)
    return out


def trivial_maps(shape):
    single = torch.zeros(shape, dtype=torch.int64)
    single.reshape(shape[0], -1)[:, -1] = 1
    return {"background": torch.zeros(shape, dtype=torch.int64), "full": torch.ones(shape, dtype=torch.int64), "single": single}
