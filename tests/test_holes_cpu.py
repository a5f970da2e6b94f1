"""The brute-force form of tests/holes_forms.py against scipy.ndimage.binary_fill_holes and against a second construction built
from scipy's label and binary_dilation; the outcomes the constructed maps are built for; and what fill_holes / find_holes do on the
host: the workspace query and the refusals of the C entry, the argument checks, the refusal of CPU tensors and the alias."""
import ctypes

import numpy as np
import pytest
import torch

from tests import holes_forms as H
from tests.components_forms import blocks, percolation, three_classes

TILES = {2: (32, 64), 3: (4, 8, 64)}
SMALL = [(3, 36, 57), (1, 65, 129), (2, 6, 10, 70), (1, 9, 17, 129)]


@pytest.mark.parametrize("shape", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_brute_force_form_is_scipy_binary_fill_holes_on_masks(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    x = percolation(shape, p=0.59)
    for connectivity in range(1, len(shape)):
        structure = ndi.generate_binary_structure(len(shape) - 1, connectivity)
        out, fill, count, voxels = H.fill_holes_brute(x, 2, connectivity)
        want = np.stack([ndi.binary_fill_holes(e.numpy() != 0, structure=structure) for e in x]).astype(np.int64)
        assert torch.equal(out, torch.from_numpy(want)), connectivity
        assert torch.equal(fill >= 0, out != x) and torch.equal(torch.where(fill >= 0, fill, x), out)
        assert voxels[:, 1].tolist() == (out != x).flatten(1).sum(1).tolist() and voxels[:, 0].tolist() == [0] * shape[0]
        assert bool((count <= voxels).all())


def _scipy_construction(x, K, connectivity, background, max_size=None):
    """ndimage.label of the background mask, binary_dilation for the ring of neighbours, the border test on the member mask."""
    ndi = pytest.importorskip("scipy.ndimage")
    x = x.numpy()
    nd = x.ndim - 1
    structure = ndi.generate_binary_structure(nd, connectivity)
    out = x.copy()
    fill = np.full(x.shape, -1, dtype=np.int64)
    count = np.zeros((x.shape[0], K), dtype=np.int64)
    voxels = np.zeros((x.shape[0], K), dtype=np.int64)
    for n in range(x.shape[0]):
        bg = x[n] == background
        lab, m = ndi.label(bg, structure=structure)
        for c in range(1, m + 1):
            member = lab == c
            if any(np.take(member, face, axis=a).any() for a in range(nd) for face in (0, -1)):
                continue
            ring = ndi.binary_dilation(member, structure=structure) & ~bg
            around = np.unique(x[n][ring])
            if around.size != 1 or not 0 <= int(around[0]) < K:
                continue
            if max_size is not None and int(member.sum()) > max_size:
                continue
            k = int(around[0])
            out[n][member] = k
            fill[n][member] = k
            count[n, k] += 1
            voxels[n, k] += int(member.sum())
    return tuple(torch.from_numpy(a) for a in (out, fill, count, voxels))


MAPS = [("three-2d", lambda: three_classes((2, 13, 21)), 3, 0), ("three-3d", lambda: three_classes((1, 6, 10, 14)), 3, 0),
        ("three-2d-background-2", lambda: three_classes((2, 13, 21)), 3, 2),
        ("three-3d-background-2", lambda: three_classes((1, 6, 10, 14)), 3, 2),
        ("three-2d-two-classes", lambda: three_classes((2, 13, 21)), 2, 0),
        ("blocks-2d", lambda: blocks(4, (2, 13, 21)), 4, 0), ("blocks-3d", lambda: blocks(4, (1, 6, 10, 14)), 4, 0),
        ("blocks-2d-background-2", lambda: blocks(4, (2, 13, 21)), 4, 2),
        ("blocks-2d-background-minus-100", lambda: blocks(4, (3, 36, 57)), 4, -100)]


@pytest.mark.parametrize("name,make,K,background", MAPS, ids=[m[0] for m in MAPS])
def test_brute_force_form_is_the_scipy_construction_on_class_maps(name, make, K, background):
    x = make()
    for connectivity in range(1, x.dim()):
        for max_size in (None, 1, 3):
            got = H.fill_holes_brute(x, K, connectivity, background, max_size)
            want = _scipy_construction(x, K, connectivity, background, max_size)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and torch.equal(g, w), (name, connectivity, max_size)


def test_the_random_maps_of_the_gpu_tests_are_not_vacuous():
    for shape in ((1, 65, 129), (3, 36, 57)):
        assert H.kinds(percolation(shape), 2)[H.FILLED] >= 50
        three = H.kinds(three_classes(shape), 3)
        assert three[H.FILLED] >= 1 and three[H.BORDER] >= 1 and three[H.MIXED] >= 1
    for shape in ((1, 9, 17, 129), (2, 6, 10, 70)):
        assert H.kinds(percolation(shape), 2)[H.FILLED] >= 50
        assert H.kinds(percolation(shape), 2, max_size=3)[H.TOO_LARGE] >= 1


def test_filling_is_idempotent():
    for x, K in ((percolation((3, 36, 57)), 2), (three_classes((2, 13, 21)), 3), (blocks(4, (1, 6, 10, 14)), 4)):
        for connectivity in range(1, x.dim()):
            once = H.fill_holes_brute(x, K, connectivity)[0]
            again = H.fill_holes_brute(once, K, connectivity)
            assert torch.equal(again[0], once) and int(again[2].sum()) == 0 and bool((again[1] == -1).all())


@pytest.mark.parametrize("shape", [(1, 65, 129), (1, 9, 17, 129)], ids=["2d", "3d"])
def test_constructed_maps_have_the_outcomes_they_are_built_for(shape):
    nd = len(shape) - 1
    tile = TILES[nd]
    cavity = H.cavity_voxels(shape)
    assert cavity == (8125 if nd == 3 else 61 * 125)
    for c in range(1, nd + 1):
        box = H.hollow_box(shape)
        out, fill, count, voxels = H.fill_holes_brute(box, 2, c)
        assert count.tolist() == [[0, 1]] and voxels.tolist() == [[0, cavity]]
        want = torch.zeros(shape, dtype=torch.int64)
        H._inner(want, 1)[...] = 1
        assert torch.equal(out, want) and H.kinds(box, 2, c) == {H.FILLED: 1, H.BORDER: 1, H.MIXED: 0, H.TOO_LARGE: 0}

        island = H.box_with_island(shape)
        out, fill, count, voxels = H.fill_holes_brute(island, 3, c)
        assert count.tolist() == [[0, 0, 1]] and H.kinds(island, 3, c)[H.MIXED] == 1
        assert int((out != island).sum()) == int(voxels[0, 2]) > 0
        assert int(out[(0,) + (2,) * nd]) == 0 and int(fill.max()) == 2 and int((fill == 2).sum()) == int(voxels[0, 2])   # the outer cavity stays
        assert H.fill_holes_brute(island, 2, c)[2].tolist() == [[0, 0]]          # class 2 is outside [0, 2): nothing is filled

        for far in (False, True):
            leaky = H.leaky_box(shape, far)
            filled = int(H.fill_holes_brute(leaky, 2, c)[3][0, 1])
            assert filled == (cavity if c < nd else 0), (c, far)

        for axis, low in ((nd - 1, False), (0, True)):
            contact = H.border_contact(shape, tile, axis, low)
            assert int(contact.select(1 + axis, 0 if low else shape[1 + axis] - 1).eq(0).sum()) == 1
            assert H.kinds(contact, 2, c) == {H.FILLED: 0, H.BORDER: 1, H.MIXED: 0, H.TOO_LARGE: 0}

        assert H.fill_holes_brute(H.poisoned_hole(shape, tile, False), 2, c)[2].tolist() == [[0, 0]]
        diagonal = H.fill_holes_brute(H.poisoned_hole(shape, tile, True), 2, c)
        assert diagonal[2].tolist() == [[0, 1 if c < nd else 0]] and diagonal[3].tolist() == [[0, 2 ** nd if c < nd else 0]]

        sizes = H.two_sizes(shape, tile, 5)
        assert H.fill_holes_brute(sizes, 2, c)[3].tolist() == [[0, 11]]
        assert H.fill_holes_brute(sizes, 2, c, max_size=5)[3].tolist() == [[0, 5]]
        assert H.fill_holes_brute(sizes, 2, c, max_size=6)[3].tolist() == [[0, 11]]
        assert H.fill_holes_brute(sizes, 2, c, max_size=4)[3].tolist() == [[0, 0]]

    snake = H.serpentine_hole(shape)
    out, fill, count, voxels = H.fill_holes_brute(snake, 2, 1)
    assert count.tolist() == [[0, 1]] and bool((out == 1).all()) and int(voxels[0, 1]) == int((snake == 0).sum())
    odd = H.serpentine_hole(shape, odd_voxel=True)
    assert H.fill_holes_brute(odd, 3, 1)[2].tolist() == [[0, 0, 0]] and H.kinds(odd, 3, 1)[H.MIXED] == 1

    three = (3,) + shape[1:]
    out, fill, count, voxels = H.fill_holes_brute(H.mixed_entries(three), 2, nd)
    assert count.tolist() == [[0, 1], [0, 0], [0, 0]] and voxels.tolist() == [[0, cavity], [0, 0], [0, 0]]
    assert bool((out[1] == 0).all()) and bool((out[2] == 1).all())


def _address(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_workspace_query_and_host_refusals_of_the_c_entry():
    from advchain_amd import _lib
    lib = _lib.load()
    for N, sp in ((3, (36, 57)), (2, (6, 10, 70)), (1, (1, 1)), (1, (2049, 1))):
        V = int(np.prod(sp))
        assert lib.advchain_fill_holes_workspace(N, len(sp), _lib.dims_array(sp)) == N * (4 * V + (V + 2047) // 2048)
    dims = _lib.dims_array((36, 57))
    # refused exactly where advchain_components_workspace is
    for N, nd, d in ((0, 2, dims), (1, 1, dims), (1, 4, dims), (1, 2, None), (1, 2, _lib.dims_array((0, 5))),
                     (1, 2, _lib.dims_array((2 ** 16, 2 ** 15))), (1, 3, _lib.dims_array((2 ** 10, 2 ** 10, 2 ** 11))),
                     (1, 2, _lib.dims_array((2 ** 15, 2 ** 15))), (4, 2, _lib.dims_array((2 ** 14, 2 ** 14)))):
        assert lib.advchain_components_workspace(N, nd, d) == -1 and lib.advchain_fill_holes_workspace(N, nd, d) == -1
    assert lib.advchain_fill_holes_workspace(3, 2, _lib.dims_array((2 ** 14, 2 ** 14))) == 3 * (2 ** 30 + 2 ** 17)

    # host memory stands in for the buffers: every call below is refused before anything is launched
    V = 36 * 57
    x, out, fill = (np.zeros(V, dtype=np.int64) for _ in range(3))
    count, voxels = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    ws = np.zeros(4 * V + 2, dtype=np.int32)
    X, O, F, C, W, S = (_address(a) for a in (x, out, fill, count, voxels, ws))

    def refused(args, code=-1):
        rc = lib.advchain_fill_holes(*args)
        assert rc == code and b"fill_holes" in lib.advchain_last_error(), (rc, lib.advchain_last_error())

    good = [X, O, F, C, W, S, 1, 2, 2, dims, 1, 0, -1, None]

    def but(**kw):
        names = ["labels", "out", "fill", "count", "voxels", "workspace", "N", "K", "ndim", "dims", "connectivity", "background",
                 "max_size", "stream"]
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args

    refused(but(labels=None))
    refused(but(workspace=None))
    refused(but(dims=None))
    refused(but(count=None))                                  # count and voxels are null together
    refused(but(voxels=None))
    refused(but(out=None, fill=None, count=None, voxels=None))
    refused(but(out=X))
    refused(but(fill=X))
    for K in (0, -1, 65536):
        refused(but(K=K))
    for c in (0, 3, -1):
        refused(but(connectivity=c))
    refused(but(ndim=3, dims=_lib.dims_array((4, 9, 57)), connectivity=4))
    refused(but(max_size=0))
    refused(but(N=0))
    refused(but(ndim=4))
    refused(but(dims=_lib.dims_array((0, 5))))
    refused(but(dims=_lib.dims_array((2 ** 16, 2 ** 15))), code=-2)
    refused(but(N=4, dims=_lib.dims_array((2 ** 14, 2 ** 14))), code=-2)


def test_host_side_checks_raise_value_errors():
    import advchain.common.postprocess as P
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    y3 = torch.zeros(1, 4, 8, 8, dtype=torch.int64)
    for fn in (P.fill_holes, P.find_holes):
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros(8, 8, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros(1, 1, 2, 8, 8, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="3-D"):
            fn([[[0]]], 2)
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(0, 8, 8, dtype=torch.int64), 2)
        for c in (0, 3, -1, 1.0, True, None):
            with pytest.raises(ValueError, match="connectivity"):
                fn(y, 2, connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            fn(y3, 2, connectivity=4)
        with pytest.raises(ValueError, match="background"):
            fn(y, 2, background=0.0)
        for K in (0, 2.0, True, None):
            with pytest.raises(ValueError, match="num_classes"):
                fn(y, K)
        for m in (0, -3, 2.0, True, "2"):
            with pytest.raises(ValueError, match="max_size"):
                fn(y, 2, max_size=m)
        with pytest.raises(ValueError, match=fn.__name__):
            fn(y, 2, max_size=0)


def test_cpu_tensors_are_refused_and_the_alias():
    import advchain.common.postprocess as P
    import advchain_amd.common.postprocess as P2
    from advchain_amd import ops
    from advchain_amd._lib import AdvchainHipError
    assert P is P2 and P.Holes is ops.Holes and P.Holes._fields == ("fill", "count", "voxels")
    assert ops.COMPONENTS_TILE == TILES
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    for kw in ({}, {"max_size": 2 ** 70}, {"background": 5, "connectivity": 2}):
        with pytest.raises(AdvchainHipError):
            P.fill_holes(y, 2, **kw)
        with pytest.raises(AdvchainHipError):
            P.find_holes(y, 2, **kw)
