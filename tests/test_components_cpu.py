"""The brute-force forms of tests/components_forms.py against scipy.ndimage.label, and what common.postprocess does on the host:
the workspace query and the refusals of the C entries, the argument checks, the refusal of CPU tensors and the alias."""
import numpy as np
import pytest
import torch

from tests.components_forms import (blocks, checkerboard, components_brute, corner_pairs, crossing_lines, double_serpentine,
                                    keep_largest_brute, offsets_in_front, percolation, remove_small_brute, serpentine, three_classes,
                                    u_shape)


def _scipy_components(x, connectivity, background, num_classes):
    """scipy.ndimage.label per entry and label value, the components of an entry renumbered by their first voxel."""
    ndi = pytest.importorskip("scipy.ndimage")
    x = x.numpy()
    structure = ndi.generate_binary_structure(x.ndim - 1, connectivity)
    out = np.zeros(x.shape, dtype=np.int32)
    sizes = np.zeros(x.shape, dtype=np.int32)
    count = np.zeros(x.shape[0], dtype=np.int64)
    for n in range(x.shape[0]):
        first = []                                                       # (first linear index, value, scipy's number)
        per_value = {}
        for value in np.unique(x[n]).tolist():
            if value == background or (num_classes is not None and not 0 <= value < num_classes):
                continue
            lab, m = ndi.label(x[n] == value, structure=structure)
            per_value[value] = lab
            flat = lab.reshape(-1)
            for c in range(1, m + 1):
                first.append((int(np.argmax(flat == c)), value, c))
        for number, (_, value, c) in enumerate(sorted(first), 1):
            member = per_value[value] == c
            out[n][member] = number
            sizes[n][member] = int(member.sum())
        count[n] = len(first)
    return torch.from_numpy(out), torch.from_numpy(count), torch.from_numpy(sizes)


MAPS = [("blocks-2d", lambda: blocks(4, (2, 13, 21)), 4), ("blocks-3d", lambda: blocks(4, (1, 6, 10, 14)), 4),
        ("blocks-unbounded", lambda: blocks(4, (2, 13, 21)), None), ("percolation-2d", lambda: percolation((1, 24, 31)), None),
        ("percolation-3d", lambda: percolation((1, 7, 9, 11), p=0.3), None), ("three-2d", lambda: three_classes((2, 12, 17)), 3),
        ("three-3d", lambda: three_classes((1, 5, 6, 9)), None), ("checkerboard-3d", lambda: checkerboard((1, 4, 5, 6)), None)]


@pytest.mark.parametrize("name,make,K", MAPS, ids=[m[0] for m in MAPS])
def test_brute_force_form_is_scipy_label_renumbered_by_first_voxel(name, make, K):
    x = make()
    for connectivity in range(1, x.dim()):
        for background in (0, 2):
            got = components_brute(x, connectivity, background, K)
            want = _scipy_components(x, connectivity, background, K)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and torch.equal(g, w), (name, connectivity, background)


def test_offsets_are_half_of_scipy_s_structure():
    ndi = pytest.importorskip("scipy.ndimage")
    for nd in (2, 3):
        for connectivity in range(1, nd + 1):
            front = offsets_in_front(nd, connectivity)
            both = set(front) | set(tuple(-c for c in d) for d in front)
            structure = ndi.generate_binary_structure(nd, connectivity)
            want = set(tuple(int(i) - 1 for i in at) for at in np.argwhere(structure)) - {(0,) * nd}
            assert both == want and len(front) * 2 == len(want)
    assert [len(offsets_in_front(nd, c)) for nd, c in ((2, 1), (2, 2), (3, 1), (3, 2), (3, 3))] == [2, 4, 3, 9, 13]


def test_constructed_maps_have_the_components_they_are_built_for():
    for shape, tile in (((1, 9, 13), (4, 8)), ((1, 5, 6, 9), (2, 2, 4))):
        full = len(shape) - 1
        assert components_brute(serpentine(shape), 1)[1].tolist() == [1]
        assert components_brute(double_serpentine(shape), 1)[1].tolist() == [2]
        assert components_brute(double_serpentine(shape), full)[1].tolist() == [2]
        assert components_brute(u_shape(shape), 1)[1].tolist() == [1]
        board = checkerboard(shape)
        assert components_brute(board, 1)[1].tolist() == [int(board.sum())]
        assert components_brute(board, full)[1].tolist() == [1]
        lines = crossing_lines(shape, tile)
        assert components_brute(lines, full)[1].tolist() == [2] and components_brute(lines, 1)[1].tolist() == [int((lines > 0).sum())]
        for name, (m, joined_from) in corner_pairs(shape, tile).items():
            for connectivity in range(1, full + 1):
                assert components_brute(m, connectivity)[1].tolist() == [1 if connectivity >= joined_from else 2], name


def test_filters_are_their_definitions():
    x = torch.zeros(1, 5, 9, dtype=torch.int64)
    x[0, 0, 0:3] = 1          # three voxels, first
    x[0, 2, 0:3] = 1          # three voxels, later: loses the tie
    x[0, 4, 0:2] = 1
    x[0, 0, 6:9] = 2
    x[0, 2, 8] = 2
    x[0, 4, 8] = 7            # outside [0, 3): copied
    kept = keep_largest_brute(x, 3)
    want = x.clone()
    want[0, 2, 0:3] = 0
    want[0, 4, 0:2] = 0
    want[0, 2, 8] = 0
    assert torch.equal(kept, want)
    assert torch.equal(remove_small_brute(x, 1, num_classes=3), x) and torch.equal(remove_small_brute(x, 1), x)
    small = remove_small_brute(x, 3)
    want = x.clone()
    want[0, 4, 0:2] = 0
    want[0, 2, 8] = 0
    want[0, 4, 8] = 0
    assert torch.equal(small, want)
    want[0, 4, 8] = 7          # with a class count the label 7 is in no component: copied
    assert torch.equal(remove_small_brute(x, 3, num_classes=3), want)


def test_workspace_query_and_host_refusals_of_the_c_entries():
    from advchain_amd import _lib
    lib = _lib.load()
    for N, sp in ((3, (36, 57)), (2, (6, 10, 70)), (1, (1, 1)), (1, (2049, 1))):
        V = int(np.prod(sp))
        assert lib.advchain_components_workspace(N, len(sp), _lib.dims_array(sp)) == N * (2 * V + (V + 2047) // 2048)
    dims = _lib.dims_array((36, 57))
    assert lib.advchain_components_workspace(0, 2, dims) == -1
    assert lib.advchain_components_workspace(1, 1, dims) == -1 and lib.advchain_components_workspace(1, 4, dims) == -1
    assert lib.advchain_components_workspace(1, 2, None) == -1
    assert lib.advchain_components_workspace(1, 2, _lib.dims_array((0, 5))) == -1
    assert lib.advchain_components_workspace(1, 2, _lib.dims_array((2 ** 16, 2 ** 15))) == -1          # 2^31 voxels in an entry
    assert lib.advchain_components_workspace(1, 3, _lib.dims_array((2 ** 10, 2 ** 10, 2 ** 11))) == -1
    assert lib.advchain_components_workspace(1, 2, _lib.dims_array((2 ** 15, 2 ** 15))) == -1          # 2^31 words of parents and sizes
    assert lib.advchain_components_workspace(4, 2, _lib.dims_array((2 ** 14, 2 ** 14))) == -1
    assert lib.advchain_components_workspace(3, 2, _lib.dims_array((2 ** 14, 2 ** 14))) == 3 * (2 ** 29 + 2 ** 17)
    rc = lib.advchain_components(None, None, None, None, None, 1, 2, dims, 1, 0, -1, None)
    assert rc < 0 and b"components" in lib.advchain_last_error()
    rc = lib.advchain_keep_largest(None, None, None, None, 1, 2, 2, dims, 1, 0, None)
    assert rc < 0 and b"keep_largest" in lib.advchain_last_error()
    rc = lib.advchain_remove_small(None, None, None, 1, 2, dims, 1, 0, -1, 1, None)
    assert rc < 0 and b"remove_small" in lib.advchain_last_error()


def test_host_side_checks_raise_value_errors():
    import advchain.common.postprocess as P
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    y3 = torch.zeros(1, 4, 8, 8, dtype=torch.int64)
    calls = (lambda t, **kw: P.connected_components(t, **kw), lambda t, **kw: P.keep_largest_component(t, 2, **kw),
             lambda t, **kw: P.remove_small_components(t, 2, **kw))
    for fn in calls:
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros(8, 8, dtype=torch.int64))
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros(1, 1, 2, 8, 8, dtype=torch.int64))
        with pytest.raises(ValueError, match="3-D"):
            fn([[[0]]])
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(0, 8, 8, dtype=torch.int64))
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(2, 0, 8, dtype=torch.int64))
        for c in (0, 3, -1, 1.0, True, None):
            with pytest.raises(ValueError, match="connectivity"):
                fn(y, connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            fn(y3, connectivity=4)
        with pytest.raises(ValueError, match="background"):
            fn(y, background=0.0)
    for m in (0, -3, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="min_size"):
            P.remove_small_components(y, m)
    for K in (0, 2.0, True):
        with pytest.raises(ValueError, match="num_classes"):
            P.keep_largest_component(y, K)
        with pytest.raises(ValueError, match="num_classes"):
            P.connected_components(y, num_classes=K)
        with pytest.raises(ValueError, match="num_classes"):
            P.remove_small_components(y, 2, num_classes=K)
    with pytest.raises(ValueError, match="num_classes"):
        P.keep_largest_component(y, None)


def test_cpu_tensors_are_refused_and_the_alias():
    import advchain.common.postprocess as P
    import advchain_amd.common.postprocess as P2
    from advchain_amd import ops
    from advchain_amd._lib import AdvchainHipError
    assert P is P2 and P.Components._fields == ("labels", "count", "sizes")
    assert ops.COMPONENTS_TILE == {2: (32, 64), 3: (4, 8, 64)}
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(AdvchainHipError):
        P.connected_components(y)
    with pytest.raises(AdvchainHipError):
        P.keep_largest_component(y, 2)
    with pytest.raises(AdvchainHipError):
        P.remove_small_components(y, 2)
