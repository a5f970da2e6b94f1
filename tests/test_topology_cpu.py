"""The reference form of tests/topology_forms.py on hand shapes whose Betti numbers are known, the identities that tie its parts
together on random masks, the class-0 and out-of-range label rules, and what betti_numbers / betti_error and the C ABI do on the
host: every ValueError, the refusal of a CPU tensor, the workspace query and the argument checks.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from tests import topology_forms as T


HANDS = T.HAND_2D + T.HAND_3D


@pytest.mark.parametrize("name,mask,at_one,at_full", HANDS, ids=[h[0] + " %dd" % h[1].ndim for h in HANDS])
def test_hand_shapes(name, mask, at_one, at_full):
    assert T.betti_of_mask(mask, 1)[0] == at_one
    assert T.betti_of_mask(mask, mask.ndim)[0] == at_full
    if name == "all one":
        assert T.betti_of_mask(mask, 1)[1] == 1 and T.betti_of_mask(mask, mask.ndim)[1] == 1
    # the same shape inside a larger array of zeros: nothing depends on where the array ends
    padded = np.pad(mask, 2)
    assert T.betti_of_mask(padded, 1)[0] == at_one and T.betti_of_mask(padded, mask.ndim)[0] == at_full


def test_the_empty_set_has_zeros():
    for shape in ((3, 4), (1, 1), (2, 3, 4), (1, 1, 5)):
        for c in T.valid_connectivities(len(shape)):
            assert T.betti_of_mask(np.zeros(shape, dtype=bool), c) == ((0, 0, 0), 0)


def test_2d_loops_are_the_bounded_components_of_the_complement():
    """b0 - chi against scipy's count of the holes: Euler-Poincare for the pairs (4, 8) and (8, 4)."""
    seen = 0
    for mask in T.random_masks((13, 13), 300, seed=0):
        for c in (1, 2):
            (b0, b1, b2), chi = T.betti_of_mask(mask, c)
            assert b1 == T.bounded_complement_form(mask, c) and b2 == 0, (mask.astype(int).tolist(), c)
            seen = max(seen, b1)
    assert seen >= 2


def test_3d_loops_are_never_negative():
    most = [0, 0, 0]
    for mask in T.random_masks((7, 7, 7), 200, seed=1, densities=(0.3, 0.5, 0.7, 0.85)):
        for c in (1, 3):
            b, chi = T.betti_of_mask(mask, c)
            assert min(b) >= 0 and chi == b[0] - b[1] + b[2], (mask.astype(int).tolist(), c)
            most = [max(m, v) for m, v in zip(most, b)]
    assert min(most) >= 2, most


def test_class_zero_is_a_class_and_labels_out_of_range_are_in_none():
    ring = T.embedded((1, 7, 8), T.RING_3X3, (2, 2))
    betti, euler = T.betti_form(ring, 2, 1)
    assert betti[0].tolist() == [[2, 1, 0], [1, 1, 0]]      # class 0: the outside and the centre, with the ring as its hole
    assert euler[0].tolist() == [1, 0]
    marked = ring.clone()
    marked[0, 3, 3] = -100                                   # the centre leaves class 0 and stays in the complement of class 1
    marked[0, 0, 0] = 5
    betti, euler = T.betti_form(marked, 2, 1)
    assert betti[0].tolist() == [[1, 1, 0], [1, 1, 0]]
    betti, euler = T.betti_form(marked, 6, 1)                # K = 6: label 5 is a class now, -100 never is
    assert betti[0, 5].tolist() == [1, 0, 0] and betti[0, 2:5].abs().sum() == 0 and euler[0, 5] == 1
    error, total, both, chis = T.error_form(ring, marked, 2, 1)
    assert error[0].tolist() == [[1, 0, 0], [0, 0, 0]] and total[0].tolist() == [1, 0]
    assert both.shape == (1, 2, 2, 3) and chis.shape == (1, 2, 2) and both[0, 0, 0].tolist() == [2, 1, 0]


def test_every_value_error_comes_before_any_gpu_work():
    import advchain.common.metrics as M
    y = torch.zeros(1, 5, 7, dtype=torch.int64)
    y3 = torch.zeros(1, 3, 5, 7, dtype=torch.int64)
    calls = (lambda x, *a, **k: M.betti_numbers(x, *a, **k), lambda x, *a, **k: M.betti_error(x, x, *a, **k))
    for call in calls:
        with pytest.raises(ValueError, match="labels"):
            call(torch.zeros(5, 7, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="labels"):
            call(torch.zeros(1, 1, 2, 5, 7, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="labels"):
            call([[0]], 2)
        with pytest.raises(ValueError, match="empty"):
            call(torch.zeros(1, 0, 7, dtype=torch.int64), 2)
        for bad in (0, -1, True, 2.0, None):
            with pytest.raises(ValueError, match="num_classes"):
                call(y, bad)
        with pytest.raises(NotImplementedError):
            call(y, 65536)
        for bad in (0, 3, True, 1.0, "1", None):
            with pytest.raises(ValueError, match="connectivity"):
                call(y, 2, connectivity=bad)
        for bad in (0, 4, False, 3.0):
            with pytest.raises(ValueError, match="connectivity"):
                call(y3, 2, connectivity=bad)
        with pytest.raises(ValueError, match="18-adjacency"):
            call(y3, 2, connectivity=2)
        with pytest.raises(M.ops._lib.AdvchainHipError):     # valid arguments: only the device is missing
            call(y, 2)
        with pytest.raises(M.ops._lib.AdvchainHipError):
            call(y3, 2, connectivity=3)
    with pytest.raises(ValueError, match="differ in shape"):
        M.betti_error(y, torch.zeros(1, 5, 8, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="target"):
        M.betti_error(y, None, 2)
    assert M.Betti is M.ops.Betti and M.Betti._fields == ("betti", "euler")
    assert M.BettiError is M.ops.BettiError and M.BettiError._fields == ("error", "total", "betti", "euler")


def test_the_workspace_query_and_the_argument_checks_of_the_c_abi_run_on_the_host():
    import ctypes
    from advchain_amd import _lib
    lib = _lib.load()
    for N, sp in ((2, (5, 7)), (32, (256, 256)), (4, (128, 128, 64)), (1, (9, 17, 129))):
        d = _lib.dims_array(sp)                              # one labelling, whatever the class count is
        assert lib.advchain_betti_workspace(N, len(sp), d) == lib.advchain_components_workspace(N, len(sp), d) > 0
    assert lib.advchain_betti_workspace(1, 3, _lib.dims_array((2048, 1024, 1024))) == -1
    assert lib.advchain_betti_workspace(0, 2, _lib.dims_array((8, 8))) == -1
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    def call(K=2, connectivity=1, pred=p, target=p, error=p, betti=p, nd=2, sp=(2, 2), N=1):
        return lib.advchain_betti(pred, target, betti, p, error, p, N, K, nd, _lib.dims_array(sp), connectivity, None)

    for kwargs, word in ((dict(K=0), b"K must be"), (dict(K=65536), b"K must be"), (dict(connectivity=0), b"connectivity"),
                         (dict(connectivity=3), b"connectivity"), (dict(pred=None), b"null pointer"),
                         (dict(betti=None), b"null pointer"), (dict(target=None), b"needs a target"),
                         (dict(betti=odd), b"aligned"), (dict(nd=3, sp=(2, 2, 2), connectivity=2), b"18-adjacency"),
                         (dict(nd=3, sp=(2, 2, 2), connectivity=4), b"connectivity"), (dict(N=0), b"bad N")):
        assert call(**kwargs) == -1 and word in lib.advchain_last_error(), (kwargs, lib.advchain_last_error())
    assert call(nd=3, sp=(2048, 1024, 1024)) == -2 and b"2^31" in lib.advchain_last_error()
