"""The brute-force form of tests/surface_dice_forms.py against the scipy formulation (binary_erosion, distance_transform_edt,
<= tau), and what common.metrics.surface_dice does on the host: its argument checks, the refusal of CPU tensors, the alias, the
threshold words and the route query of the library (no GPU)."""
import math
import struct

import numpy as np
import pytest
import torch

from tests.edt_forms import SAMPLING
from tests.surface_dice_forms import surface_dice_brute
from tests.surface_forms import label_pair


def _scipy_dice(ndi, pred, target, K, sampling, tau):
    N = pred.shape[0]
    within = np.zeros((N, K, 2), dtype=np.int64)
    counts = np.zeros((N, K, 2), dtype=np.int64)
    for n in range(N):
        for k in range(K):
            A, B = (pred[n] == k).numpy(), (target[n] == k).numpy()
            ea, eb = A ^ ndi.binary_erosion(A), B ^ ndi.binary_erosion(B)
            counts[n, k] = (ea.sum(), eb.sum())
            if not ea.any() or not eb.any():
                continue
            for d, (own, other) in enumerate(((ea, eb), (eb, ea))):
                within[n, k, d] = (ndi.distance_transform_edt(~other, sampling=sampling)[own] <= tau).sum()
    return within, counts


@pytest.mark.parametrize("K,shape", [(2, (2, 9, 13)), (4, (1, 20, 31)), (4, (1, 6, 10, 14)), (1, (1, 12, 9))])
@pytest.mark.parametrize("sampled", [False, True], ids=["unit", "sampling"])
def test_brute_force_form_is_the_scipy_formulation(K, shape, sampled):
    ndi = pytest.importorskip("scipy.ndimage")
    p, y = label_pair(K, shape, seed=K)
    s = SAMPLING[len(shape) - 1] if sampled else None
    # (with a sampling: tolerances that no distance of these spacings equals, so that scipy's roots cannot fall on the other side)
    for tau in (((1.6, 2.2, 3.1) if len(shape) == 3 else (0.7, 1.5, 2.2, 4.1)) if sampled else (0, 1, 1.5, 2, 3)):
        within, counts = _scipy_dice(ndi, p, y, K, s, tau)
        got = surface_dice_brute(p, y, K, tau, s)
        assert np.array_equal(got.surface_voxels.numpy(), counts)
        assert np.array_equal(got.within.numpy(), within), tau
        total = counts.sum(-1)
        want = np.where(total > 0, within.sum(-1) / np.maximum(total, 1), np.nan)
        np.testing.assert_array_equal(got.surface_dice.numpy(), want)
        assert (within <= counts).all()
    assert within.sum() > 0


def test_host_side_checks_raise_value_errors():
    import advchain.common.metrics as M
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="3-D"):
        M.surface_dice(torch.zeros(8, 8, dtype=torch.int64), torch.zeros(8, 8, dtype=torch.int64), 2, 1.0)
    with pytest.raises(ValueError, match="shape"):
        M.surface_dice(y, torch.zeros(2, 8, 9, dtype=torch.int64), 2, 1.0)
    with pytest.raises(ValueError, match="num_classes"):
        M.surface_dice(y, y, 0, 1.0)
    with pytest.raises(ValueError, match="sampling"):
        M.surface_dice(y, y, 2, 1.0, sampling=(1.0,))
    for bad in (True, "1", float("nan"), float("inf"), -0.5, None, [1.0], (1.0, 2.0, 3.0), [1.0, -1.0], [1.0, True], [1.0, float("nan")],
                torch.tensor([1.0, 2.0, 3.0]), torch.tensor(1.0), torch.tensor([[1.0, 2.0]])):
        with pytest.raises(ValueError, match="tolerance"):
            M.surface_dice(y, y, 2, bad)


def test_numpy_scalars_and_arrays_are_tolerances():
    from advchain_amd import ops
    f = ops.surface_dice_tolerances
    assert f("surface_dice", np.float32(1.5), 2) == (1.5, 1.5) and f("surface_dice", np.int64(2), 2) == (2.0, 2.0)
    assert f("surface_dice", np.array([1.0, 2.5], dtype=np.float32), 2) == (1.0, 2.5)
    assert f("surface_dice", [np.float64(1.0), np.int32(3)], 2) == (1.0, 3.0)
    assert f("surface_dice", torch.tensor([1, 2]), 2) == (1.0, 2.0)
    for bad in (np.bool_(True), np.array([True, False]), np.array(1.0), np.array([[1.0, 2.0]]), torch.tensor([True, False]),
                np.array([1.0, np.nan]), 1 + 0j):
        with pytest.raises(ValueError, match="tolerance must be one finite real number"):
            f("surface_dice", bad, 2)
    assert ops.surface_dice_threshold_words(f("surface_dice", np.float32(2), 3), True) == (4, 4, 4)


def test_cpu_tensors_are_refused():
    import advchain.common.metrics as M
    from advchain_amd._lib import AdvchainHipError
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    for tol in (1.0, 2, [1.0, 2.0], (0, 3), torch.tensor([1.0, 2.0])):
        with pytest.raises(AdvchainHipError):
            M.surface_dice(y, y, 2, tol)


def test_alias_and_the_namedtuple():
    import advchain.common.metrics as M
    import advchain_amd.common.metrics as M2
    from advchain_amd import ops
    assert M is M2 and M.SurfaceDice is ops.SurfaceDice
    assert M.SurfaceDice._fields == ("surface_dice", "within", "surface_voxels")
    assert ops.SURFACE_DICE_TILE == {2: (32, 64), 3: (8, 8, 32)}


def test_threshold_words():
    from advchain_amd import ops
    tol = ops.surface_dice_tolerances("surface_dice", (2, 1.5, math.sqrt(3), 1e9), 4)
    assert ops.surface_dice_threshold_words(tol, True) == (4, 2, 2, 2 ** 30 - 1)
    assert ops.surface_dice_tolerances("surface_dice", 2, 3) == (2.0, 2.0, 2.0)
    bits = ops.surface_dice_threshold_words((1.4, 0.0, 1e200), False)
    want = tuple(struct.unpack("<I", struct.pack("<f", v))[0] for v in (1.4 * 1.4, 0.0, 1.0e29))
    assert bits == want and bits[0] == int(np.float32(1.4 * 1.4).view(np.uint32))


def test_route_query():
    from advchain_amd import ops
    assert ops.surface_dice_route(3, 4, (36, 57), 2) == "ball"
    assert ops.surface_dice_route(2, 4, (6, 10, 70), 1.5, (2.5, 1.0, 0.8)) == "ball"
    assert ops.surface_dice_route(1, 20, (70, 130), (1.0,) * 19 + (3.0,)) == "ball"
    assert ops.surface_dice_route(1, 20, (70, 130), 40) == "fields"
    # the dispatch limits: caps up to 5 in 2D and 2 in 3D go to the ball, larger ones to the fields while they can take the shape
    assert ops.surface_dice_route(1, 20, (70, 130), 5.9) == "ball" and ops.surface_dice_route(1, 20, (70, 130), 6) == "fields"
    assert ops.surface_dice_route(1, 4, (16, 40, 40), 2.9) == "ball" and ops.surface_dice_route(1, 4, (16, 40, 40), 3) == "fields"
    assert ops.surface_dice_route(1, 4, (16, 40, 40), 3, route="ball") == "ball"
    assert ops.surface_dice_route(1, 4, (16, 40, 40), 3, (2.0, 1.0, 1.5)) == "fields"                 # caps 1, 3, 2
    assert ops.surface_dice_route(1, 4, (16, 40, 40), 2.9, (2.0, 1.0, 1.5)) == "ball"                 # caps 1, 2, 1
    assert ops.surface_dice_route(1, 20, (70, 130), (1.0,) * 19 + (40.0,)) == "fields"
    assert ops.surface_dice_route(1, 20, (70, 130), 2, route="fields") == "fields"
    with pytest.raises(NotImplementedError, match="ball"):
        ops.surface_dice_route(1, 20, (70, 130), 40, route="ball")
    # a tolerance beyond the image needs no more than the image: the cap stops at the axis
    assert ops.surface_dice_route(1, 2, (5, 7), 1e9, route="ball") == "ball"
    # a row that the distance fields refuse: the ball takes it where it can, nothing does otherwise
    assert ops.surface_dice_route(1, 2, (2, 40000), 3) == "ball"
    with pytest.raises(NotImplementedError, match="distance fields"):
        ops.surface_dice_route(1, 2, (2, 40000), 1000)
    # more classes than the two halves of a staged word hold
    assert ops.surface_dice_route(1, 65535, (8, 8), 1) == "fields"
    with pytest.raises(ValueError, match="tolerance"):
        ops.surface_dice_route(1, 2, (8, 8), -1)
    with pytest.raises(ValueError, match="route"):
        ops.surface_dice_route(1, 2, (8, 8), 1, route="edt")


def test_the_c_entries_check_their_arguments_on_the_host():
    from advchain_amd import _lib
    lib = _lib.load()
    dims = _lib.dims_array((36, 57))
    V, N, K = 36 * 57, 3, 4
    assert lib.advchain_surface_dice_workspace(N, K, 2, dims, None, 2.0, 0) == 0
    assert lib.advchain_surface_dice_workspace(N, K, 2, dims, None, 2.0, 2) == 2 * N * K * V + 4 * N * V + 6 * N * K
    assert lib.advchain_surface_dice_workspace(N, K, 2, _lib.dims_array((70, 130)), None, 40.0, 1) == -1
    assert lib.advchain_surface_dice_workspace(0, K, 2, dims, None, 2.0, 0) == -1
    assert lib.advchain_surface_dice_route(N, K, 2, dims, None, 2.0, 0) == 1
    assert lib.advchain_surface_dice_route(N, K, 2, dims, None, 2.0, 7) == -1 and b"surface_dice" in lib.advchain_last_error()
    assert lib.advchain_surface_dice_route(N, K, 2, dims, _lib.float_array([1.0, -1.0]), 2.0, 0) == -1
    assert b"surface_dice" in lib.advchain_last_error() and b"sampling" in lib.advchain_last_error()
    assert lib.advchain_surface_dice_route(N, K, 2, dims, None, float("nan"), 0) == -1 and b"tolerance" in lib.advchain_last_error()
    rc = lib.advchain_surface_dice(None, None, None, None, 2.0, 0, None, None, None, None, N, K, 2, dims, None)
    assert rc < 0 and b"surface_dice" in lib.advchain_last_error()
