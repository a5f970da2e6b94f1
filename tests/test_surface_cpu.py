"""The brute-force forms of tests/surface_forms.py against the scipy formulation (binary_erosion, distance_transform_edt,
numpy.percentile), and what common.metrics does on the host: its argument checks, the refusal of CPU tensors and the alias."""
import numpy as np
import pytest
import torch

from tests.edt_forms import SAMPLING
from tests.surface_forms import border, label_pair, surface_brute


def _scipy_metrics(pred, target, K, sampling, q):
    ndi = pytest.importorskip("scipy.ndimage")
    N = pred.shape[0]
    out = np.zeros((N, K, 2, 3))
    counts = np.zeros((N, K, 2), dtype=np.int64)
    for n in range(N):
        for k in range(K):
            A, B = (pred[n] == k).numpy(), (target[n] == k).numpy()
            ea, eb = A ^ ndi.binary_erosion(A), B ^ ndi.binary_erosion(B)
            counts[n, k] = (ea.sum(), eb.sum())
            if not ea.any() or not eb.any():
                out[n, k] = np.nan if not ea.any() and not eb.any() else np.inf
                continue
            for d, (own, other) in enumerate(((ea, eb), (eb, ea))):
                dist = ndi.distance_transform_edt(~other, sampling=sampling)[own]
                out[n, k, d] = (dist.max(), np.percentile(dist, q), dist.mean())
    return out, counts


@pytest.mark.parametrize("K,shape", [(2, (2, 9, 13)), (4, (1, 20, 31)), (4, (1, 6, 10, 14)), (1, (1, 12, 9))])
@pytest.mark.parametrize("sampled", [False, True], ids=["unit", "sampling"])
def test_brute_force_form_is_the_scipy_formulation(K, shape, sampled):
    p, y = label_pair(K, shape, seed=K)
    s = SAMPLING[len(shape) - 1] if sampled else None
    for q in (95.0, 37.5):
        want, counts = _scipy_metrics(p, y, K, s, q)
        got = surface_brute(p, y, K, s, q)
        assert np.array_equal(got.surface_voxels.numpy(), counts)
        g = got.directed.numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want)) and np.array_equal(np.isinf(g), np.isinf(want))
        ok = np.isfinite(want)
        assert ok.any()
        np.testing.assert_allclose(g[ok], want[ok], rtol=1e-14, atol=0)
        fin = ok.all((-1, -2))
        np.testing.assert_allclose(got.hausdorff.numpy()[fin], want[..., 0].max(-1)[fin], rtol=1e-14)
        np.testing.assert_allclose(got.hausdorff_percentile.numpy()[fin], want[..., 1].max(-1)[fin], rtol=1e-14)


def test_border_is_the_set_minus_its_erosion():
    m = torch.zeros(7, 9, dtype=torch.bool)
    m[1:6, 2:8] = True
    e = border(m)
    assert int(e.sum()) == 5 * 6 - 3 * 4 and not bool(e[2:5, 3:7].any())
    full = torch.ones(4, 5, dtype=torch.bool)                 # a position outside the image is outside the set
    assert int(border(full).sum()) == 4 * 5 - 2 * 3
    cube = torch.ones(3, 3, 3, dtype=torch.bool)
    assert int(border(cube).sum()) == 26


def test_host_side_checks_raise_value_errors():
    import advchain.common.metrics as M
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    for fn in (M.surface_distance_metrics, M.hausdorff_distance, M.average_surface_distance):
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros(8, 8, dtype=torch.int64), torch.zeros(8, 8, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="3-D"):
            fn(y, [[0]], 2)
        with pytest.raises(ValueError, match="shape"):
            fn(y, torch.zeros(2, 8, 9, dtype=torch.int64), 2)
        with pytest.raises(ValueError, match="num_classes"):
            fn(y, y, 0)
        with pytest.raises(ValueError, match="num_classes"):
            fn(y, y, 2.0)
        with pytest.raises(ValueError, match="sampling"):
            fn(y, y, 2, sampling=(1.0,))
        with pytest.raises(ValueError, match="sampling"):
            fn(y, y, 2, sampling=(1.0, -1.0))
    for fn in (M.surface_distance_metrics, M.hausdorff_distance):
        for q in (-1.0, 100.5, float("nan"), float("inf"), "95", True):
            with pytest.raises(ValueError, match="percentile"):
                fn(y, y, 2, percentile=q)
    with pytest.raises(ValueError, match="percentile"):
        M.surface_distance_metrics(y, y, 2, percentile=None)


def test_cpu_tensors_are_refused():
    import advchain.common.metrics as M
    from advchain_amd._lib import AdvchainHipError
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    for fn in (M.surface_distance_metrics, M.hausdorff_distance, M.average_surface_distance):
        with pytest.raises(AdvchainHipError):
            fn(y, y, 2)


def test_alias_and_the_workspace_query():
    import advchain.common.metrics as M
    import advchain_amd.common.metrics as M2
    from advchain_amd import _lib
    assert M is M2 and M.SurfaceMetrics._fields == ("hausdorff", "hausdorff_percentile", "assd", "directed", "surface_voxels",
                                                    "max_squared", "overlap", "dice")
    lib = _lib.load()
    dims = _lib.dims_array((36, 57))
    V, N, K = 36 * 57, 3, 4
    assert lib.advchain_surface_metrics_workspace(N, K, 2, dims) == 2 * N * K * V + 4 * N * V + 2 * N * K * (512 + 2 + 2 * 1 + 4)
    assert lib.advchain_surface_metrics_workspace(1, 1, 2, _lib.dims_array((2, 40000))) == -1
    assert lib.advchain_surface_metrics_workspace(1, 1, 2, _lib.dims_array((9000, 4))) == -1     # the limit of the signed maps
    assert lib.advchain_surface_metrics_workspace(0, 1, 2, dims) == -1
    rc = lib.advchain_surface_metrics(None, None, None, 95.0, None, None, None, None, None, None, None, None, None, 1, 1, 2, dims, None)
    assert rc < 0 and b"surface_metrics" in lib.advchain_last_error()
