"""The case list of tests/bias_config_cases.py holds what it promises, and the product's host side (AdvBias with its band
tables, on the test-only dense backend tests/cpu_backend.py) agrees with OracleBias in double on every case, within the
bounds the GPU tests use (tests/test_bias_configs_gpu.py).  No GPU."""
import pytest
import torch

from oracle import advchain_oracle as O
from tests import bias_config_cases as K
from tests import cpu_backend

CPU = torch.device("cpu")
NAMES = list(K.CASES)


def _product(name, power_iteration=False):
    from advchain_amd.augmentor import AdvBias
    t = AdvBias(K.CASES[name][0], K.config(name), power_iteration=power_iteration, device=CPU)
    t.init_parameters()
    return t


def test_the_list_covers_what_it_claims():
    from advchain_amd import bands
    assert set(K.EXPECT) == set(K.CASES) and 18 <= len(K.CASES) <= 22
    inner = {K.EXPECT[n][1][2] for n in NAMES}
    assert set(range(1, 8)) <= inner and max(inner) <= bands.BAND_MAX, inner
    third = (len(NAMES) + 2) // 3
    assert sum(K.CASES[n][1][0] == 2 for n in NAMES) >= third                  # a batch
    assert sum(K.CASES[n][1][1] >= 2 for n in NAMES) >= third                  # channels
    assert {K.CASES[n][5] for n in NAMES} == {"log", "linear"}
    assert {K.CASES[n][3] for n in NAMES} == {1, 2, 4}
    assert {K.CASES[n][4] for n in NAMES} >= {0, 1, 2, 3, 5, 7}
    assert any(K.CASES[n][5] == "linear" and K.CASES[n][1][0] > 1 and K.CASES[n][1][1] > 1 for n in NAMES)
    for n in K.LONG_ROW:
        assert K.EXPECT[n][0][2] > 64, n
    widths = {K.CASES[n][1][-1] for n in NAMES}
    assert any(w % 4 for w in widths) and any(w > 1024 for w in widths)        # one voxel a thread; no dense reduction
    assert any(K.CASES[n][1][2:] == (1, 16) for n in NAMES) and any(K.CASES[n][1][2:] == (2, 2) for n in NAMES)
    assert any(K.CASES[n][0] == 3 and K.CASES[n][1][2] == 1 for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_clip_condition(name):
    """both modes: the power iteration's parameters are param / xi rounded to float32, a field of its own"""
    for pi in (False, True):
        dist, share = K.clip_stats(name, pi)
        print("%s pi=%d: distance from the kink %.3g, clipped share %.3f" % (name, pi, dist, share))
        assert dist >= K.KINK_MARGIN, (name, pi, dist)
        assert K.CLIPPED_SHARE[0] <= share <= K.CLIPPED_SHARE[1], (name, pi, share)


@pytest.mark.parametrize("name", NAMES)
def test_geometry_and_tables(name):
    t = _product(name)
    sd, size, spacing, downscale, order, _, _ = K.CASES[name]
    geom = O.BiasGeometry(list(size), list(spacing), downscale, order)
    assert list(t.param.shape) == geom.cp_grid
    assert t._crop_start.tolist() == geom.crop_start.tolist() and t._crop_end.tolist() == geom.crop_end.tolist()
    assert t._stride == geom.stride
    tb = t._tables
    assert (tuple(tb.g), tuple(tb.B)) == K.EXPECT[name], (name, tb.g, tb.B)
    assert tuple(tb.S[3 - sd:]) == tuple(size[2:]) and tuple(K.inputs(name)[0].shape) == tuple(t.param.shape)


@pytest.mark.parametrize("power_iteration", [False, True], ids=["eval", "power_iteration"])
@pytest.mark.parametrize("name", NAMES)
def test_host_parity(name, power_iteration, monkeypatch):
    cpu_backend.install(monkeypatch)
    t = _product(name, power_iteration)
    param, data, gout = K.inputs(name, power_iteration)
    if power_iteration:
        t.train()
    p, d = param.clone().requires_grad_(True), data.clone().requires_grad_(True)
    t.param = p
    out = t.forward(d)
    (out * gout).sum().backward()
    K.check("%s %s" % (name, "power_iteration" if power_iteration else "eval"), (t.bias_field, out, p.grad, d.grad),
            K.reference(name, power_iteration), power_iteration)
    # the field the class computes on its own from the parameters (no forward before): in eval only, it has no cp_scale
    if not power_iteration:
        t.bias_field = None
        ref = K.reference(name)[0][:, :1]
        assert float((t.bias_field.double() - ref).abs().max()) <= 5e-6


def _cfg(size, spacing, downscale, order):
    return dict(epsilon=0.3, control_point_spacing=list(spacing), downscale=downscale, data_size=list(size),
                interpolation_order=order, init_mode="identity", space="log")


def test_a_band_above_the_limit_is_refused_at_table_construction():
    from advchain_amd.augmentor import AdvBias
    t = AdvBias(2, _cfg((1, 1, 40, 28), (6, 6), 1, 9), device=CPU)
    with pytest.raises(NotImplementedError, match="exceeds the kernel limit"):
        t.init_parameters()


@pytest.mark.parametrize("order", [0, 2])
def test_a_field_that_misses_the_image_size_is_refused_before_any_launch(order):
    """downscale 1 with an even-length window: conv_transpose and crop give 33 x 33 for a 32 x 32 image and nothing resamples it.
    The oracle's forward fails at `field * data`; the product refuses when it builds its tables."""
    from advchain_amd.augmentor import AdvBias
    cfg = _cfg((1, 1, 32, 32), (16, 16), 1, order)
    o = O.OracleBias(2, cfg)
    o.init_parameters()
    assert tuple(o.bias_field.shape[2:]) == (33, 33)
    with pytest.raises(RuntimeError):
        o.forward(torch.ones(1, 1, 32, 32))
    t = AdvBias(2, cfg, device=CPU)
    with pytest.raises(NotImplementedError, match="larger than the image"):
        t.init_parameters()
