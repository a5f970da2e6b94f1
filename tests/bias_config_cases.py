"""AdvBias over its configuration space: the cases, their seeded inputs and the float64 reference the CPU and GPU tests share
(tests/test_bias_configs_cpu.py, tests/test_bias_configs_gpu.py).

CASES: name -> (spatial_dims, data_size, control_point_spacing, downscale, interpolation_order, space, seed), the smallest shapes
that reach a branch of the bias kernels no other test reaches with tables built by AdvBias: innermost bands of 1..7 (orders 0, 1,
2, 3, 5, 7), a control-point row of more than 64, rows that are no multiple of 4 or longer than 1024, images of one row and of
2 x 2, a 3D leading axis of 1, downscale 1 / 2 / 4, both spaces with N > 1 and C > 1.  EXPECT holds the (g, B) of each case's
band tables (with the trivial leading axis in 2D), obtained on the CPU; both test files assert them.

The reference is oracle.advchain_oracle.OracleBias in double: parameters and data in double and the B-spline window cast to
double AFTER BiasGeometry has rounded it to float32 (the reference's window is float32: that rounding is part of the definition).

The clip has a kink at |field - 1| = epsilon: a voxel within rounding distance of it takes the other branch in float32 and its
gradient differs by its whole value, which says nothing about a kernel.  The seed of a case is chosen so that, on the double
reference alone, every voxel is at least KINK_MARGIN from the kink and between 1 % and 60 % of the voxels are clipped
(`clip_stats`; tests/test_bias_configs_cpu.py asserts it for every case, in both modes).

Importing this module needs no GPU."""
import copy
import functools
import json

import torch

from oracle import advchain_oracle as O

EPSILON = 0.3
XI = 1e-6             # OracleBias.xi / AdvBias.xi: the power iteration evaluates the field at xi * param
KINK_MARGIN = 1e-5    # twice the 5e-6 bound on the field
CLIPPED_SHARE = (0.01, 0.60)

CASES = {
    # a control-point row of more than 64: tp_rows in several passes, reduced backward and dense reduction refused
    "2d_g68_o3":        (2, (2, 2, 12, 264), (8, 4), 2, 3, "log", 1),
    "2d_g68_o1_w262":   (2, (1, 1, 12, 262), (8, 4), 2, 1, "log", 0),
    "2d_w1028":         (2, (2, 1, 9, 1028), (4, 32), 2, 3, "log", 0),
    "3d_g68":           (3, (1, 2, 4, 6, 264), (4, 4, 4), 2, 3, "log", 0),
    # bands of 5, 6, 7 and 1: the run-time band loop
    "2d_o5_ds1":        (2, (2, 1, 40, 28), (7, 5), 1, 5, "log", 0),
    "2d_o7_ds1":        (2, (2, 1, 40, 28), (7, 5), 1, 7, "linear", 0),
    "2d_o5_b6_nc":      (2, (2, 2, 28, 40), (5, 7), 1, 5, "linear", 0),
    "2d_o0_ds4":        (2, (1, 3, 17, 64), (32, 32), 4, 0, "log", 0),
    "2d_odd_o3_log":    (2, (2, 2, 33, 47), (12, 10), 2, 3, "log", 1),
    "2d_odd_o1_linear": (2, (2, 2, 33, 47), (12, 10), 2, 1, "linear", 0),
    # spacing above the image
    "2d_o2_wide_sp":    (2, (2, 1, 9, 8), (16, 16), 2, 2, "log", 0),
    "2d_wide_sp_ds1":   (2, (2, 1, 64, 20), (64, 64), 1, 3, "log", 1),
    # edge shapes
    "2d_one_row":       (2, (1, 1, 1, 16), (4, 4), 1, 3, "log", 0),
    "2d_2x2":           (2, (2, 1, 2, 2), (2, 2), 2, 1, "log", 2),
    "2d_5x4":           (2, (1, 1, 5, 4), (4, 4), 1, 3, "linear", 0),
    # 3D
    "3d_odd_linear":    (3, (1, 1, 9, 11, 13), (5, 7, 3), 1, 3, "linear", 2),
    "3d_o1_nc":         (3, (2, 2, 12, 10, 8), (6, 4, 4), 2, 1, "log", 0),
    "3d_wide_sp":       (3, (1, 1, 5, 20, 33), (16, 16, 16), 1, 3, "log", 0),
    "3d_s0_1":          (3, (1, 1, 1, 8, 8), (2, 4, 4), 1, 3, "log", 0),
    "3d_o2_ds4":        (3, (1, 1, 16, 16, 8), (8, 8, 4), 4, 2, "log", 0),
}

# name -> (g, B) of AdvBias._tables (three axes; 2D has a trivial leading one)
EXPECT = {
    "2d_g68_o3": ((1, 4, 68), (1, 4, 3)),
    "2d_g68_o1_w262": ((1, 4, 68), (1, 2, 2)),
    "2d_w1028": ((1, 5, 35), (1, 3, 4)),
    "3d_g68": ((3, 4, 68), (3, 3, 3)),
    "2d_o5_ds1": ((1, 8, 8), (1, 6, 5)),
    "2d_o7_ds1": ((1, 8, 8), (1, 7, 7)),
    "2d_o5_b6_nc": ((1, 8, 8), (1, 5, 6)),
    "2d_o0_ds4": ((1, 3, 4), (1, 1, 2)),
    "2d_odd_o3_log": ((1, 5, 7), (1, 4, 4)),
    "2d_odd_o1_linear": ((1, 5, 7), (1, 2, 2)),
    "2d_o2_wide_sp": ((1, 3, 3), (1, 3, 3)),
    "2d_wide_sp_ds1": ((1, 3, 3), (1, 3, 3)),
    "2d_one_row": ((1, 3, 6), (1, 3, 4)),
    "2d_2x2": ((1, 3, 3), (1, 1, 1)),
    "2d_5x4": ((1, 4, 3), (1, 4, 3)),
    "3d_odd_linear": ((4, 4, 7), (4, 4, 3)),
    "3d_o1_nc": ((4, 5, 4), (2, 2, 2)),
    "3d_wide_sp": ((3, 4, 5), (3, 4, 4)),
    "3d_s0_1": ((3, 4, 4), (3, 4, 4)),
    "3d_o2_ds4": ((4, 4, 4), (3, 3, 2)),
}

LONG_ROW = ("2d_g68_o3", "2d_g68_o1_w262", "3d_g68")     # g2 = 68 > 64
G68, BAND7 = "2d_g68_o3", "2d_o7_ds1"                     # the tables of the kernel-level tests


def config(name):
    sd, size, spacing, downscale, order, space, _ = CASES[name]
    return dict(epsilon=EPSILON, control_point_spacing=list(spacing), downscale=downscale, data_size=list(size),
                interpolation_order=order, init_mode="identity", space=space)


@functools.lru_cache(maxsize=None)
def _oracle64(cfg_json, spatial_dims):
    """built once a configuration (the 2D window of spacing 64 is 643 x 643 and takes seconds) and only copied afterwards"""
    o = O.OracleBias(spatial_dims, json.loads(cfg_json))
    o.init_parameters()
    o.geom.window = o.geom.window.double()
    return o


def oracle64(cfg, spatial_dims, power_iteration=False):
    """OracleBias with its (float32-rounded) window in double: a shallow copy that shares the geometry, which nothing writes"""
    o = copy.copy(_oracle64(json.dumps(cfg, sort_keys=True), spatial_dims))
    o.power_iteration, o.is_training, o.param = bool(power_iteration), False, None
    return o


def reference64(cfg, spatial_dims, param, data, gout, power_iteration=False):
    """(field, out, grad_param, grad_data) of OracleBias in double, the gradients of (out * gout).sum() by autograd.
    power_iteration: the training forward of the power iteration, which evaluates the field at xi * param."""
    o = oracle64(cfg, spatial_dims, power_iteration)
    p = param.detach().cpu().double().requires_grad_(True)
    d = data.detach().cpu().double().requires_grad_(True)
    o.param = p
    o.is_training = bool(power_iteration)
    out = o.forward(d)
    (out * gout.detach().cpu().double()).sum().backward()
    return o.bias_field.detach(), out.detach(), p.grad, d.grad


@functools.lru_cache(maxsize=None)
def inputs(name, power_iteration=False):
    """Seeded (param, data, gout) on the CPU in float32: param = 0.5 * randn, data = rand + 0.5, gout = randn.
    power_iteration: param / xi, so that xi * param is the same field and the clip still has both branches."""
    sd, size, _, _, _, _, seed = CASES[name]
    cp_grid = O.BiasGeometry(list(size), list(CASES[name][2]), CASES[name][3], 0).cp_grid
    g = torch.Generator().manual_seed(seed)
    param = 0.5 * torch.randn(cp_grid, generator=g)
    data = torch.rand(size, generator=g) + 0.5
    gout = torch.randn(size, generator=g)
    if power_iteration:
        param = (param / XI).float()
    return param, data, gout


@functools.lru_cache(maxsize=None)
def reference(name, power_iteration=False):
    """reference64 of the case's inputs, computed once and shared: do not modify"""
    sd = CASES[name][0]
    return reference64(config(name), sd, *inputs(name, power_iteration), power_iteration=power_iteration)


def clip_stats(name, power_iteration=False):
    """(smallest distance of a voxel of the double reference's field from the kink, share of clipped voxels)"""
    o = oracle64(config(name), CASES[name][0])
    param = inputs(name, power_iteration)[0].double()
    dev = (o.compute_smoothed_bias((XI if power_iteration else 1.0) * param) - 1).abs()
    return float((dev - EPSILON).abs().min()), float((dev > EPSILON).double().mean())


def reduced_backward_accepts(tables):
    """what advchain_bias_field_bwd_reduced accepts on 16-byte aligned operands (it returns 0; -2 otherwise): rows of a
    multiple of 4 and at most 1024 voxels, at most 64 control points a row, a dense table of at most 4096 floats"""
    S2, g2, WB = int(tables.S[2]), int(tables.g[2]), int(tables.dense_inner[2])
    return S2 % 4 == 0 and S2 <= 1024 and g2 <= 64 and g2 * WB <= 4096


def figures_line(what, figures):
    """one line a case: the worst error per quantity and its bound"""
    return "%s: " % what + ", ".join("%s %.3g (bound %.3g)" % (k, e, b) for k, (e, b) in figures.items())


def errors(got, ref, power_iteration=False):
    """{quantity: (worst error, bound)} of (field, out, grad_param, grad_data) against reference64's.  The bounds are the
    project's for these quantities against the reference (test_bias_golden, test_bias_data_gradient).

    power_iteration: the gradient with respect to param is xi times the gradient with respect to xi * param, about 1e-5, and
    the bound 2e-5 * max(1, .) says little about it (tests/test_bias_rows_gpu.py::test_against_float64 keeps that bound at
    cp_scale = 1e-6 and so does grad_param here).  grad_param/xi is the same comparison with both sides divided by xi, the
    gradient with respect to xi * param: the very quantity the bound is for when the scale is 1."""
    err = lambda a, b: float((a.detach().cpu().double() - b).abs().max())      # noqa: E731
    field, out, gp, gd = got
    rfield, rout, rgp, rgd = ref
    fig = {"field": (err(field, rfield), 5e-6), "out": (err(out, rout), 5e-6),
           "grad_param": (err(gp, rgp), 2e-5 * max(1.0, float(rgp.abs().max()))), "grad_data": (err(gd, rgd), 1e-5)}
    if power_iteration:
        fig["grad_param/xi"] = (err(gp, rgp) / XI, 2e-5 * max(1.0, float(rgp.abs().max()) / XI))
    return fig


def check(what, got, ref, power_iteration=False):
    """print the case's line, then assert every bound, that everything is finite and that the gradients are not zero"""
    fig = errors(got, ref, power_iteration)
    print(figures_line(what, fig))
    assert all(bool(torch.isfinite(t).all()) for t in got), what
    assert float(got[2].abs().max()) > 0 and float(got[3].abs().max()) > 0, what
    for k, (e, b) in fig.items():
        assert e <= b, (what, k, e, b)
    return fig
