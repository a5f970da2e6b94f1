"""distance_transform_edt / signed_distance_maps / boundary_loss of common.loss without a GPU: the public names and signatures,
the brute-force forms of tests/edt_forms.py against scipy, against plain loops and against autograd (the formulas the kernels
implement), what fp32 arithmetic reaches at the cases of tests/test_boundary_gpu.py, the host-side argument checks of the Python
layer and of the C entries, and no CPU path.  For the edge cases of tests/test_edt_edges_gpu.py: that each takes the dispatch
branch it is listed for (by edt_plan, the plain-Python mirror of the host loops of csrc/edt.hip), that together the cases run
every tile width, that no pattern leaves a trivial answer, what fp32 reaches there, and where the entries stop accepting."""
import ctypes
import inspect
import warnings

import pytest
import torch

from tests.edt_forms import (EDGE_EDT_CASES, EDGE_EDT_LIMITS, EDGE_MAP_CASES, EDGE_MAP_LIMITS, EDGE_SURFACE_CASES, EDT_PATTERNS,
                             EDT_SHAPES, LOSS_SHAPES, MAP_CASES, SAMPLING, SAMPLING_TOL, boundary_closed, boundary_gradient,
                             boundary_loop, boundary_scale, edge_case_id, edge_edt_reference, edge_label_case, edge_surface_pair,
                             edt_axis_passes, edt_brute, edt_case_plan, edt_plan, gate_of, label_case, loss_case, loss_weights,
                             mask_pattern, omega_of, signed_maps_brute)

E = inspect.Parameter.empty


@pytest.mark.parametrize("pkg", ["advchain.common.loss", "advchain_amd.common.loss"])
def test_public_names_and_signatures(pkg):
    import importlib
    mod = importlib.import_module(pkg)

    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]

    assert params(mod.distance_transform_edt) == [("mask", E), ("sampling", None), ("squared", False)]
    assert params(mod.signed_distance_maps) == [("target", E), ("num_classes", E), ("sampling", None)]
    assert params(mod.boundary_loss) == [("input", E), ("target", None), ("weight", None), ("ignore_background", True),
                                         ("sampling", None), ("dist_maps", None)]


@pytest.mark.parametrize("sampling", [False, True], ids=["unit", "sampling"])
@pytest.mark.parametrize("shape", [(2, 9, 13), (2, 5, 7, 6)], ids=["2d", "3d"])
def test_brute_force_transform_is_scipys(shape, sampling):
    ndi = pytest.importorskip("scipy.ndimage")
    s = SAMPLING[len(shape) - 1] if sampling else None
    for name in ("fg05", "fg95", "corner", "half", "checker", "sparse"):
        m = mask_pattern(shape, name, seed=3)
        m.reshape(shape[0], -1)[:, 0] = False                    # at least one zero per entry: scipy's value is defined
        got = edt_brute(m, s)
        for b in range(shape[0]):
            want = torch.from_numpy(ndi.distance_transform_edt(m[b].numpy(), sampling=s))
            assert float((got[b] - want).abs().max()) <= 1e-12, (name, b)
        sq = edt_brute(m, s, squared=True)
        assert float((sq - got * got).abs().max()) <= 1e-9
    full = torch.ones(shape, dtype=torch.bool)
    assert bool(torch.isinf(edt_brute(full, s)).all())


def _maps_and_case(shape, seed=0):
    x, y = loss_case(shape, seed)
    return x.double(), y, signed_maps_brute(y, shape[1])


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (2, 3, 3, 4, 5), (1, 1, 4, 4)], ids=["2d", "3d", "one_class"])
def test_closed_form_agrees_with_plain_loops(shape):
    x, y, maps = _maps_and_case(shape)
    K = shape[1]
    for ign in ((False,) if K == 1 else (False, True)):
        for w in (None, loss_weights(K)):
            for tgt in (y, None):
                a = float(boundary_closed(x, tgt, weight=w, ignore_background=ign, dist_maps=maps))
                b = boundary_loop(x, maps, tgt, weight=w, ignore_background=ign)
                assert abs(a - b) <= 1e-12, (ign, w, a, b)
    if K > 1:
        assert float(boundary_closed(x, y)) == float(boundary_closed(x, y, dist_maps=maps))
        yb = y.clone()
        yb[0].reshape(-1)[2] = K
        assert torch.isnan(boundary_closed(x, yb, dist_maps=maps)) and boundary_loop(x, maps, yb) != boundary_loop(x, maps, yb)


@pytest.mark.parametrize("shape", [(2, 4, 5, 7), (2, 3, 3, 4, 5)], ids=["2d", "3d"])
def test_gradient_formula_agrees_with_autograd(shape):
    x, y, maps = _maps_and_case(shape, seed=1)
    K = shape[1]
    for ign in (False, True):
        for w in (None, loss_weights(K)):
            for tgt in (y, None):
                xr = x.clone().requires_grad_(True)
                (g,) = torch.autograd.grad(boundary_closed(xr, tgt, weight=w, ignore_background=ign, dist_maps=maps), xr)
                want = boundary_gradient(x, maps, gate_of(x, tgt), omega_of(K, w, ign, x.dtype))
                assert float((g - want).abs().max()) <= 1e-14, (ign, w)
                if tgt is not None:
                    assert float(g.movedim(1, -1)[tgt == -100].abs().max()) == 0.0


def test_degenerate_planes_are_zero_and_signs():
    for K, shape in ((1, (3, 5, 7)), (4, (3, 6, 5, 4))):
        y = label_case(K, shape, seed=5)
        maps = signed_maps_brute(y, K)
        assert float(maps[-1].abs().max()) == 0.0                  # class 0 fills the last entry, the others are absent from it
        if K == 1:
            assert float(maps[1].abs().max()) == 0.0               # the class is absent (every voxel -100)
        else:
            assert float(maps[:, K - 1].abs().max()) == 0.0        # absent everywhere
        for k in range(K):
            inside = y[0] == k
            if bool(inside.any()) and not bool(inside.all()):
                assert float(maps[0, k][inside].max()) <= -1.0 and float(maps[0, k][~inside].min()) >= 1.0


def _fp32_sampling_error(shape, name):
    s = SAMPLING[len(shape) - 1]
    m = mask_pattern(shape, name, seed=len(shape))
    want = edt_brute(m, s)
    got = edt_brute(m, s, dtype=torch.float32)
    fin = torch.isfinite(want) & (want > 0)
    assert torch.equal(torch.isfinite(got), torch.isfinite(want))
    return float(((got - want).abs()[fin] / want[fin]).max()) if bool(fin.any()) else 0.0


@pytest.mark.parametrize("shape", EDT_SHAPES, ids=["x".join(map(str, s)) for s in EDT_SHAPES])
def test_fp32_stays_a_factor_of_ten_inside_the_sampling_bound_of_the_gpu_test(shape):
    """|S (v - u)| evaluated in fp32 straight from its definition (products, squares, sums, root: one rounding each) against
    float64, at the GPU test's shapes, patterns and samplings, stays a factor of ten inside SAMPLING_TOL.  That bound is widened
    from 1e-6 to 2e-6 relative: the fp32 evaluation itself reaches 1.34e-7 at 3x36x57, 1.49e-7 at 1x70x130 and 1.44e-7 at
    2x6x10x70, because besides the roundings of the squared sum and the root's each s * delta is rounded before it is squared.
    Worst case by the roundings: (3 + 2) 2^-24 on the squared sum, half of it after the root, plus the root's own half ulp =
    2.1e-7; ten times that is the bound."""
    worst = max(_fp32_sampling_error(shape, name) for name in EDT_PATTERNS)
    print("fp32 sampling error at %s: %.3g" % (shape, worst))
    assert worst <= SAMPLING_TOL / 10


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["x".join(map(str, s)) for s in LOSS_SHAPES])
def test_fp32_closed_form_stays_a_factor_of_ten_inside_the_gpu_bounds(shape):
    """Value within 2e-6 max(|want|, S) and gradient within 1e-6 of the largest |expected|: a tenth of the GPU test's bounds."""
    K = shape[1]
    x, y = loss_case(shape, seed=K)
    maps = signed_maps_brute(y, K)
    for ign in ((False,) if K == 1 else (False, True)):
        for w in (None, loss_weights(K)):
            for tgt in (y, None):
                opt = dict(weight=w, ignore_background=ign, dist_maps=maps)
                x64 = x.double().requires_grad_(True)
                x32 = x.clone().requires_grad_(True)
                v64 = boundary_closed(x64, tgt, **opt)
                v32 = boundary_closed(x32, tgt, **opt)
                (g64,), (g32,) = torch.autograd.grad(v64, x64), torch.autograd.grad(v32, x32)
                S = boundary_scale(x.double(), tgt, weight=w, ignore_background=ign, dist_maps=maps)
                err = abs(float(v32.detach()) - float(v64.detach()))
                gerr, gmax = float((g32.double() - g64).abs().max()), float(g64.abs().max())
                print("%s ign=%s w=%s labels=%s: value err %.3g of %.3g, gradient err %.3g of %.3g"
                      % (shape, ign, w is not None, tgt is not None, err, max(abs(float(v64.detach())), S), gerr, gmax))
                assert err <= 2e-6 * max(abs(float(v64.detach())), S)
                assert gerr <= 1e-6 * gmax


def test_argument_errors_come_before_any_device_work():
    from advchain.common.loss import boundary_loss, distance_transform_edt, signed_distance_maps
    x = torch.rand(2, 4, 8, 8)
    y = torch.randint(0, 4, (2, 8, 8))
    maps = torch.rand(2, 4, 8, 8)
    m = torch.ones(2, 8, 8, dtype=torch.bool)
    for bad in ((1.0,), (1.0, 2.0, 3.0), (1.0, 0.0), (1.0, -2.0), (float("nan"), 1.0), (float("inf"), 1.0), 2.0):
        with pytest.raises(ValueError, match="sampling"):
            distance_transform_edt(m, sampling=bad)
        with pytest.raises(ValueError, match="sampling"):
            signed_distance_maps(y, 4, sampling=bad)
        with pytest.raises(ValueError, match="sampling"):
            boundary_loss(x, y, sampling=bad)
    for bad in (m[0], m[None, None, None], 3):
        with pytest.raises(ValueError):
            distance_transform_edt(bad)
    for bad in (y[0], y[None, None, None]):
        with pytest.raises(ValueError):
            signed_distance_maps(bad, 4)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="num_classes"):
            signed_distance_maps(y, bad)
    with pytest.raises(ValueError):
        boundary_loss(x[0], y[0])
    with pytest.raises(ValueError, match="ignore_background"):
        boundary_loss(x[:, :1], y)
    with pytest.raises(ValueError, match="weight"):
        boundary_loss(x, y, weight=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="weight"):
        boundary_loss(x, y, weight=torch.ones(5))
    with pytest.raises(ValueError, match="weight"):
        boundary_loss(x, y, weight=2.0)
    with pytest.raises(ValueError, match="exactly one"):
        boundary_loss(x)
    with pytest.raises(ValueError, match="exactly one"):
        boundary_loss(x, y, dist_maps=maps)
    with pytest.raises(ValueError, match="target"):
        boundary_loss(x, y[:, :4])
    with pytest.raises(ValueError, match="dist_maps"):
        boundary_loss(x, dist_maps=maps[:, :3])
    with pytest.raises(ValueError, match="sampling"):
        boundary_loss(x, dist_maps=maps, sampling=(1.0, 1.0))


def test_cpu_tensors_raise():
    from advchain.common.loss import boundary_loss, distance_transform_edt, signed_distance_maps
    from advchain_amd import _lib
    for shape in ((2, 4, 8, 8), (2, 4, 4, 8, 8)):
        x = torch.rand(shape)
        y = torch.randint(0, 4, (2,) + shape[2:])
        with pytest.raises(_lib.AdvchainHipError):
            distance_transform_edt(y > 0)
        with pytest.raises(_lib.AdvchainHipError):
            signed_distance_maps(y, 4)
        with pytest.raises(_lib.AdvchainHipError):
            boundary_loss(x, y)
        with pytest.raises(_lib.AdvchainHipError):
            boundary_loss(x, dist_maps=torch.rand(shape), ignore_background=False, weight=[1.0, 2.0, 1.0, 1.0])
    maps = torch.rand(2, 4, 8, 8, requires_grad=True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with pytest.raises(_lib.AdvchainHipError):
            boundary_loss(torch.rand(2, 4, 8, 8), dist_maps=maps)
    assert any("constant" in str(w.message) for w in seen)


def test_workspace_queries_reject_bad_sizes():
    from advchain_amd import _lib
    lib = _lib.load()
    d2, d3 = _lib.dims_array((8, 8)), _lib.dims_array((4, 8, 8))
    bad = _lib.dims_array((0, 8))
    for query in (lib.advchain_signed_maps_workspace, lib.advchain_boundary_workspace):
        assert query(2, 4, 4, d2) < 0
        assert query(2, 4, 1, d2) < 0
        assert query(2, 4, 2, bad) < 0
        assert query(2, 4, 2, None) < 0
        assert query(2, 0, 2, d2) < 0
        assert query(0, 4, 2, d2) < 0
        assert query(2, 65536, 2, d2) < 0
    assert lib.advchain_signed_maps_workspace(2, 4, 2, d2) == 2 * 4 * 2 * 64
    assert lib.advchain_signed_maps_workspace(2, 4, 3, d3) == 2 * 4 * 2 * 256
    assert lib.advchain_boundary_workspace(2, 4, 2, d2) == 2
    assert lib.advchain_boundary_workspace(2, 4, 3, d3) == 2
    assert lib.advchain_boundary_workspace(3, 4, 2, _lib.dims_array((36, 57))) == 9
    # the distance fields: an axis above 32767, a squared diagonal of 2^30 or more, a line that does not fit in LDS
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8, 32768))) < 0
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8, 32767))) > 0
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8192, 32767))) < 0          # 8191^2 + 32766^2 >= 2^30
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8193, 8))) < 0
    assert lib.advchain_signed_maps_workspace(1, 1, 2, _lib.dims_array((8192, 8))) > 0
    assert lib.advchain_signed_maps_workspace(65535, 65535, 3, _lib.dims_array((8192, 8192, 8192))) < 0


def test_c_entries_reject_bad_arguments_on_the_host():
    from advchain_amd import _lib
    lib = _lib.load()
    d2 = _lib.dims_array((8, 8))
    bad = _lib.dims_array((0, 8))
    p = ctypes.c_void_p(16)            # never dereferenced: every call below fails validation before any launch
    ok_s, neg_s, nan_s = _lib.float_array([1.5, 0.7]), _lib.float_array([1.5, -0.7]), _lib.float_array([float("nan"), 1.0])

    def edt(mask=p, kind=1, s=None, sq=0, out=p, B=2, ndim=2, dims=d2):
        return lib.advchain_edt(mask, kind, s, sq, out, B, ndim, dims, None)

    def maps(lab=p, s=None, out=p, ws=p, N=2, K=4, ndim=2, dims=d2):
        return lib.advchain_signed_maps(lab, s, out, ws, N, K, ndim, dims, None)

    def fwd(x=p, bf16=0, lab=p, m=p, ws=p, value=p, N=2, K=4, ndim=2, dims=d2, flags=0):
        return lib.advchain_boundary_fwd(x, bf16, lab, m, None, p, ws, value, N, K, ndim, dims, flags, None)

    def bwd(x=p, bf16=0, lab=None, m=p, saved=p, gx=p, N=2, K=4, ndim=2, dims=d2, flags=0):
        return lib.advchain_boundary_bwd(x, bf16, lab, m, None, saved, None, gx, N, K, ndim, dims, flags, None)

    cases = [
        (lambda: edt(mask=None), b"null"), (lambda: edt(out=None), b"null"), (lambda: edt(kind=0), b"kind"),
        (lambda: edt(kind=4), b"kind"), (lambda: edt(sq=2), b"squared"), (lambda: edt(ndim=4), b"dims"),
        (lambda: edt(ndim=1), b"dims"), (lambda: edt(dims=bad), b"dims"), (lambda: edt(dims=None), b"dims"),
        (lambda: edt(B=0), b"B"), (lambda: edt(s=neg_s), b"sampling"), (lambda: edt(s=nan_s), b"sampling"),
        (lambda: edt(s=ok_s, out=None), b"null"),
        (lambda: edt(dims=_lib.dims_array((8, 40000))), b"too large"),
        (lambda: edt(dims=_lib.dims_array((30000, 30000))), b"too large"),
        (lambda: edt(dims=_lib.dims_array((20000, 8))), b"too large"),
        (lambda: maps(lab=None), b"null"), (lambda: maps(out=None), b"null"), (lambda: maps(ws=None), b"null"),
        (lambda: maps(K=0), b"K"), (lambda: maps(K=65536), b"K"), (lambda: maps(N=0), b"N"),
        (lambda: maps(ndim=5), b"dims"), (lambda: maps(dims=bad), b"dims"), (lambda: maps(s=neg_s), b"sampling"),
        (lambda: maps(dims=_lib.dims_array((8, 40000))), b"too large"),
        (lambda: maps(dims=_lib.dims_array((9000, 8))), b"too large"),
        (lambda: fwd(x=None), b"null"), (lambda: fwd(m=None), b"null"), (lambda: fwd(ws=None), b"null"),
        (lambda: fwd(value=None), b"null"), (lambda: fwd(K=0), b"K"), (lambda: fwd(K=65536), b"K"),
        (lambda: fwd(dims=bad), b"dims"), (lambda: fwd(ndim=4), b"dims"), (lambda: fwd(N=0), b"dims"),
        (lambda: fwd(bf16=2), b"bf16"), (lambda: fwd(flags=2), b"flags"), (lambda: fwd(K=1, flags=1), b"ignore_background"),
        (lambda: bwd(x=None), b"null"), (lambda: bwd(m=None), b"null"), (lambda: bwd(saved=None), b"null"),
        (lambda: bwd(gx=None), b"null"), (lambda: bwd(K=0), b"K"), (lambda: bwd(dims=bad), b"dims"),
        (lambda: bwd(bf16=-1), b"bf16"), (lambda: bwd(flags=4), b"flags"), (lambda: bwd(K=1, flags=1), b"ignore_background"),
    ]
    for i, (call, word) in enumerate(cases):
        rc = call()
        assert rc < 0, (i, word)
        assert word in lib.advchain_last_error(), (i, word, lib.advchain_last_error())
    assert edt(dims=_lib.dims_array((8, 40000))) == -2 and maps(dims=_lib.dims_array((9000, 8))) == -2


# ---- the edge cases of tests/test_edt_edges_gpu.py -------------------------------------------------------------------------------

def test_the_plan_mirror_at_the_figures_of_the_source():
    """edt_plan against the numbers the header of csrc/edt.hip and its constants give by hand."""
    assert edt_plan(70, 300, 12, 70, 1)[:3] == (2, 1024, 1)                 # the largest K * chunks of the older tests: 600
    assert edt_plan(1900, 70, 3, 1900, 2)[:3] == (30, 68, 2)
    assert edt_plan(32767, 5, 2, 32767, 2)[:3] == (512, 4, 2)
    assert edt_plan(32767, 4, 2, 32767, 2)[2] == 1 and edt_plan(64, 2048, 2, 64, 1)[:3] == (1, 2048, 1)
    for L, TX in ((64, 64), (65, 32), (128, 32), (129, 16), (1024, 16), (1025, 8), (2048, 8), (2049, 4), (4096, 4), (4097, 2),
                  (8192, 2), (8193, 1), (16384, 1)):                           # one field, lines wide apart
        assert edt_plan(64, 1, L, 4096, 1)[3] == TX, L
        if L % 2 == 0:
            assert edt_plan(64, 1, L // 2, 4096, 2)[3] == TX, L               # two fields: every limit half as long
    for I, TX in ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64)):
        assert edt_plan(64, 1, 8, I, 1)[3] == TX, I                           # the loop that narrows because TX / 2 >= I
    assert edt_plan(2, 1, 16384, 2, 1)[3:] == (1, 65536) and edt_plan(2, 2, 8192, 2, 2)[3:] == (1, 65536)


ALL_EDGE = [(1, c[0], c[2], 1) for c in EDGE_EDT_CASES] + [(c[0], c[1], c[2], 2) for c in EDGE_MAP_CASES] + \
           [(c[0], c[1], c[2], 1) for c in EDGE_SURFACE_CASES]


@pytest.mark.parametrize("K,shape,claim,NF", ALL_EDGE, ids=["%s-nf%d" % (edge_case_id((K, sh)), nf) for K, sh, _, nf in ALL_EDGE])
def test_edge_cases_take_the_branch_they_are_listed_for(K, shape, claim, NF):
    plan = edt_case_plan(K, shape[1:], NF)
    assert claim, shape
    for key, want in claim.items():
        assert plan[key] == want, (shape, key, plan)


def test_edge_case_lists_hold_every_branch_they_are_there_for():
    plans = {c[0]: edt_case_plan(1, c[0][1:], 1) for c in EDGE_EDT_CASES}
    maps = {(c[0], c[1]): edt_case_plan(c[0], c[1][1:], 2) for c in EDGE_MAP_CASES}
    assert sorted({p["TX"] for p in plans.values()} & {8, 4, 2, 1}) == [1, 2, 4, 8]
    assert sorted({p["TX"] for p in maps.values()} & {8, 2, 1}) == [1, 2, 8]
    assert all(plans[s]["lds"] == 65536 or plans[s]["chunks"] == 512 for s in EDGE_EDT_LIMITS)
    assert plans[(1, 16384, 2)]["lds"] == 65536 and maps[(2, (1, 8192, 2))]["lds"] == 65536
    assert all(case in maps for case in EDGE_MAP_LIMITS)
    assert sum(p["launches"] == 2 for p in maps.values()) == 2
    assert any(p["chunks"] > 4 and p["chunks"] % 4 for p in plans.values()) and any(p["chunks"] > 8 for p in plans.values())
    assert any(s[-1] % 64 == 0 and s[-1] > 64 for s in plans) and any(s[-1] == 64 for s in plans)     # rows without a tail
    assert all(any(s[1 + a] == 1 for s in plans if len(s) == 1 + nd) for nd in (2, 3) for a in range(nd))   # every axis 1-wide
    assert edt_case_plan(300, (3, 400), 1)["launches"] == 2 and all(p["launches"] == 1 for p in plans.values())


def test_old_and_edge_cases_together_run_every_tile_width():
    """AXIS_FINISH at every TX from 64 down to 1, AXIS_FINISH_SIGNED at 32, 8, 2 and 1 at least, and AXIS_PLAIN (the second pass
    of a 3D call) at 64, 8 and 1."""
    finish = {edt_case_plan(1, s[1:], 1)["TX"] for s in EDT_SHAPES + [c[0] for c in EDGE_EDT_CASES]}
    assert finish == {64, 32, 16, 8, 4, 2, 1}, finish
    signed = {edt_case_plan(K, s[1:], 2)["TX"] for K, s in MAP_CASES + [(c[0], c[1]) for c in EDGE_MAP_CASES]}
    assert signed >= {32, 8, 2, 1}, signed
    plain = {edt_case_plan(1, c[0][1:], 1)["plain_TX"] for c in EDGE_EDT_CASES if len(c[0]) == 4}
    assert plain >= {64, 8, 1}, plain
    assert all(L >= 1 and I >= 1 for c in EDGE_EDT_CASES for L, I in edt_axis_passes(c[0][1:]))


@pytest.mark.parametrize("case", EDGE_EDT_CASES, ids=[edge_case_id(c) for c in EDGE_EDT_CASES])
def test_no_pattern_of_an_edge_case_has_a_trivial_answer(case):
    """Every (case, pattern) has an entry whose answer is neither all zero nor all infinite -- but for the single voxel, whose
    answer is one or the other: its two patterns give both."""
    shape, patterns = case[0], case[1]
    assert patterns
    if shape == (1, 1, 1):
        assert float(edge_edt_reference(shape, "one_corner")[1][0]) == 0.0
        assert float(edge_edt_reference(shape, "full_entry")[1][0]) == float("inf")
        return
    for name in patterns:
        m, sq, _ = edge_edt_reference(shape, name)
        assert any(bool((e[torch.isfinite(e)] > 0).any()) for e in sq), (shape, name)
        if name in ("far_left", "far_right") and shape[-1] > 64:
            assert float(sq[torch.isfinite(sq)].max()) >= (shape[-1] - 1) ** 2
    if shape == (1, 2, 32767):                                # the farthest squared distance the fields can hold, above 2^24
        assert float(edge_edt_reference(shape, "far_left")[1].max()) == 32766.0 ** 2
        assert float(edge_edt_reference(shape, "one_corner")[1].max()) == 32766.0 ** 2 + 1 < 2 ** 30


@pytest.mark.parametrize("case", EDGE_MAP_CASES, ids=[edge_case_id(c) for c in EDGE_MAP_CASES])
def test_label_edge_cases_hold_every_class_and_the_second_group_in_the_middle(case):
    K, shape = case[0], case[1]
    y = edge_label_case(K, shape, seed=K)
    W = shape[-1]
    group = edt_case_plan(K, shape[1:], 2)["group"]
    assert bool((y == -100).any()) and bool((y == K + 3).any())
    for k in range(K):
        at = torch.nonzero(y == k)
        assert 0 < at.shape[0] < y.numel(), k
        if k >= group:                                         # one run of 9 voxels, at least a chunk away from both ends of its row
            assert at.shape[0] == 9 and int(at[:, -1].min()) >= 64 and int(at[:, -1].max()) < W - 64
            assert len({tuple(v[:-1].tolist()) for v in at}) == 1 and int(at[:, -1].max() - at[:, -1].min()) == 8
    if K > group:
        assert K - group <= 2 and group < K


def test_surface_edge_case_holds_the_second_group_in_both_maps():
    K, shape = EDGE_SURFACE_CASES[0][:2]
    p, y = edge_surface_pair(K, shape, seed=K)
    group = edt_case_plan(K, shape[1:], 1)["group"]
    assert group < K
    for k in range(group, K):
        for t in (p, y):
            x = torch.nonzero(t == k)[:, -1]
            assert int(((x >= 64) & (x < shape[-1] - 64)).sum()) >= 9, k      # (the random blocks may hold the class elsewhere too)
        assert not torch.equal(p == k, y == k)


@pytest.mark.parametrize("case", EDGE_EDT_CASES, ids=[edge_case_id(c) for c in EDGE_EDT_CASES])
def test_fp32_stays_inside_the_sampling_bound_at_the_edge_cases(case):
    """The fp32 evaluation of |S (v - u)| from its definition against float64 at the edge shapes and patterns: inside SAMPLING_TOL
    on its own (the worst case by its roundings is 2.1e-7 whatever the distance: every bound of the older test's docstring is
    relative), here at distances up to 0.7 * 32766 and 1.5 * 16383."""
    shape, patterns = case[0], case[1]
    s = SAMPLING[len(shape) - 1]
    worst = 0.0
    for name in patterns:
        m, _, want = edge_edt_reference(shape, name)
        got = edt_brute(m, s, dtype=torch.float32)
        fin = torch.isfinite(want) & (want > 0)
        assert torch.equal(torch.isfinite(got), torch.isfinite(want))
        if bool(fin.any()):
            worst = max(worst, float(((got - want).abs()[fin] / want[fin]).max()))
    print("fp32 sampling error at %s: %.3g" % (shape, worst))
    assert worst <= SAMPLING_TOL


def test_the_entries_accept_the_limit_cases_and_refuse_one_voxel_more():
    from advchain_amd import _lib
    lib = _lib.load()
    maps_ws, surface_ws = lib.advchain_signed_maps_workspace, lib.advchain_surface_metrics_workspace
    for K, shape in EDGE_MAP_LIMITS:
        N, dims = shape[0], shape[1:]
        assert maps_ws(N, K, len(dims), _lib.dims_array(dims)) == N * K * 2 * dims[0] * dims[1]
        assert surface_ws(N, K, len(dims), _lib.dims_array(dims)) > 0
    for query in (maps_ws, surface_ws):
        assert query(1, 2, 2, _lib.dims_array((8193, 2))) < 0
        assert query(1, 5, 2, _lib.dims_array((2, 32768))) < 0
        assert query(1, 1, 3, _lib.dims_array((8193, 2, 2))) < 0 and query(1, 1, 3, _lib.dims_array((2, 8193, 2))) < 0
        assert query(1, 1, 3, _lib.dims_array((8192, 2, 2))) > 0 and query(1, 1, 3, _lib.dims_array((2, 8192, 2))) > 0
    # the transform has no query: its refusals come from the entry itself, before any launch (the pointer is never read)
    p = ctypes.c_void_p(16)
    for dims in ((16385, 2), (2, 32768), (16385, 2, 2), (2, 16385, 2), (2, 2, 32768)):
        assert lib.advchain_edt(p, 1, None, 0, p, 1, len(dims), _lib.dims_array(dims), None) == -2, dims
        assert b"too large" in lib.advchain_last_error()
    for dims in ((8193, 2), (2, 32768)):
        assert lib.advchain_signed_maps(p, None, p, p, 1, 2, 2, _lib.dims_array(dims), None) == -2, dims
        assert b"too large" in lib.advchain_last_error()
