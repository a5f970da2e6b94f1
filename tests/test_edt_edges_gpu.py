"""The dispatch edges of csrc/edt.hip on the device, against the brute-force float64 forms of tests/edt_forms.py and
tests/surface_forms.py: rows of more than four chunks and of exact multiples of 64 (a wave's second and third chunk, carries
across empty chunks from both ends), a second launch of k_edt_rows (K * chunks above 2048 ballots: signed maps, the surface
metrics' fields and boundary_loss from labels), the axis kernel at every tile width from 8 x down to 1 in both finishing modes,
the largest shapes the entries accept (a row of 32767, a leading axis of 16384 or 8192: 64 KiB of dynamic LDS, squared
distances next to the int32 sentinel) with their refusals one voxel later, and axes of length 1.  tests/test_boundary_cpu.py
checks with a mirror of the host loops that each case takes the branch it is listed for.

Two properties need no reference: a transposed (permuted) mask gives the transposed result bit for bit -- the row pass with
its ballots and carries against the axis pass with its scan -- and entry b of a batch is the transform of that mask alone.

Bounds: those of tests/test_boundary_gpu.py (ULP = 1.2e-7 relative with unit spacing, SAMPLING_TOL with a sampling and twice
that for its squares, TOL_V and TOL_G for the loss) and of tests/test_surface_gpu.py, unchanged.  squared=True is compared with
the float64 integer ROUNDED ONCE to fp32 (want.float().double()): a square above 2^24 need not be an fp32 number, and the
kernel converts the exact int32 once; below 2^24 that is the older test's torch.equal with the integer itself."""
import pytest
import torch

from tests.edt_forms import (EDGE_EDT_CASES, EDGE_EDT_LIMITS, EDGE_MAP_CASES, EDGE_MAP_LIMITS, EDGE_SURFACE_CASES, SAMPLING,
                             SAMPLING_TOL, edge_case_id, edge_edt_reference, edge_label_case, edge_map_reference, edge_surface_pair,
                             edt_case_plan, mask_pattern)
from tests.surface_forms import surface_brute
from tests.test_boundary_gpu import ULP, _against_closed, _grads_of, _relative_close
from tests.test_surface_gpu import _against as _surface_against

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
EDT_PAIRS = [(c[0], name) for c in EDGE_EDT_CASES for name in c[1]]


def _L():
    import advchain.common.loss as L
    return L


@pytest.mark.parametrize("shape,name", EDT_PAIRS, ids=["%s-%s" % ("x".join(map(str, s)), n) for s, n in EDT_PAIRS])
def test_transform_against_brute_force(shape, name):
    """Squared distances: the exact integer rounded once to fp32 (module docstring); distances: one fp32 ulp of the float64 root;
    with a sampling SAMPLING_TOL (twice for the squares); every mask dtype gives the bits of bool."""
    L = _L()
    m, want_sq, want_s = edge_edt_reference(shape, name)
    md = m.to(DEV)
    sq = L.distance_transform_edt(md, squared=True)
    assert sq.dtype == torch.float32 and sq.shape == md.shape
    assert torch.equal(sq.cpu().double(), want_sq.float().double()), (shape, name)
    d = L.distance_transform_edt(md)
    _relative_close(d, want_sq.sqrt(), ULP, "edt %s %s" % (shape, name))
    s = SAMPLING[len(shape) - 1]
    _relative_close(L.distance_transform_edt(md, sampling=s), want_s, SAMPLING_TOL, "edt sampling %s %s" % (shape, name))
    _relative_close(L.distance_transform_edt(md, sampling=s, squared=True), want_s * want_s, 2 * SAMPLING_TOL,
                    "edt sampling squared %s %s" % (shape, name))
    for other in (md.to(torch.uint8), md.long() * 7, md.float() * -0.5):
        assert torch.equal(L.distance_transform_edt(other), d)
    assert torch.equal(L.distance_transform_edt(md), d)
    if name == "full_entry":
        assert bool(torch.isinf(d[0]).all()) and torch.equal(torch.isfinite(d[1:]).cpu(), torch.isfinite(want_sq[1:]))
    if tuple(shape) in EDGE_EDT_LIMITS:                             # (their patterns all have a zero voxel in every entry)
        assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(sq).all())


@pytest.mark.parametrize("case", EDGE_MAP_CASES, ids=[edge_case_id(c) for c in EDGE_MAP_CASES])
def test_signed_maps_against_brute_force(case):
    L = _L()
    K, shape = case[0], case[1]
    y, want, want_s = edge_map_reference(K, shape)
    yd = y.to(DEV)
    got = L.signed_distance_maps(yd, K)
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], K) + tuple(shape[1:])
    _relative_close(got, want, ULP, "maps %s" % edge_case_id(case))
    assert bool(torch.isfinite(got).all())
    assert float(got[got != 0].abs().min()) >= 1.0                  # at least one spacing in magnitude
    inside = torch.stack([yd == k for k in range(K)], 1)
    assert bool((got[inside] <= 0).all()) and bool((got[~inside] >= 0).all())
    _relative_close(L.signed_distance_maps(yd, K, sampling=SAMPLING[len(shape) - 1]), want_s, SAMPLING_TOL,
                    "maps sampling %s" % edge_case_id(case))
    assert torch.equal(L.signed_distance_maps(yd, K), got)
    # the map of class k is the difference of two transforms of its membership mask: the first class, the last, and the first
    # that a second launch of the row kernel writes
    group = edt_case_plan(K, shape[1:], 2)["group"]
    for k in sorted({0, K - 1, min(group, K - 1)}):
        member = yd == k
        pair = L.distance_transform_edt(~member) - L.distance_transform_edt(member)
        assert bool(torch.isfinite(pair).all())                     # every class of these cases is present and fills no entry
        assert torch.equal(got[:, k], pair), k
    for k in range(group, K):                                       # a group that was never written, or written over
        assert float(got[:, k].abs().max()) > 0.0, k


@pytest.mark.parametrize("case", EDGE_SURFACE_CASES, ids=[edge_case_id(c) for c in EDGE_SURFACE_CASES])
def test_surface_metrics_against_brute_force(case):
    import advchain.common.metrics as M
    K, shape = case[0], case[1]
    p, y = edge_surface_pair(K, shape, seed=K)
    pd, yd = p.to(DEV), y.to(DEV)
    got = M.surface_distance_metrics(pd, yd, K)
    _surface_against(got, surface_brute(p, y, K), False, "surface %s" % edge_case_id(case))
    group = edt_case_plan(K, shape[1:], 1)["group"]
    for k in range(group, K):                                       # the second group: both borders exist and do not coincide
        assert bool((got.surface_voxels[0, k] > 0).all()) and float(got.hausdorff[0, k]) > 0.0, k
    s = SAMPLING[len(shape) - 1]
    _surface_against(M.surface_distance_metrics(pd, yd, K, sampling=s), surface_brute(p, y, K, s), True,
                     "surface sampling %s" % edge_case_id(case))


def _edt_all(L, m, s):
    return (L.distance_transform_edt(m), L.distance_transform_edt(m, squared=True), L.distance_transform_edt(m, sampling=s))


@pytest.mark.parametrize("name", ["sparse", "ends", "one_corner", "mid_chunk", "fg95", "full_entry"])
def test_transposed_masks_give_the_transposed_transform(name):
    """With unit spacing every tiling gives the same bits, so the axis a line lies along cannot matter: rows of 257 (5 chunks)
    against an axis pass of 257 and the reverse, 2D; one permutation of all three axes in 3D (rows of 200, 70 and 9)."""
    L = _L()
    m = mask_pattern((1, 300, 257), name, seed=7).to(DEV)
    assert torch.equal(L.distance_transform_edt(m.transpose(-1, -2).contiguous()), L.distance_transform_edt(m).transpose(-1, -2))
    assert torch.equal(L.distance_transform_edt(m.transpose(-1, -2).contiguous(), squared=True),
                       L.distance_transform_edt(m, squared=True).transpose(-1, -2))
    m = mask_pattern((2, 9, 70, 200), name, seed=8).to(DEV)
    want = L.distance_transform_edt(m)
    assert bool(torch.isfinite(want[-1]).any()) and float(want[-1][torch.isfinite(want[-1])].max()) > 0.0
    for order in ((0, 3, 1, 2), (0, 2, 3, 1)):
        assert torch.equal(L.distance_transform_edt(m.permute(order).contiguous()), want.permute(order)), order


def test_transposed_labels_give_the_transposed_signed_maps():
    L = _L()
    y = edge_label_case(3, (1, 300, 257), seed=3).to(DEV)
    y[0, 40:200, 100:230] = 0                                       # one large block: distances across several chunks
    want = L.signed_distance_maps(y, 3)
    assert float(want.abs().max()) > 40.0
    assert torch.equal(L.signed_distance_maps(y.transpose(-1, -2).contiguous(), 3), want.transpose(-1, -2))
    y = edge_label_case(3, (2, 9, 70, 200), seed=4).to(DEV)
    y[0, 2:8, 10:60, 30:190] = 1
    want = L.signed_distance_maps(y, 3)
    for order in ((0, 3, 1, 2), (0, 2, 3, 1)):
        got = L.signed_distance_maps(y.permute(order).contiguous(), 3)
        assert torch.equal(got, want.permute((0, 1) + tuple(a + 1 for a in order[1:]))), order


@pytest.mark.parametrize("shape", [(3, 2, 600), (3, 2100, 3)], ids=["long-row", "narrow-tile"])
def test_an_entry_of_a_batch_is_the_transform_of_that_mask_alone(shape):
    L = _L()
    one = (1,) + shape[1:]
    batch = torch.cat([mask_pattern(one, name, seed=5) for name in ("ends", "sparse", "fg95")]).to(DEV)
    s = SAMPLING[2]
    whole = _edt_all(L, batch, s)
    assert all(not torch.equal(whole[0][0], whole[0][b]) for b in (1, 2))
    for b in range(3):
        alone = _edt_all(L, batch[b:b + 1].contiguous(), s)
        assert all(torch.equal(w[b], a[0]) for w, a in zip(whole, alone)), b
    y = torch.cat([edge_label_case(2, one, seed=sd) for sd in (1, 2, 3)]).to(DEV)
    maps = L.signed_distance_maps(y, 2)
    for b in range(3):
        assert torch.equal(maps[b], L.signed_distance_maps(y[b:b + 1].contiguous(), 2)[0]), b


def test_one_voxel_beyond_a_limit_is_refused_on_the_host():
    """NotImplementedError from the Python layer; from the C entries the `unsupported` code (-2) before any launch: a pre-filled
    output and workspace keep their values.  (The limit cases themselves run in the tests above.)"""
    from advchain_amd import _lib, ops
    L = _L()
    lib = _lib.load()
    for sp in ((2, 32768), (16385, 2)):
        with pytest.raises(NotImplementedError):
            L.distance_transform_edt(torch.ones((1,) + sp, device=DEV, dtype=torch.bool))
        mask = torch.ones((1,) + sp, device=DEV, dtype=torch.uint8)
        out = torch.full((1,) + sp, -7.0, device=DEV)
        assert lib.advchain_edt(ops._ptr(mask), 1, None, 0, ops._ptr(out), 1, 2, _lib.dims_array(sp), ops._stream()) == -2
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
    for K, sp in ((5, (2, 32768)), (2, (8193, 2))):
        y = torch.zeros((1,) + sp, device=DEV, dtype=torch.int64)
        with pytest.raises(NotImplementedError):
            L.signed_distance_maps(y, K)
        with pytest.raises(NotImplementedError):
            L.boundary_loss(torch.zeros((1, K) + sp, device=DEV), y)
        out = torch.full((1, K) + sp, -7.0, device=DEV)
        ws = torch.full((2 * K * sp[0] * sp[1],), -7.0, device=DEV)
        assert lib.advchain_signed_maps(ops._ptr(y), None, ops._ptr(out), ops._ptr(ws), 1, K, 2, _lib.dims_array(sp), ops._stream()) == -2
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((ws == -7.0).all())


@pytest.mark.parametrize("K,shape", [(2, (1, 2100, 3)), (70, (1, 3, 1900))], ids=["narrow-tile", "class-groups"])
def test_boundary_loss_from_labels_at_the_edges(K, shape):
    """boundary_loss with a label target runs the same passes (AXIS_FINISH_SIGNED at TX 2; two launches of the row kernel):
    against the closed form on the brute-force maps, and bit for bit the loss on the maps given."""
    L = _L()
    y, maps64, _ = edge_map_reference(K, shape)
    y = torch.where(y == K + 3, torch.full_like(y, -100), y)        # (no class either way: the same maps, and a finite loss)
    g = torch.Generator().manual_seed(K)
    x = (torch.randn((shape[0], K) + tuple(shape[1:]), generator=g) * 2).to(DEV).requires_grad_(True)
    yd = y.to(DEV)
    for ign in (False, True):
        _against_closed(x, lambda: L.boundary_loss(x, yd, ignore_background=ign),
                        dict(target=y, ignore_background=ign, dist_maps=maps64), "labels %s ign=%s" % (shape, ign))
    # bit for bit needs every voxel counted on both paths: the voxels without a class go to class 0 (no reference needed)
    yc = torch.where(yd < 0, torch.zeros_like(yd), yd)
    given = L.signed_distance_maps(yc, K)
    assert all(float(given[:, k].abs().max()) > 0.0 for k in range(K))
    for ign in (False, True):
        va, ga = _grads_of(lambda: L.boundary_loss(x, yc, ignore_background=ign), x)
        vb, gb = _grads_of(lambda: L.boundary_loss(x, dist_maps=given, ignore_background=ign), x)
        assert bool(torch.isfinite(va)) and float(ga.abs().max()) > 0.0
        assert torch.equal(va, vb) and torch.equal(ga, gb)
