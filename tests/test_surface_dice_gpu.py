"""common.metrics.surface_dice on the HIP kernels (csrc/seg_surface.hip: the ball route k_surface_ball and the field route
k_surface_within on the fields of csrc/edt.hip) against the brute-force form of tests/surface_dice_forms.py: every case of
tests/surface_forms.CASES (1 to 300 classes, rows longer than a wave, the 600-long column, 3D with the longest axis outermost) on
every eligible route, the two routes against each other (also at exact ties of the sampled comparison), the seams of the ball
kernel's tiles, identities, the empty-border conventions, bitwise reproducibility, a captured graph, misaligned and
non-contiguous inputs and the device guard.

Bounds.  within and surface_voxels are integers: torch.equal.  surface_dice is a quotient of those integers taken in fp64 and
rounded to fp32 once (half an ulp): within 1.2e-7 relative of the float64 reference, NaN and zeros exactly.  With a sampling the
tolerances are chosen so that no float64 squared distance of the reference is within 1e-3 relative of tau^2 (asserted); the fp32
fields are within 4e-6 of the float64 squares (twice SAMPLING_TOL), so the counts must be equal.

The share of border voxels within the tolerance in the reference, with unit spacing, pooled over ALL border voxels of a case
(both maps, every entry and class -- the issue's wording; a class with one empty border adds voxels and nothing within) and, after
the slash, over the classes with both borders only:
    case            0          1          1.5        2          3
    K1-2x5x7        0          0          0          0          0          (no border voxel of the two maps nearer than 3.2)
    K4-3x36x57      .209/.255  .535/.653  .576/.704  .710/.867  .768/.938
    K20-1x70x130    .197/.203  .572/.590  .644/.664  .838/.864  .918/.946
    K2-1x600x9      .446/.446  .815/.815  .856/.856  .937/.937  .979/.979
    K4-2x6x10x70    .291/.357  .568/.696  .609/.746  .705/.864  .775/.949
    K70-1x33x9x5    .131/.135  .373/.381  .470/.482  .559/.572  .629/.644
    K300-1x12x70    .202/.207  .544/.559  .615/.632  .832/.855  .904/.929
The test asserts 10 to 95 % for both poolings at every tolerance of part 1, except in the two cells where the maps do not give
it: K1-2x5x7 (0 at every tolerance: asserted to be 0) and K2-1x600x9 at tolerance 3 (asserted to be 95 to 99 %)."""
import pytest
import torch

from tests.edt_forms import SAMPLING, SAMPLING_TOL
from tests.surface_dice_forms import dice_of, smallest_gap
from tests.surface_forms import CASES, case_id, directed_squares
from tests.test_surface_gpu import _case                      # (the maps and squares of a case, computed once for both modules)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ULP = 1.2e-7
UNIT_TOLERANCES = [0, 1, 1.5, 2, 3]
FIELD_TOLERANCES = [9.5, 30]
SAMPLED_TOLERANCES = {2: [1.6, 2.2, 3.1], 3: [0.7, 1.5, 2.2, 4.1]}
TIES = {2: [0.7, 1.4], 3: [1.6, 2.0]}


def _M():
    import advchain.common.metrics as M
    return M


def _ops():
    from advchain_amd import ops
    return ops


def _routes(N, K, sp, tolerance, sampling=None):
    """The routes that can take the call."""
    out = []
    for r in ("ball", "fields"):
        try:
            _ops().surface_dice_route(N, K, sp, tolerance, sampling, route=r)
            out.append(r)
        except NotImplementedError:
            pass
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x).cpu(), _bits(y).cpu()) for x, y in zip(a, b))


def _against(got, want, what):
    N, K = want.surface_dice.shape
    assert isinstance(got, _M().SurfaceDice)
    for t, shape, dtype in ((got.surface_dice, (N, K), torch.float32), (got.within, (N, K, 2), torch.int64),
                            (got.surface_voxels, (N, K, 2), torch.int64)):
        assert t.is_cuda and tuple(t.shape) == shape and t.dtype == dtype, what
    assert torch.equal(got.surface_voxels.cpu(), want.surface_voxels), what
    assert torch.equal(got.within.cpu(), want.within), what
    g, w = got.surface_dice.cpu().double(), want.surface_dice
    nan = torch.isnan(w)
    assert torch.equal(torch.isnan(g), nan), what
    zero = (w == 0) & ~nan
    assert bool((g[zero] == 0).all()), what
    rest = ~zero & ~nan
    rel = (g - w).abs()[rest] / w[rest]
    worst = float(rel.max()) if rel.numel() else 0.0
    print("%s: relative error %.3g (bound %.3g)" % (what, worst, ULP))
    assert worst <= ULP, (what, worst)


def _pooled_shares(ref):
    """(over all border voxels, over the classes with both borders)"""
    both = (ref.surface_voxels > 0).all(-1)
    return (float(ref.within.sum()) / float(ref.surface_voxels.sum()),
            float(ref.within[both].sum()) / float(ref.surface_voxels[both].sum()))


@pytest.mark.parametrize("K,shape", CASES, ids=[case_id(c) for c in CASES])
def test_against_brute_force_with_unit_spacing(K, shape):
    ops = _ops()
    p, y, squares = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    N, sp = shape[0], shape[1:]
    for tau in UNIT_TOLERANCES + FIELD_TOLERANCES:
        want = dice_of(squares, N, K, tau, True)
        if tau in UNIT_TOLERANCES:
            shares = _pooled_shares(want)
            print("K=%d %s tolerance %g: %.3f / %.3f of the border voxels are within" % ((K, shape, tau) + shares))
            for share in shares:
                if shape == (2, 5, 7):
                    assert share == 0
                elif shape == (1, 600, 9) and tau == 3:
                    assert 0.95 < share <= 0.99
                else:
                    assert 0.10 <= share <= 0.95
        routes = _routes(N, K, sp, tau) if tau in UNIT_TOLERANCES else ["fields"]
        assert "fields" in routes and (tau not in UNIT_TOLERANCES or "ball" in routes)
        got = {r: ops.surface_dice(pd, yd, K, tau, route=r) for r in routes}
        for r in routes:
            _against(got[r], want, "%s tolerance %g K=%d %s" % (r, tau, K, shape))
        if len(routes) == 2:
            assert _same_bits(got["ball"], got["fields"])
        assert _same_bits(_M().surface_dice(pd, yd, K, tau), got["fields"])                 # (the public call: dispatch)
    if K >= 4:                                                # class K-1 is in neither map, class K-2 not in pred
        got = _M().surface_dice(pd, yd, K, 2)
        assert bool(torch.isnan(got.surface_dice[:, K - 1]).all()) and bool((got.within[:, K - 1:] == 0).all())
        present = got.surface_voxels[:, K - 2, 1] > 0
        assert bool(present.any()) and bool((got.surface_dice[:, K - 2][present] == 0).all())
        assert bool((got.within[:, K - 2] == 0).all())


@pytest.mark.parametrize("K,shape", CASES, ids=[case_id(c) for c in CASES])
def test_against_brute_force_with_a_sampling(K, shape):
    ops = _ops()
    nd = len(shape) - 1
    s = SAMPLING[nd]
    p, y, squares = _case(K, shape, True)
    pd, yd = p.to(DEV), y.to(DEV)
    for tau in SAMPLED_TOLERANCES[nd]:
        gap = smallest_gap(squares, K, tau)
        print("K=%d %s tolerance %g: no squared distance within %.3g relative of tau^2" % (K, shape, tau, gap))
        assert gap >= 1e-3 and gap > 100 * 2 * SAMPLING_TOL
        want = dice_of(squares, shape[0], K, tau, False)
        routes = _routes(shape[0], K, shape[1:], tau, s)
        assert routes == ["ball", "fields"]
        got = {r: ops.surface_dice(pd, yd, K, tau, sampling=s, route=r) for r in routes}
        for r in routes:
            _against(got[r], want, "%s sampling tolerance %g K=%d %s" % (r, tau, K, shape))
        assert _same_bits(got["ball"], got["fields"])
        assert _same_bits(_M().surface_dice(pd, yd, K, tau, sampling=s), got["ball"])


@pytest.mark.parametrize("K,shape", CASES, ids=[case_id(c) for c in CASES])
def test_both_routes_give_equal_bits_at_exact_ties(K, shape):
    """Tolerances that are multiples of a spacing: the fp32 square of the distance may fall on either side of the fp32 threshold,
    but on the same side on both routes.  The reference is the other route."""
    ops = _ops()
    nd = len(shape) - 1
    s = SAMPLING[nd]
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    for tau in TIES[nd] + [tuple(TIES[nd][k % 2] for k in range(K))]:
        ball = ops.surface_dice(pd, yd, K, tau, sampling=s, route="ball")
        fields = ops.surface_dice(pd, yd, K, tau, sampling=s, route="fields")
        assert _same_bits(ball, fields), tau
        assert bool((ball.within <= ball.surface_voxels).all())
    assert int(ball.within.sum()) > 0 or shape == (2, 5, 7)


# (K, shape, tolerance, owned tile): calls whose halo does not fit the widest tile of ops.SURFACE_DICE_TILE, one per narrower tile of
# the ball kernel.  Cells of a tile: prod(tile_a + 2 (cap_a + 1)), cap_a = min(tolerance, dims_a - 1), 5 bytes each in 61440.
NARROW = [(4, (2, 6, 10, 70), 4, (4, 8, 32)),        # caps 4, 4, 4: 18 x 18 x 42 cells for (8,8,32) do not fit, 14 x 18 x 42 do
          (4, (2, 6, 10, 70), 5, (4, 4, 32)),        # caps 5, 5, 5: 16 x 20 x 44 do not fit, 16 x 16 x 44 do
          (4, (2, 6, 10, 70), 6, (2, 4, 32)),        # caps 5, 6, 6: 16 x 18 x 46 do not fit, 14 x 18 x 46 do
          (4, (2, 6, 10, 70), 7, (2, 2, 32)),        # caps 5, 7, 7: 14 x 20 x 48 do not fit, 14 x 18 x 48 do
          (70, (1, 33, 9, 5), 6, (2, 4, 32)),        # caps 6, 6, 4: 18 x 18 x 42 do not fit, 16 x 18 x 42 do
          (20, (1, 70, 130), 33, (16, 64)),          # caps 33, 33: 100 x 132 do not fit, 84 x 132 do
          (20, (1, 70, 130), 36, (8, 64))]           # caps 36, 36: 90 x 138 do not fit, 82 x 138 do


def _ball_tile(sp, tolerance):
    """The owned tile the ball kernel takes at unit spacing, by the rule of csrc/seg_surface.hip."""
    halo = [min(int(tolerance), d - 1) + 1 for d in sp]
    tiles = [(32, 64), (16, 64), (8, 64)] if len(sp) == 2 else [(8, 8, 32), (4, 8, 32), (4, 4, 32), (2, 4, 32), (2, 2, 32)]
    for tile in tiles:
        cells = 1
        for t, h in zip(tile, halo):
            cells *= t + 2 * h
        if 4 * cells + (cells + 3) // 4 * 4 <= 61440:
            return tile
    return None


@pytest.mark.parametrize("K,shape,tau,tile", NARROW, ids=["%s-tolerance%d" % (case_id(c[:2]), c[2]) for c in NARROW])
def test_ball_on_its_narrowed_tiles(K, shape, tau, tile):
    """Halos that only a narrower tile can hold: the forced ball route against the brute force and against the fields, with unit
    spacing and with a sampling that keeps the caps (a hair below one voxel: nothing is tied)."""
    ops = _ops()
    assert _ball_tile(shape[1:], tau) == tile and tile != ops.SURFACE_DICE_TILE[len(tile)]
    assert "ball" in _routes(shape[0], K, shape[1:], tau)
    p, y, squares = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    ball = ops.surface_dice(pd, yd, K, tau, route="ball")
    _against(ball, dice_of(squares, shape[0], K, tau, True), "narrow ball tolerance %g K=%d %s" % (tau, K, shape))
    assert _same_bits(ball, ops.surface_dice(pd, yd, K, tau, route="fields"))
    s = (0.999,) * (len(shape) - 1)
    assert _same_bits(ops.surface_dice(pd, yd, K, tau, sampling=s, route="ball"),
                      ops.surface_dice(pd, yd, K, tau, sampling=s, route="fields"))


def _seam_maps(nd, cap, second_tile):
    tile = _ops().SURFACE_DICE_TILE[nd]
    at = tuple(t if second_tile else t - 1 for t in tile)
    dims = tuple(t + cap + 3 for t in tile)
    offsets = torch.cartesian_prod(*[torch.arange(-cap - 1, cap + 2)] * nd)
    N = offsets.shape[0]
    p = torch.full((N,) + dims, -100, dtype=torch.int64)
    y = torch.full((N,) + dims, -100, dtype=torch.int64)
    for n in range(N):
        p[(n,) + at] = 1
        y[(n,) + tuple(a + int(o) for a, o in zip(at, offsets[n]))] = 1
    return p, y, offsets


@pytest.mark.parametrize("second_tile", [False, True], ids=["last-of-first-tile", "first-of-second-tile"])
@pytest.mark.parametrize("nd,tau,T", [(2, 2, 4), (3, 1.5, 2)], ids=["2d", "3d"])
def test_ball_across_the_seams_of_its_tiles(nd, tau, T, second_tile):
    """One border voxel per map and entry, `pred`'s at a corner of the first tile, `target`'s at every offset of the ball's
    bounding box and one beyond: within is [1, 1] exactly inside the ball."""
    ops = _ops()
    cap = 2 if nd == 2 else 1
    p, y, offsets = _seam_maps(nd, cap, second_tile)
    inside = (offsets * offsets).sum(1) <= T
    assert 0 < int(inside.sum()) < inside.numel() and int(offsets.abs().max()) == cap + 1
    want = torch.stack([inside, inside], 1).long()
    pd, yd = p.to(DEV), y.to(DEV)
    for kw in (dict(), dict(sampling=(1.0,) * nd)):               # (the fp32 comparison: every square is exact at unit spacing)
        assert ops.surface_dice_route(p.shape[0], 2, p.shape[1:], tau, kw.get("sampling")) == "ball"
        for route in ("ball", "fields"):
            got = ops.surface_dice(pd, yd, 2, tau, route=route, **kw)
            assert bool((got.surface_voxels[:, 1] == 1).all()) and bool((got.surface_voxels[:, 0] == 0).all())
            assert torch.equal(got.within[:, 1].cpu(), want), route
            assert torch.equal(got.surface_dice[:, 1].cpu(), inside.float())
            assert bool(torch.isnan(got.surface_dice[:, 0]).all())


@pytest.mark.parametrize("K,shape", [(1, (2, 5, 7)), (4, (3, 36, 57)), (4, (2, 6, 10, 70)), (70, (1, 33, 9, 5))],
                         ids=["tiny", "2d", "3d", "3d-K70"])
def test_identities(K, shape):
    ops, M = _ops(), _M()
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    N, sp = shape[0], shape[1:]
    diagonal = sum(s * s for s in sp) ** 0.5
    for route in _routes(N, K, sp, diagonal):                     # everything is within the diagonal
        got = ops.surface_dice(pd, yd, K, diagonal, route=route)
        both = (got.surface_voxels > 0).all(-1)
        assert bool(both.any()) and torch.equal(got.within[both], got.surface_voxels[both])
        assert bool((got.within[~both] == 0).all())
        assert bool((got.surface_dice[both] == 1).all())
    last = None
    for tau in (0, 0.5, 1, 1.5, 2, 2.5, 3, 7, diagonal):            # monotone in the tolerance
        got = M.surface_dice(pd, yd, K, tau)
        assert last is None or bool((got.within >= last).all())
        last = got.within
    same = M.surface_dice(yd, yd.clone(), K, 0)                     # equal maps
    there = same.surface_voxels[..., 0] > 0
    assert bool(there.any()) and bool((same.surface_dice[there] == 1).all()) and bool(torch.isnan(same.surface_dice[~there]).all())
    assert torch.equal(same.within, same.surface_voxels)
    per_class = [(0, 1.5, 3, 2)[k % 4] for k in range(K)]           # a tolerance per class: column k is the scalar call's
    for kw in (dict(), dict(sampling=SAMPLING[len(sp)])):
        for route in ("ball", "fields"):
            for tol in (per_class, tuple(per_class), torch.tensor(per_class, dtype=torch.float64)):
                got = ops.surface_dice(pd, yd, K, tol, route=route, **kw)
                for tau in sorted(set(per_class)):
                    one = ops.surface_dice(pd, yd, K, tau, route=route, **kw)
                    cols = [k for k in range(K) if per_class[k] == tau]
                    assert _same_bits([t[:, cols].contiguous() for t in got], [t[:, cols].contiguous() for t in one])
    full = M.surface_distance_metrics(pd, yd, K)                    # against the distances
    for tau in (0, 1, 2, 3, 7):
        got = M.surface_dice(pd, yd, K, tau)
        assert torch.equal(got.surface_voxels, full.surface_voxels)
        all_within = full.max_squared <= tau * tau                 # (NaN and inf compare false)
        assert torch.equal(got.within == got.surface_voxels, all_within | (got.surface_voxels == 0))


def test_empty_borders_and_voxels_without_a_class():
    """The maps of tests/test_surface_gpu.py::test_empty_borders_and_voxels_without_a_class."""
    ops = _ops()
    y = torch.zeros(2, 5, 5, dtype=torch.int64)
    p = y.clone()
    y[0, 2, 2] = -100                       # no class: its four neighbours become border voxels of class 0
    p[0, 2, 2] = 5                          # out of range (K = 3): the same
    p[1, 1, 1] = 1                          # class 1 in pred only (entry 1); class 2 nowhere
    want = dice_of(directed_squares(p, y, 3), 2, 3, 1, True)
    for route in ("ball", "fields"):
        for kw in (dict(), dict(sampling=(1.5, 0.7))):
            got = ops.surface_dice(p.to(DEV), y.to(DEV), 3, 1 if not kw else 1.45, route=route, **kw)
            assert got.surface_voxels[0, 0].tolist() == [20, 20] and got.within[0, 0].tolist() == [20, 20]
            assert float(got.surface_dice[0, 0]) == 1.0
            assert got.surface_voxels[1, 1].tolist() == [1, 0] and got.within[1, 1].tolist() == [0, 0]
            assert float(got.surface_dice[1, 1]) == 0.0 and bool(torch.isnan(got.surface_dice[0, 1]))
            assert bool(torch.isnan(got.surface_dice[:, 2]).all()) and got.surface_voxels[:, 2].tolist() == [[0, 0], [0, 0]]
            assert got.within[:, 2].tolist() == [[0, 0], [0, 0]]
            if not kw:
                _against(got, want, "conventions " + route)


def test_runs_are_bitwise_identical_and_a_captured_graph_replays_them():
    ops = _ops()
    K, shape = 4, (3, 36, 57)
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    per_class = (0.0, 1.5, 3.0, 2.0)

    def step():
        out = ()
        for route in ("ball", "fields", None):
            out += tuple(ops.surface_dice(pd, yd, K, 2, route=route))
            out += tuple(ops.surface_dice(pd, yd, K, per_class, sampling=(1.5, 0.7), route=route))
        return out

    eager = step()
    again = step()
    assert _same_bits(eager, again)
    assert _same_bits(eager[:6], eager[6:12])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(static, eager)
    with torch.no_grad():
        pd.copy_(yd)
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(static, step())
    there = static[2][..., 0] > 0
    assert bool((static[0][there] == 1).all()) and torch.equal(static[1], static[2])


def _offset_copy(t):
    """The same values one element further into a fresh storage."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("K,shape", [(4, (3, 36, 57)), (4, (2, 6, 10, 70))], ids=["2d", "3d"])
def test_offset_and_non_contiguous_inputs_give_the_same_bits(K, shape):
    ops = _ops()
    p, y, _ = _case(K, shape)
    pd, yd = p.to(DEV), y.to(DEV)
    for route in ("ball", "fields"):
        want = ops.surface_dice(pd, yd, K, 1.5, route=route)
        assert _same_bits(ops.surface_dice(_offset_copy(pd), _offset_copy(yd), K, 1.5, route=route), want)
        pt = pd.transpose(1, 2).contiguous().transpose(1, 2)
        yt = yd.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert not pt.is_contiguous() and not yt.is_contiguous()
        assert _same_bits(ops.surface_dice(pt, yt, K, 1.5, route=route), want)


def test_tensors_on_another_device_than_the_current_one():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    M = _M()
    K, shape = 4, (3, 36, 57)
    p, y, _ = _case(K, shape)
    assert torch.cuda.current_device() == 0
    for tau in (2, (0.0, 1.5, 3.0, 40.0)):
        want = M.surface_dice(p.to(DEV), y.to(DEV), K, tau)
        got = M.surface_dice(p.to("cuda:1"), y.to("cuda:1"), K, tau)
        torch.cuda.synchronize("cuda:1")
        assert all(t.device == torch.device("cuda:1") for t in got)
        assert _same_bits(got, want)
    with pytest.raises(RuntimeError, match="same device"):
        M.surface_dice(p.to("cuda:1"), y.to(DEV), K, 2)


def test_refusals_on_the_device():
    M, ops = _M(), _ops()
    y = torch.zeros(1, 8, 8, device=DEV, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="int64"):
        M.surface_dice(y.int(), y, 2, 1)
    with pytest.raises(RuntimeError, match="int64"):
        M.surface_dice(y, y.float(), 2, 1)
    y = torch.zeros(1, 70, 130, device=DEV, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="ball"):
        ops.surface_dice(y, y, 20, 40, route="ball")
    assert float(ops.surface_dice(y, y, 20, 40).surface_dice[0, 0]) == 1.0
    y = torch.zeros(1, 2, 40000, device=DEV, dtype=torch.int64)     # a row the distance fields refuse: the ball takes it
    y[0, :, 20000:] = 1                                             # (two rows: every voxel is a border voxel)
    t = torch.zeros_like(y)
    t[0, :, 20002:] = 1
    got = M.surface_dice(y, t, 2, 2)
    assert got.surface_voxels.tolist() == [[[40000, 40004], [40000, 39996]]] and got.within.tolist() == got.surface_voxels.tolist()
    t[0, :, 20002] = 0                                              # the step three voxels away: one column of each class is too far
    got = M.surface_dice(y, t, 2, 2)
    assert got.surface_voxels.tolist() == [[[40000, 40006], [40000, 39994]]]
    assert got.within.tolist() == [[[40000, 40004], [39998, 39994]]]
    with pytest.raises(NotImplementedError, match="distance fields"):
        M.surface_dice(y, y, 2, 1000)
