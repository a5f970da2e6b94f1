"""The brute-force form of tests/morph_forms.py against the scipy.ndimage compositions it is defined by (binary_erosion with
border_value=1, binary_dilation with border_value=0, the ball as structure), the consequences of the definitions on the form, the
outcomes the constructed maps are built for, and what erosion / dilation / opening / closing do on the host: the workspace query
and the refusals of the C entry, the argument checks, the refusal of CPU tensors and the alias."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import morph_forms as M

SMALL = [(3, 36, 57), (1, 65, 129), (2, 6, 10, 70), (1, 9, 17, 129)]
IDS = ["x".join(map(str, s)) for s in SMALL]
SAMPLING = {2: (1.25, 0.5), 3: (1.5, 1.0, 0.75)}
OPS = ("erosion", "dilation", "opening", "closing")


def _structure(radius, dims, sampling):
    offsets = M.ball_offsets(radius, dims, sampling)
    reach = [max(abs(o[a]) for o, _ in offsets) for a in range(len(dims))]
    st = np.zeros([2 * r + 1 for r in reach], dtype=bool)
    for o, _ in offsets:
        st[tuple(c + r for c, r in zip(o, reach))] = True
    return st


def _scipy_sets(ndi, member, st):
    """(erosion, dilation, opening, closing) of one mask under the border rule of the definitions."""
    ero = ndi.binary_erosion(member, structure=st, border_value=1)
    dil = ndi.binary_dilation(member, structure=st, border_value=0)
    return (ero, dil, ndi.binary_dilation(ero, structure=st, border_value=0), ndi.binary_erosion(dil, structure=st, border_value=1))


@functools.lru_cache(maxsize=None)
def _blobs(K, shape):
    return M.blobs(K, shape)


@pytest.mark.parametrize("shape", SMALL, ids=IDS)
def test_form_is_the_scipy_composition_on_masks(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    x = M.percolation(shape)
    nd = len(shape) - 1
    for radius, sampling in ((1, None), (1.5, None), (1.8, None), (2, None), (2.3, SAMPLING[nd]), (5, None)):
        st = _structure(radius, shape[1:], sampling)
        want = [np.stack(t) for t in zip(*[_scipy_sets(ndi, e.numpy() != 0, st) for e in x])]
        for name, w in zip(OPS, want):
            got = M.BRUTE[name](x, radius, 2, sampling)
            assert torch.equal(got, torch.from_numpy(w.astype(np.int64))), (name, radius, sampling)


@pytest.mark.parametrize("shape", SMALL, ids=IDS)
@pytest.mark.parametrize("K", [3, 20])
def test_form_is_the_per_class_scipy_composition_on_blobs(K, shape):
    ndi = pytest.importorskip("scipy.ndimage")
    nd = len(shape) - 1
    x = M.with_odd_labels(_blobs(K, shape), K)
    for radius, sampling, background in ((1.5, None, 0), (2, None, 0), (2.3, SAMPLING[nd], 0), (5, None, 0), (2, None, 2), (2, None, -1)):
        st = _structure(radius, shape[1:], sampling)
        xs = x.numpy()
        want = {name: xs.copy() for name in OPS}
        for n in range(shape[0]):
            e = xs[n]
            claims = np.zeros(e.shape, dtype=np.int64)
            who = np.zeros(e.shape, dtype=np.int64)
            d2 = []
            classes = [k for k in range(K) if k != background]
            for k in classes:
                member = e == k
                ero, dil, opened, closed = _scipy_sets(ndi, member, st)
                want["erosion"][n][member & ~ero] = background
                want["opening"][n][member & ~opened] = background
                claims += closed & member.any()
                who[closed] = k
                dist = ndi.distance_transform_edt(~member, sampling=sampling) if member.any() else np.full(e.shape, 1e9)
                d2.append(np.round(16.0 * dist * dist) / 16.0)   # (every squared length here is a multiple of 1/16)
            take = (e == background) & (claims == 1)
            want["closing"][n][take] = who[take]
            d2 = np.stack(d2)
            nearest = np.array(classes)[np.argmin(d2, axis=0)]   # (the first minimum: the smaller class)
            r2 = np.floor(radius * radius) if sampling is None else radius * radius
            grow = (e == background) & (d2.min(axis=0) <= r2)
            want["dilation"][n][grow] = nearest[grow]
        for name in OPS:
            got = M.BRUTE[name](x, radius, K, sampling, background)
            assert torch.equal(got, torch.from_numpy(want[name])), (name, radius, sampling, background)


def test_consequences_on_the_form():
    for x, K in ((M.percolation((3, 36, 57)), 2), (M.with_odd_labels(_blobs(3, (3, 36, 57)), 3), 3), (_blobs(20, (2, 6, 10, 70)), 20)):
        for radius in (1, 1.5, 2, 5):
            is_class = (x >= 0) & (x < K) & (x != 0)
            opened = M.opening_brute(x, radius, K)
            closed = M.closing_brute(x, radius, K)
            dilated = M.dilation_brute(x, radius, K)
            eroded = M.erosion_brute(x, radius, K)
            assert torch.equal(M.opening_brute(opened, radius, K), opened)
            assert torch.equal(M.closing_brute(closed, radius, K), closed)
            assert bool((is_class & (opened == 0))[opened != x].all()) and bool((is_class & (eroded == 0))[eroded != x].all())
            assert bool((x == 0)[closed != x].all()) and bool((x == 0)[dilated != x].all())
            assert bool(((eroded == x) <= (opened == x)).all())                       # what erosion keeps, opening keeps
    for name in OPS:
        x = M.with_odd_labels(_blobs(3, (3, 36, 57)), 3)
        assert torch.equal(M.BRUTE[name](x, 0, 3), x) and torch.equal(M.BRUTE[name](x, 0.5, 3), x)
        full = torch.ones((1, 9, 11), dtype=torch.int64)
        assert torch.equal(M.BRUTE[name](full, 40, 2), full)                         # the border is no obstacle


def test_ball_sizes_and_the_gap_of_the_sampling_cases():
    assert len(M.ball_offsets(1, (9, 9))) == 5 and len(M.ball_offsets(1.5, (9, 9))) == 9 and len(M.ball_offsets(2, (9, 9))) == 13
    assert len(M.ball_offsets(5, (20, 20))) == 81 and len(M.ball_offsets(2.24, (9, 9))) == 21
    assert len(M.ball_offsets(1.5, (9, 9, 9))) == 19 and len(M.ball_offsets(1.8, (9, 9, 9))) == 27
    for shape, nd in (((6, 10, 70), 3), ((36, 57), 2)):
        assert M.smallest_relative_gap(2.3, shape, SAMPLING[nd]) > 1e-3


def test_constructed_maps_have_the_outcomes_they_are_built_for():
    for shape in ((1, 21, 41), (1, 9, 21, 41)):
        x, gap = M.gap_between_two_classes(shape)
        for radius in (1, 2, 5):
            assert int(M.closing_brute(x, radius, 3)[gap]) == 0 and int(M.dilation_brute(x, radius, 3)[gap]) == 1
        x, at = M.tie_at_25(shape)
        assert int(M.dilation_brute(x, 5, 4)[at]) == 1 and int(M.dilation_brute(x, 4.9, 4)[at]) == 0
        x, bridge = M.two_discs_and_a_bridge((1,) + shape[1:-1] + (61,))
        opened = M.opening_brute(x, 1, 2)
        assert torch.equal(opened != x, bridge) and int(bridge.sum()) > 0
        x = M.class_on_the_border(shape)
        eroded = M.erosion_brute(x, 2, 2)
        assert int(eroded[(0,) + (0,) * (len(shape) - 1)]) == 1 and int((eroded != x).sum()) > 0
        assert torch.equal(M.closing_brute(x, 3, 2), x)
        for axis in range(len(shape) - 1):
            seam = shape[1 + axis] // 2
            for radius in (1, 3):
                if seam - 1 + radius + 1 >= shape[1 + axis]:
                    continue
                x, at = M.seam_probe(shape, axis, seam, radius)
                assert int(M.erosion_brute(x, radius, 3)[at]) == 0
                x, at = M.seam_probe(shape, axis, seam, radius + 1)
                assert int(M.erosion_brute(x, radius, 3)[at]) == 1


def _address(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_workspace_query_and_host_refusals_of_the_c_entry():
    from advchain_amd import _lib
    lib = _lib.load()
    for N, K, sp in ((3, 2, (36, 57)), (2, 40, (6, 10, 70)), (1, 1, (1, 1)), (1, 3, (2049, 1))):
        V, d = int(np.prod(sp)), _lib.dims_array(sp)
        assert lib.advchain_morph_workspace(0, N, K, len(sp), d) == N * V
        assert lib.advchain_morph_workspace(1, N, K, len(sp), d) == 2 * N * V
        assert lib.advchain_morph_workspace(2, N, K, len(sp), d) == N * V * (2 + K)
        assert lib.advchain_morph_workspace(3, N, K, len(sp), d) == N * V * (2 + K) + (N * K * V + 3) // 4
        for op in (0, 1):                                     # one field whatever K is
            assert lib.advchain_morph_workspace(op, N, 2, len(sp), d) == lib.advchain_morph_workspace(op, N, 40, len(sp), d)
        assert lib.advchain_morph_workspace(-1, N, K, len(sp), d) == -1 and lib.advchain_morph_workspace(4, N, K, len(sp), d) == -1
    dims = _lib.dims_array((36, 57))
    # refused exactly where advchain_signed_maps_workspace is
    cases = [(0, 2, 2, dims), (1, 0, 2, dims), (1, 65536, 2, dims), (1, 2, 1, dims), (1, 2, 4, dims), (1, 2, 2, None),
             (1, 2, 2, _lib.dims_array((0, 5))), (1, 2, 2, _lib.dims_array((32768, 2))), (1, 2, 2, _lib.dims_array((8193, 4))),
             (1, 2, 2, _lib.dims_array((8192, 32767))), (1, 2, 3, _lib.dims_array((8193, 2, 2))), (2 ** 41, 2, 2, dims),
             (1, 2, 2, _lib.dims_array((8192, 4))), (1, 2, 2, _lib.dims_array((4, 32767))), (7, 65535, 3, _lib.dims_array((3, 8192, 5)))]
    refused = 0
    for N, K, nd, d in cases:
        signed = lib.advchain_signed_maps_workspace(N, K, nd, d)
        for op in range(4):
            assert (lib.advchain_morph_workspace(op, N, K, nd, d) < 0) == (signed < 0), (op, N, K, nd)
        refused += signed < 0
    assert refused == len(cases) - 3

    # host memory stands in for the buffers: every call below is refused before anything is launched
    V = 36 * 57
    x, out = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
    ws = np.zeros(8 * V, dtype=np.int32)
    X, O, S = _address(x), _address(out), _address(ws)
    names = ["labels", "sampling", "radius", "op", "out", "workspace", "N", "K", "background", "ndim", "dims", "stream"]
    good = [X, None, 2.0, 0, O, S, 1, 2, 0, 2, dims, None]

    def refused_call(code=-1, **kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        rc = lib.advchain_morph(*args)
        assert rc == code and b"morph" in lib.advchain_last_error(), (kw, rc, lib.advchain_last_error())

    refused_call(labels=None)
    refused_call(out=None)
    refused_call(workspace=None)
    refused_call(dims=None)
    for op in (-1, 4, 17):
        refused_call(op=op)
    for r in (-1.0, -1e-9, float("nan"), float("inf"), -float("inf")):
        refused_call(radius=r)
    refused_call(out=X)
    for K in (0, -1, 65536):
        refused_call(K=K)
    refused_call(N=0)
    refused_call(ndim=1)
    refused_call(ndim=4)
    refused_call(dims=_lib.dims_array((0, 5)))
    for bad in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (float("inf"), 1.0)):
        refused_call(sampling=_lib.float_array(list(bad)))
    refused_call(code=-2, dims=_lib.dims_array((32768, 2)))
    refused_call(code=-2, dims=_lib.dims_array((8193, 4)))
    refused_call(code=-2, dims=_lib.dims_array((8192, 32767)))


def test_host_side_checks_raise_value_errors():
    import advchain.common.postprocess as P
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    y3 = torch.zeros(1, 4, 8, 8, dtype=torch.int64)
    for fn in (P.erosion, P.dilation, P.opening, P.closing):
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros(8, 8, dtype=torch.int64), 1, 2)
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros(1, 1, 2, 8, 8, dtype=torch.int64), 1, 2)
        with pytest.raises(ValueError, match="3-D"):
            fn([[[0]]], 1, 2)
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(0, 8, 8, dtype=torch.int64), 1, 2)
        for r in (-1, -0.5, float("nan"), float("inf"), True, None, "2", 1 + 0j):
            with pytest.raises(ValueError, match="radius"):
                fn(y, r, 2)
        with pytest.raises(ValueError, match=fn.__name__):
            fn(y, -1, 2)
        with pytest.raises(ValueError, match="background"):
            fn(y, 1, 2, background=0.0)
        with pytest.raises(ValueError, match="background"):
            fn(y, 1, 2, background=True)
        for K in (0, 2.0, True, None):
            with pytest.raises(ValueError, match="num_classes"):
                fn(y, 1, K)
        for s in ((1.0,), (1.0, 1.0, 1.0), (0.0, 1.0), (1.0, float("inf")), 2.0):
            with pytest.raises(ValueError, match="sampling"):
                fn(y, 1, 2, sampling=s)
        with pytest.raises(ValueError, match="sampling"):
            fn(y3, 1, 2, sampling=(1.0, 1.0))


def test_cpu_tensors_are_refused_and_the_alias():
    import advchain.common.postprocess as P
    import advchain_amd.common.postprocess as P2
    from advchain_amd import ops
    from advchain_amd._lib import AdvchainHipError
    assert P is P2
    assert ops.MORPH_TILE == {2: (None, 64), 3: (None, None, 64)}
    y = torch.zeros(2, 8, 8, dtype=torch.int64)
    for fn in (P.erosion, P.dilation, P.opening, P.closing):
        for kw in ({}, {"sampling": (1.0, 2.0)}, {"background": -1}):
            with pytest.raises(AdvchainHipError):
                fn(y, 1.5, 2, **kw)
