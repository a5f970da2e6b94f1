"""Host side of what completes the deterministic mode (include/advchain_hip.h): the bicubic backward twin
(advchain_grid_sample_bicubic2d_bwd_det), the step-count norm in a fixed order (advchain_tp_interp_sumsq_ordered) and the
consistency loss with its sums in a fixed order (the *_fwd_ord entries and advchain_consistency_finish_ord).  Symbols, the size
queries against their documented formulas, the argument checks, and the premise of the GPU tests of the loss value: for the
inputs they use, the order in which workgroup partials are added changes the bits of an fp32 sum.  No kernel is launched.

tests/test_det_complete_gpu.py takes its shapes and inputs from here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from advchain_amd import _lib
from tests.helpers import rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("advchain_bicubic2d_det_workspace", "advchain_grid_sample_bicubic2d_bwd_det", "advchain_tp_interp_sumsq_partials",
       "advchain_tp_interp_sumsq_ordered", "advchain_consistency_fwd_partials", "advchain_consistency_fwd_ord",
       "advchain_consistency_fused_fwd_partials", "advchain_consistency_fused_fwd_ord", "advchain_consistency_wide_fwd_partials",
       "advchain_consistency_wide_fwd_ord", "advchain_consistency_lp_fwd_partials", "advchain_consistency_lp_fwd_ord",
       "advchain_consistency_finish_ord")


@pytest.fixture(scope="module")
def lib():
    from advchain_amd.build import build_library
    build_library()
    return _lib.load()


def test_new_entries_are_declared_exported_and_prototyped(lib):
    assert lib.advchain_version() >= 180
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advchain_hip.h")).read(), flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared in the header"
        assert hasattr(cdll, name), name + " is not exported"
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name + " has no prototype"


# ---- geometry: the launches of every forward family, mirrored from csrc/loss*.hip ---------------------------------------------

def cdiv(a, b):
    return -(-a // b)


def dims3(dims):
    return (1,) + tuple(dims) if len(dims) == 2 else tuple(dims)


def march4_wgs(N, dims):
    """k_loss_fused_fwd4 / k_edge_fwd_march4: a lane owns 4 x, a group of S2/4 lanes a row, strips of `mlen` rows."""
    s0, s1, s2 = dims3(dims)
    per_wave = 64 // (s2 // 4)
    mlen = 2
    for m in (8, 4):
        if N * s0 * cdiv(s1, m) // per_wave >= 1024:
            mlen = m
            break
    return cdiv(cdiv(s1, mlen) * s0, 4 * per_wave) * N


def z3_wgs(N, dims):
    """k_loss_fused_fwd3d_z: tiles of 4 x (64 / (S2 / 4)) - 2 own rows, chunks of planes halved while the launch is small."""
    s0, s1, s2 = dims
    nyt = cdiv(s1, 4 * (64 // (s2 // 4)) - 2)
    zc = s0
    while zc > 4 and N * nyt * cdiv(s0, zc) < 768:
        zc = (zc + 1) // 2
    return nyt * cdiv(s0, zc) * N


def tile_wgs(N, dims):
    """k_wide_edge / k_lp_edge: tiles of 64 x 8 (2D) or 32 x 8 x 4 (3D) voxels."""
    s0, s1, s2 = dims3(dims)
    return (cdiv(s2, 64) * cdiv(s1, 8) if len(dims) == 2 else cdiv(s2, 32) * cdiv(s1, 8) * cdiv(s0, 4)) * N


def launches(family, N, K, dims, mask_ch):
    """Workgroups of every launch of the family's forward ('mse' + 'contour' + 'kl', 16-byte aligned tensors)."""
    s0, s1, s2 = dims3(dims)
    V = s0 * s1 * s2
    if family == "fused":
        return [march4_wgs(N, dims) if len(dims) == 2 else z3_wgs(N, dims)]
    if family == "three":
        stats = cdiv(V // 4, 256) * N if (V % 4 == 0 and 2 <= K <= 5) else cdiv(V, 256) * N
        if mask_ch <= 1 and 2 <= K <= 5 and s2 % 4 == 0 and s2 // 4 <= 64:
            edge = march4_wgs(N, dims)
        elif mask_ch <= 1 and 2 <= K <= 5 and s2 % 64 == 0:
            edge = cdiv((s2 >> 6) * cdiv(s1, 8) * s0, 4) * N
        else:
            edge = cdiv(V, 256) * N
        return [stats, edge]
    assert family in ("wide", "lp", "cw")
    return [cdiv(cdiv(V, 4), 256) * N, tile_wgs(N, dims)]


def query(lib, family, N, K, dims, mask_ch, has_mask=1):
    d = _lib.dims_array(dims)
    nd = len(dims)
    if family == "fused":
        return lib.advchain_consistency_fused_fwd_partials(N, K, nd, d, has_mask, mask_ch, 1, 1)
    if family == "three":
        return lib.advchain_consistency_fwd_partials(N, K, nd, d, mask_ch, 1, 1)
    if family == "wide":
        return lib.advchain_consistency_wide_fwd_partials(N, K, nd, d, 1, 1)
    return lib.advchain_consistency_lp_fwd_partials(N, K, nd, d, 1)


def _smallest(family, N, K, tail, mask_ch, lead=None):
    """The smallest H (2D: (H,) + tail; 3D: (lead, H) + tail) at which EVERY launch of the family has at least 130 workgroups:
    at least two of them add into each of the 64 slots of the default mode."""
    for H in range(1, 5000):
        dims = ((H,) if lead is None else (lead, H)) + tail
        if min(launches(family, N, K, dims, mask_ch)) >= 130:
            return dims
    raise AssertionError("no shape")


# name -> (family, N, K, dims, mask channels (K: per class), storage of (prediction, reference), class weights)
# A mask of one channel where the kernel under test takes no other: the fused form and the marching edge kernel are reached with
# at most one mask channel (a per-class mask sends the call to the generic three-kernel form, which "three_k8" covers).
def _cases():
    f32, b16 = torch.float32, torch.bfloat16
    out = {}
    out["fused_k4"] = ("fused", 2, 4, _smallest("fused", 2, 4, (256,), 1), 1, (f32, f32), None)
    out["fused_k2_3d"] = ("fused", 2, 2, _smallest("fused", 2, 2, (128,), 1, lead=8), 1, (f32, f32), None)
    out["march_k5"] = ("three", 2, 5, _smallest("three", 2, 5, (256,), 1), 1, (f32, f32), None)
    out["three_k8"] = ("three", 2, 8, _smallest("three", 2, 8, (128,), 8), 8, (f32, f32), None)
    out["wide_k20"] = ("wide", 2, 20, _smallest("wide", 2, 20, (256,), 20), 20, (f32, f32), None)
    out["wide_k20_3d"] = ("wide", 2, 20, _smallest("wide", 2, 20, (128,), 20, lead=8), 20, (f32, f32), None)
    out["lp_bf16_k4"] = ("lp", 2, 4, _smallest("lp", 2, 4, (256,), 4), 4, (b16, b16), None)
    out["cw_k4"] = ("cw", 2, 4, _smallest("cw", 2, 4, (256,), 4), 4, (f32, f32), (0.25, 2.0, 0.0, 1.5))
    return out


LOSS_CASES = _cases()
TYPES, WEIGHTS = ["mse", "contour", "kl"], [0.7, 0.5, 1.3]


def order_mask(N, ch, dims):
    """Ones, with a band of rows scaled by 1e4 and another by 1e-3 (per class the bands move by a tenth of the height): the
    terms of the sums then span many orders of magnitude, so the order workgroup partials are added in shows in the bits."""
    m = torch.ones((N, ch) + tuple(dims))
    H = dims[-2]
    for c in range(ch):
        rows = (torch.arange(H) + c * H // 10) % H
        scale = torch.ones(H)
        scale[rows[: H // 3]] = 1e4
        scale[rows[2 * H // 3:]] = 1e-3
        m[:, c] *= scale.reshape(H, 1)
    return m.contiguous()


def loss_inputs(name):
    """(prediction, reference, mask, class weights) of a case, CPU tensors in the storage types of the case."""
    family, N, K, dims, mch, (pt, rt), cw = LOSS_CASES[name]
    pred = (rand((N, K) + tuple(dims), 911) * 3).to(pt)
    ref = (rand((N, K) + tuple(dims), 912) * 3).to(rt)
    return pred, ref, order_mask(N, mch, dims), cw


def oracle_value(pred, ref, mask, cw, types=TYPES, weights=WEIGHTS):
    """The oracle (class weights: tests/test_class_weights_cpu.weighted_loss) in fp32 on the exact upcast of the operands."""
    from oracle import advchain_oracle as O
    from tests.test_class_weights_cpu import weighted_loss
    with torch.no_grad():
        if cw is None:
            return float(O.consistency_loss(pred.float(), ref.float(), types, weights, mask=mask))
        return float(weighted_loss(pred.float(), ref.float(), types, weights, cw, mask=mask))


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_loss_shapes_have_130_workgroups_in_every_launch_and_the_queries_agree(lib, name):
    family, N, K, dims, mch, _, _ = LOSS_CASES[name]
    wgs = launches(family, N, K, dims, mch)
    assert min(wgs) >= 130, (name, dims, wgs)
    got = query(lib, family, N, K, dims, mch)
    assert got == max(wgs), (name, dims, got, wgs)
    # the smallest such shape along its height
    smaller = tuple(dims[:-2]) + (dims[-2] - 1, dims[-1])
    assert min(launches(family, N, K, smaller, mch)) < 130, (name, smaller)


def test_loss_queries_on_other_shapes_and_bad_arguments(lib):
    d = _lib.dims_array
    # unaligned tensors: one voxel per thread in the statistics kernels of the K <= 16 families, no 16-byte marching form; the
    # run-time-K statistics kernel gives a thread 4 voxels at any alignment (the wide query ignores `aligned16`)
    assert lib.advchain_consistency_wide_fwd_partials(2, 20, 2, d((12, 64)), 1, 0) == max(cdiv(cdiv(12 * 64, 4), 256), 1 * 2) * 2
    assert lib.advchain_consistency_wide_fwd_partials(2, 20, 2, d((12, 64)), 0, 1) == cdiv(cdiv(12 * 64, 4), 256) * 2
    assert lib.advchain_consistency_wide_fwd_partials(2, 20, 2, d((37, 52)), 0, 0) == cdiv(cdiv(37 * 52, 4), 256) * 2
    assert lib.advchain_consistency_fwd_partials(3, 8, 2, d((37, 52)), 8, 1, 1) == cdiv(37 * 52, 256) * 3
    assert lib.advchain_consistency_fwd_partials(3, 5, 2, d((37, 52)), 1, 1, 0) == cdiv(37 * 52, 256) * 3
    assert lib.advchain_consistency_lp_fwd_partials(2, 4, 3, d((3, 5, 7)), 1) == max(cdiv(cdiv(105, 4), 256), 1 * 1 * 1) * 2
    # the fused form declines: more than 4 classes, a per-class mask, unaligned tensors, 3D rows that are too long
    assert lib.advchain_consistency_fused_fwd_partials(2, 5, 2, d((64, 64)), 0, 1, 1, 1) == -2
    assert lib.advchain_consistency_fused_fwd_partials(2, 4, 2, d((64, 64)), 1, 4, 1, 1) == -2
    assert lib.advchain_consistency_fused_fwd_partials(2, 4, 2, d((64, 64)), 0, 1, 1, 0) == -2
    assert lib.advchain_consistency_fused_fwd_partials(2, 4, 3, d((8, 8, 256)), 0, 1, 1, 1) == -2
    assert lib.advchain_consistency_fused_fwd_partials(2, 4, 2, d((64, 64)), 0, 1, 1, 1) == march4_wgs(2, (64, 64))
    for bad in (lib.advchain_consistency_fwd_partials(2, 17, 2, d((8, 8)), 1, 1, 1),
                lib.advchain_consistency_fwd_partials(2, 4, 2, None, 1, 1, 1),
                lib.advchain_consistency_wide_fwd_partials(-1, 20, 2, d((8, 8)), 1, 1),
                lib.advchain_consistency_lp_fwd_partials(2, 0, 2, d((8, 8)), 1),
                lib.advchain_consistency_fused_fwd_partials(2, 4, 4, d((8, 8, 8, 8)), 0, 1, 1, 1)):
        assert bad == -1


@pytest.mark.parametrize("N,C,dims", [(2, 3, (9, 11)), (3, 1, (5, 5)), (1, 7, (33, 47)), (5, 2, (64, 64))])
def test_bicubic_workspace_is_the_documented_formula(lib, N, C, dims):
    """int32 elements: the int64 image (2 N C H W) plus one maximum per batch entry, padded to a multiple of four.  (2, 3,
    (9, 11)) and (3, 1, (5, 5)): an odd C H W, so the image of the second entry starts 8 bytes off a 16-byte boundary."""
    want = 2 * N * C * dims[0] * dims[1] + ((N + 3) // 4) * 4
    was = lib.advchain_get_deterministic()
    try:
        for on in (0, 1):
            lib.advchain_set_deterministic(on)
            assert lib.advchain_bicubic2d_det_workspace(N, C, _lib.dims_array(dims)) == want
    finally:
        lib.advchain_set_deterministic(was)
    assert want % 2 == 0          # the maxima follow the image on an 8-byte boundary


def test_bicubic_workspace_and_twin_check_their_arguments(lib):
    d = _lib.dims_array
    assert lib.advchain_bicubic2d_det_workspace(2, 0, d((8, 8))) < 0
    assert lib.advchain_bicubic2d_det_workspace(-1, 3, d((8, 8))) < 0
    assert lib.advchain_bicubic2d_det_workspace(2, 3, None) < 0
    P = ctypes.c_void_p(64)

    def twin(gout=P, inp=P, grid=P, gin=P, ggrid=P, ws=P, N=2, C=3, idims=(9, 11), odims=(8, 8), padding=0):
        return lib.advchain_grid_sample_bicubic2d_bwd_det(gout, inp, grid, gin, ggrid, ws, N, C, d(idims), d(odims), padding, None)
    for kw in (dict(gout=None), dict(inp=None), dict(grid=None), dict(gin=None, ggrid=None), dict(ws=None), dict(padding=3),
               dict(padding=-1), dict(C=0), dict(N=70000), dict(idims=(0, 4))):
        assert twin(**kw) < 0, kw
        assert b"grid_sample_bicubic2d_bwd_det" in lib.advchain_last_error(), kw
    assert twin(N=0) == 0 and twin(N=0, gin=None, ws=None) == 0


@pytest.mark.parametrize("S,planes", [((16, 16, 8), 6), ((1, 33, 40), 4), ((5, 64, 7), 3), ((128, 128, 64), 12)])
def test_step_count_partials_is_the_documented_formula(lib, S, planes):
    assert lib.advchain_tp_interp_sumsq_partials(_lib.dims_array(S), planes) == cdiv(S[1], 32) * S[0] * planes


def test_step_count_entries_check_their_arguments(lib):
    d = _lib.dims_array
    assert lib.advchain_tp_interp_sumsq_partials(None, 2) < 0
    assert lib.advchain_tp_interp_sumsq_partials(d((4, 0, 4)), 2) < 0
    assert lib.advchain_tp_interp_sumsq_partials(d((4, 4, 4)), -1) < 0
    P = ctypes.c_void_p(64)
    S = d((4, 4, 4))
    assert lib.advchain_tp_interp_sumsq_ordered(P, P, P, S, S, S, 2, 3, None, P, None) < 0
    assert b"tp_interp_sumsq_ordered" in lib.advchain_last_error()
    assert lib.advchain_tp_interp_sumsq_ordered(P, P, P, S, S, S, 2, 3, P, None, None) < 0
    assert lib.advchain_tp_interp_sumsq_ordered(None, P, P, S, S, S, 2, 3, P, P, None) < 0


def test_ordered_loss_entries_check_their_arguments(lib):
    d = _lib.dims_array((8, 8))
    P = ctypes.c_void_p(64)
    counts = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    coef = _lib.float_array((1.0, 1.0, 1.0, 1.0))
    # no counts / no stride
    assert lib.advchain_consistency_fwd_ord(P, P, None, P, P, P, P, 4, None, 2, 8, 2, d, 1, 0, 1, 1, None) < 0
    assert b"consistency_fwd_ord" in lib.advchain_last_error()
    assert lib.advchain_consistency_fused_fwd_ord(P, P, None, P, P, 0, counts, 2, 4, 2, d, 1, 0, 1, 1, None) < 0
    assert lib.advchain_consistency_wide_fwd_ord(P, P, None, P, P, P, 0, counts, 2, 20, 2, d, 1, 0, 1, 1, None) < 0
    assert lib.advchain_consistency_lp_fwd_ord(P, 0, P, 0, None, P, P, P, 4, None, 2, 4, 2, d, 1, 0, 1, 1, None, None) < 0
    assert b"consistency_lp_fwd_ord" in lib.advchain_last_error()
    # a buffer smaller than a launch is refused before anything is enqueued (2 x 8 x 8 voxels: 2 workgroups)
    assert lib.advchain_consistency_fwd_ord(P, P, None, P, P, P, P, 1, counts, 2, 8, 2, d, 1, 0, 1, 1, None) < 0
    assert b"partial buffer" in lib.advchain_last_error()
    assert lib.advchain_consistency_wide_fwd_ord(P, P, None, P, P, P, 1, counts, 2, 20, 2, d, 1, 0, 1, 1, None) < 0
    assert lib.advchain_consistency_lp_fwd_ord(P, 0, P, 0, None, P, P, P, 1, counts, 2, 4, 2, d, 1, 0, 1, 1, None, None) < 0
    assert b"partial buffer" in lib.advchain_last_error()
    # an empty batch: nothing enqueued, every row empty
    assert lib.advchain_consistency_fwd_ord(P, P, None, P, P, P, P, 4, counts, 0, 8, 2, d, 1, 0, 1, 1, None) == 0
    assert list(counts) == [0, 0, 0, 0]
    # the finisher: null pointers, a count above the stride
    assert lib.advchain_consistency_finish_ord(None, 4, counts, coef, P, P, None) < 0
    assert lib.advchain_consistency_finish_ord(P, 4, None, coef, P, P, None) < 0
    assert lib.advchain_consistency_finish_ord(P, 0, counts, coef, P, P, None) < 0
    over = (ctypes.c_int32 * 4)(1, 5, 0, 0)
    assert lib.advchain_consistency_finish_ord(P, 4, over, coef, P, P, None) < 0
    assert b"consistency_finish_ord" in lib.advchain_last_error()


def test_new_ops_functions_refuse_cpu_tensors():
    from advchain_amd import bands, ops
    tables = bands.upsample_tables([4, 4, 4], [16, 16, 8], torch.device("cpu"))
    with pytest.raises(_lib.AdvchainHipError):
        ops.field_sumsq(torch.rand(2, 3, 4, 4, 4), tables, 3)
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        with pytest.raises(_lib.AdvchainHipError):
            ops.field_sumsq(torch.rand(2, 3, 4, 4, 4), tables, 3)
        with pytest.raises(_lib.AdvchainHipError):
            ops.grid_sample(torch.rand(1, 1, 5, 5), torch.rand(1, 2, 4, 4), "bicubic", "zeros")
        with pytest.raises(_lib.AdvchainHipError):
            ops.consistency_sums(torch.rand(1, 4, 8, 8), torch.rand(1, 4, 8, 8), None, (1.0, 0.5, 0.5, 1.0))
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("name", ["fused_k4", "three_k8"])
def test_the_order_of_the_partials_shows_in_an_fp32_sum(name):
    """The premise of the GPU tests of the loss value.  The 'mse' term of the oracle, per 256-voxel tile as a workgroup of the
    generic kernel sees it, summed in fp32 over the tiles in two orders (ascending; the 64 slots of the default mode filled
    round-robin and then added up): different bits.  So a value that is equal over repeated evaluations is not equal by
    accident of the input."""
    pred, ref, mask, _ = loss_inputs(name)
    with torch.no_grad():
        e = (torch.softmax(pred.float(), 1) * mask - torch.softmax(ref.float(), 1) * mask) ** 2
    N, K = e.shape[:2]
    V = e[0, 0].numel()
    per_voxel = e.reshape(N, K, V).sum(1)                              # a thread's sum over the classes
    pad = cdiv(V, 256) * 256 - V
    tiles = torch.nn.functional.pad(per_voxel, (0, pad)).reshape(N, -1, 256).sum(2).reshape(-1).numpy().astype(np.float32)
    assert tiles.size >= 130
    ascending = np.float32(0)
    for t in tiles:
        ascending = np.float32(ascending + t)
    slots = np.zeros(64, np.float32)
    for i, t in enumerate(tiles[::-1]):                                # another arrival order
        slots[i % 64] = np.float32(slots[i % 64] + t)
    slotted = np.float32(0)
    for s in slots:
        slotted = np.float32(slotted + s)
    assert ascending.tobytes() != slotted.tobytes(), (float(ascending), float(slotted))
    assert abs(float(ascending) - float(slotted)) < 2e-5 * float(ascending)
