"""Autograd-composable operators backed by the HIP kernels (C ABI via ctypes).

Every operator requires CUDA(ROCm) fp32 tensors and the built ``libadvchain_hip.so``; there is no
PyTorch / CPU fallback -- a CPU tensor or a missing library raises.  PyTorch is used for device
memory (``torch.empty``), the current stream and the autograd tape only.
"""
import collections
import ctypes
import functools
import math
import numbers
import struct

import numpy as np
import torch

from . import _lib
from .bands import gaussian_weights_1d

_INTERP = {"bilinear": 0, "trilinear": 0, "linear": 0, "nearest": 1, "bicubic": 2}
_PAD = {"zeros": 0, "border": 1, "reflection": 2}
_GAUSS9 = _lib.float_array(gaussian_weights_1d(1.0))
_GAUSS9_CACHE = {}


GENERIC_MAX_TAPS = 129


def gauss9(sigma, taps=None):
    """The tap weights of the Gaussian for `sigma` (ctypes array).  The reference sizes its window as
    max(gaussian_ks, 2 * int(4 sigma + 0.5) + 1) taps (adv_morph.py:393-398; `taps`, default the rule alone): 9 for
    0.875 <= sigma < 1.125 with the default gaussian_ks = 5 -- the fast kernels; any other window runs
    advchain_gauss_axis_generic (raw_gauss; no fused prologue / epilogue there)."""
    sigma = float(sigma)
    if taps is None:
        taps = 2 * int(4 * sigma + 0.5) + 1
    taps = int(taps)
    if sigma == 1.0 and taps == 9:
        return _GAUSS9
    w = _GAUSS9_CACHE.get((sigma, taps))
    if w is None:
        if not sigma > 0.0:
            raise ValueError("Gaussian smoothing needs sigma > 0, got %r" % (sigma,))
        if taps % 2 == 0:
            # (the reference's conv then pads k // 2 on both sides and returns a field one voxel larger per axis)
            raise NotImplementedError("Gaussian smoothing with an even window (%d taps) is not implemented" % taps)
        if taps > GENERIC_MAX_TAPS:
            raise NotImplementedError("Gaussian smoothing with sigma=%g needs a %d-tap window (at most %d)"
                                      % (sigma, taps, GENERIC_MAX_TAPS))
        if len(_GAUSS9_CACHE) > 16:
            _GAUSS9_CACHE.clear()
        w = _GAUSS9_CACHE[(sigma, taps)] = _lib.float_array(gaussian_weights_1d(sigma, taps))
    return w


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    # torch.cuda.current_stream() builds a Stream object through five Python layers (~10 us; ~300 calls per solver
    # call): ask the C layer for the raw handle of the current stream of the current device instead
    if _raw_stream is not None and _raw_device is not None:
        return ctypes.c_void_p(_raw_stream(_raw_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_STREAM_OBJ = {}


def _stream_obj():
    """The current stream of the current device as a torch Stream object (Event.record() without an argument builds one
    through five Python layers on every call): cached per device, rebuilt when the raw handle has changed."""
    if _raw_stream is None or _raw_device is None:
        return torch.cuda.current_stream()
    dev = _raw_device()
    s = _STREAM_OBJ.get(dev)
    if s is None or s.cuda_stream != _raw_stream(dev):
        s = _STREAM_OBJ[dev] = torch.cuda.current_stream()
    return s


def _require_device(t, name):
    """t, a device tensor, or AdvchainHipError."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.AdvchainHipError("%s must be a CUDA/ROCm tensor: the advchain_amd kernels have no CPU path" % name)
    return t


def _dev(t, name="tensor"):
    _require_device(t, name)
    if t.dtype != torch.float32:
        raise _lib.AdvchainHipError("%s must be float32, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _same_device(*tensors):
    """All operands of one launch must live on one GPU (raw pointers carry no device)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("Expected all tensors to be on the same device, but found at least two devices, "
                               "%s and %s!" % (dev, t.device))


def _on_tensor_device(fn):
    """Run `fn` with the first tensor argument's GPU as the current device: `_stream()` hands the kernels the current
    stream of the CURRENT device, so an operator called on cuda:1 tensors while cuda:0 is current would otherwise
    launch on device 0's stream against device-1 pointers.  The common case (already current) costs one C call.
    (Autograd runs a Function's backward on the device thread of its forward: only entry points need the guard.)"""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        for a in args:
            if isinstance(a, (tuple, list)) and a and isinstance(a[0], torch.Tensor):
                a = a[0]
            if isinstance(a, torch.Tensor):
                if a.is_cuda:
                    cur = _raw_device() if _raw_device is not None else torch.cuda.current_device()
                    if a.device.index != cur:
                        with torch.cuda.device(a.device):
                            return fn(*args, **kwargs)
                break
        return fn(*args, **kwargs)
    return guarded


def interp_code(interp):
    if interp not in _INTERP:
        raise NotImplementedError("interpolation mode %r is not implemented by the HIP sampler "
                                  "(supported: bilinear/trilinear, nearest, bicubic (2D))" % (interp,))
    return _INTERP[interp]


def pad_code(padding_mode):
    if padding_mode not in _PAD:
        raise NotImplementedError("padding_mode %r" % (padding_mode,))
    return _PAD[padding_mode]


# ------------------------------------------------------------------------------------------------
# raw (non-autograd) wrappers: one C-ABI call each
# ------------------------------------------------------------------------------------------------
def _hint_bits(disp):
    """Displacement estimate (voxels) -> the hint bits 8..15 of an int argument (0 = unknown); see include/advchain_hip.h."""
    if disp is None or not disp == disp or disp < 0:
        return 0
    return min(int(disp) + 1, 255) << 8


def _fine_bits(disp):
    """Displacement estimate in 1/1024 voxel (at least 1 when known, 0 = unknown): bits 8.. of a chain hint."""
    if disp is None or not disp == disp or disp < 0:
        return 0
    return max(1, min(int(disp * 1024.0) + 1, (1 << 22) - 1))


def raw_grid_sample_fwd(inp, grid, interp, padding, clamp_grid, disp_hint=None):
    N, C = inp.shape[:2]
    nd = inp.dim() - 2
    odims = grid.shape[2:]
    out = torch.empty((N, C) + tuple(odims), device=inp.device, dtype=torch.float32)
    _lib.check(_lib.load().advchain_grid_sample_fwd(_ptr(inp), _ptr(grid), _ptr(out), N, C, nd,
                                                    _lib.dims_array(inp.shape[2:]), _lib.dims_array(odims),
                                                    interp, padding, int(clamp_grid) | _hint_bits(disp_hint), _stream()),
               "grid_sample_fwd")
    return out


def raw_grid_sample_fwd_ride(inp, grid, ride, interp, padding, clamp_grid, nonzero, disp_hint=None):
    """raw_grid_sample_fwd for `inp` and a one-channel rider through the same grid (one launch in 2D)."""
    N, C = inp.shape[:2]
    nd = inp.dim() - 2
    odims = tuple(grid.shape[2:])
    out = torch.empty((N, C) + odims, device=inp.device, dtype=torch.float32)
    rout = torch.empty((N, 1) + odims, device=inp.device, dtype=torch.float32)
    _lib.check(_lib.load().advchain_grid_sample_fwd_ride(_ptr(inp), _ptr(grid), _ptr(out), _ptr(ride), _ptr(rout), N, C, nd,
                                                         _lib.dims_array(inp.shape[2:]), _lib.dims_array(odims), interp, padding,
                                                         int(clamp_grid) | _hint_bits(disp_hint), int(bool(nonzero)), _stream()),
               "grid_sample_fwd_ride")
    return out, rout


DISP_SLOTS = 4096     # ADVCHAIN_DISP_SLOTS of include/advchain_hip.h
ADAPTIVE_HALO = True  # measure the displacement in forward and size the backward halos from it
PAIR_FIELDS = True    # a solver step integrates field(+v) and field(-v) as one batch
TILED_SCATTER = True  # LDS-tiled owner-computes scatter (False: global-atomic kernels; for A/B tests)
FUSED_LOSS = True     # the consistency loss straight from the logits (no P / D intermediates); False: A/B tests
WIDE_LOSS_MIN_K = 17  # class counts from here on take the run-time-K loss kernels (loss_lp.hip: any K < 65536, no P / D); below:
                      # the K <= 16 kernels of loss.hip, unchanged.  Tests and tools lower it to compare the two implementations
SKELETON_FUSED_MAX_ITERATIONS = 4   # ADVCHAIN_SKELETON_FUSED_MAX: soft skeletons of up to this many iterations can run as one LDS-tile
                      # launch (seg_skeleton.hip); beyond, and for volumes, level by level with the same bits
SKELETON_MAX_ITERATIONS = 32        # ADVCHAIN_SKELETON_MAX_ITERATIONS
REF_GRAD_REG_MAX_K = 4  # the gradient w.r.t. the reference (loss_ref.hip) keeps K = 2..this many classes in registers (at most 4);
                      # 0: the run-time-K form for every class count.  Tests and tools lower it to compare the two forms
FUSE_2D = True        # the leading sub-pixel squarings of a 2D chain in one launch (expo_fused2d.hip); False: A/B tests
COMPOSITE = True      # a paired 2D DemonsCompose direction as ONE C call (demons_compose.cpp: same launches); False: A/B tests
RIDE_MASK = True      # the solver's validity mask rides through the data's warps (one launch for both); False: A/B tests
RIDE_INTERPS = ("bilinear", "trilinear", "linear", "nearest")
WINDOW_STAGED = True  # deterministic mode, 2D: the window scatter stages its windows and a merge kernel sums them (no int64 image:
                      # scatter_window.hip); False: the int64 twin, bit for bit the same results.  Read at every call: tests and
                      # tools compare the two forms in one process
WINDOW_STAGED_CHANNELS = (1, 2, 4)   # the channel counts that take the staged form (measured: profiles/r14/window_staged)
BIAS_REDUCED = True   # the bias backward reduces its rows along x itself (advchain_bias_field_bwd_reduced); False: the two launches
GAUSS_XY_LANES = True  # raw_gauss calls advchain_gauss_xy (the lane form for rows of 256 voxels); False: advchain_gauss_xy_staged,
                      # the same bits.  Read at every call (the composite entries of demons_compose.cpp always call the former)

# advchain_last_bwd_route (include/advchain_hip.h: ADVCHAIN_ROUTE_*)
BWD_ROUTES = ("none", "general", "rows", "gather", "march", "window_float", "window_int64", "window_staged", "tiled")


def last_bwd_route():
    """Which formulation the last raw_grid_sample_bwd of this thread ended in (a host-side note of the launcher)."""
    return BWD_ROUTES[_lib.load().advchain_last_bwd_route()]


def set_deterministic(on):
    """Process-wide: route the backward formulations whose bits depend on arrival order -- the window scatter's float-atomic
    flush, and the general float-atomic kernels that warps of more than four channels (affine: more than eight), nearest and
    size-changing warps end in, and the bicubic backward -- through their 64-bit fixed-point twins (include/advchain_hip.h:
    advchain_set_deterministic, advchain_grid_sample_bwd_det, advchain_affine_warp_bwd_det,
    advchain_grid_sample_bicubic2d_bwd_det), and the two VALUES that arrive through float atomics in the default mode -- the
    consistency loss (the *_fwd_ord entries) and the norm behind the 3D step count (field_sumsq) -- through one partial per
    workgroup and an ordered reduction.  The solver sets it at
    the start of every call from its `deterministic` attribute; two solvers with different settings in one process are fine as
    long as their calls do not interleave (a workspace is sized when it is allocated, for the mode of that moment)."""
    _lib.load().advchain_set_deterministic(1 if on else 0)


def is_deterministic():
    return bool(_lib.load().advchain_get_deterministic())


def set_tp_wide_loads(on):
    """Process-wide: whether the row-blended kernels (raw_tp_interp, the smoothed pair, the bias field) fetch bands of 2 and
    4 by 16-byte requests (the default) or every band by dword loads (advchain_set_tp_wide_loads; the composite entries of
    demons_compose.cpp follow it too).  The same bits either way: tests and tools compare the two forms in one process."""
    _lib.load().advchain_set_tp_wide_loads(1 if on else 0)


def tp_wide_loads():
    return bool(_lib.load().advchain_get_tp_wide_loads())


def _scatter_workspace(N, dims, device):
    n = _lib.load().advchain_scatter_workspace(N, len(dims), _lib.dims_array(dims))
    return torch.empty(n, device=device, dtype=torch.int32)


def _det_warp_workspace(N, C, dims, device):
    n = _lib.load().advchain_det_warp_workspace(N, C, len(dims), _lib.dims_array(dims))
    return torch.empty(max(1, n), device=device, dtype=torch.int32)


def _general_warp_kernel(C, interp, in_dims, out_dims):
    """True for the calls advchain_grid_sample_bwd sends to its general float-atomic kernel rather than to a C <= 4 route:
    the negation of the condition `same && interp == INTERP_LINEAR && C <= 4` of advchain_grid_sample_bwd in
    csrc/sampler.hip (keep the two in step).  Deterministic mode sends these to advchain_grid_sample_bwd_det."""
    return C > 4 or interp != 0 or tuple(in_dims) != tuple(out_dims)


def raw_grid_sample_bwd(gout, inp, grid, interp, padding, clamp_grid, need_gin, need_ggrid, halo=0):
    N, C = inp.shape[:2]
    nd = inp.dim() - 2
    if need_gin and is_deterministic() and _general_warp_kernel(C, interp, inp.shape[2:], grid.shape[2:]):
        ws = _det_warp_workspace(N, C, inp.shape[2:], inp.device)
        gin = torch.empty_like(inp)
        ggrid = torch.empty_like(grid) if need_ggrid else None
        _lib.check(_lib.load().advchain_grid_sample_bwd_det(_ptr(gout), _ptr(inp), _ptr(grid), _ptr(gin), _ptr(ggrid), _ptr(ws),
                                                            N, C, nd, _lib.dims_array(inp.shape[2:]),
                                                            _lib.dims_array(grid.shape[2:]), interp, padding, int(clamp_grid),
                                                            _stream()), "grid_sample_bwd_det")
        return gin, ggrid
    tiled = TILED_SCATTER and need_gin
    ws = _scatter_workspace(N, inp.shape[2:], inp.device) if tiled else None
    gin = (torch.empty_like(inp) if tiled else torch.zeros_like(inp)) if need_gin else None
    ggrid = torch.empty_like(grid) if need_ggrid else None
    if (tiled and WINDOW_STAGED and nd == 2 and C in WINDOW_STAGED_CHANNELS and is_deterministic()
            and not _general_warp_kernel(C, interp, inp.shape[2:], grid.shape[2:])):
        lib = _lib.load()
        n = lib.advchain_window_stage_workspace(N, C, nd, _lib.dims_array(inp.shape[2:]))
        stage = torch.empty(max(4, n), device=inp.device, dtype=torch.int32)       # (not initialised: the stage kernel fills what the merge reads)
        _lib.check(lib.advchain_grid_sample_bwd_staged(_ptr(gout), _ptr(inp), _ptr(grid), _ptr(gin), _ptr(ggrid), _ptr(ws),
                                                       N, C, nd, _lib.dims_array(inp.shape[2:]),
                                                       _lib.dims_array(grid.shape[2:]), interp, padding, int(clamp_grid),
                                                       int(halo), _stream(), _ptr(stage)), "grid_sample_bwd_staged")
        return gin, ggrid
    _lib.check(_lib.load().advchain_grid_sample_bwd(_ptr(gout), _ptr(inp), _ptr(grid), _ptr(gin), _ptr(ggrid), _ptr(ws),
                                                    N, C, nd, _lib.dims_array(inp.shape[2:]),
                                                    _lib.dims_array(grid.shape[2:]), interp, padding, int(clamp_grid),
                                                    int(halo), _stream()), "grid_sample_bwd")
    return gin, ggrid


def raw_compose_self_fwd(phi, phi0=None, final_mode=0, disp_out=None, disp_hint=None):
    """phi o phi; `disp_out` (DISP_SLOTS zero-initialised floats) max-accumulates the displacement of the result.
    `disp_hint`: the caller's estimate of phi's displacement in voxels (picks the forward kernel; results do not depend on it)."""
    N = phi.shape[0]
    nd = phi.dim() - 2
    out = torch.empty_like(phi)
    _lib.check(_lib.load().advchain_compose_self_fwd(_ptr(phi), _ptr(out), _ptr(phi0), N, nd,
                                                     _lib.dims_array(phi.shape[2:]), final_mode | _hint_bits(disp_hint), _ptr(disp_out),
                                                     _stream()), "compose_self_fwd")
    return out


def raw_compose_self_bwd(gout, phi, ws=None, chain=False, halo=0):
    """chain=True: ``gout`` is the result of the previous call that used the same workspace ``ws``."""
    N = phi.shape[0]
    nd = phi.dim() - 2
    if TILED_SCATTER and ws is None:
        ws, chain = _scatter_workspace(N, phi.shape[2:], phi.device), False
    gphi = torch.empty_like(phi) if ws is not None else torch.zeros_like(phi)
    _lib.check(_lib.load().advchain_compose_self_bwd(_ptr(gout), _ptr(phi), _ptr(gphi), _ptr(ws), int(bool(chain)), int(halo), N, nd,
                                                     _lib.dims_array(phi.shape[2:]), _stream()), "compose_self_bwd")
    return gphi


def raw_max_displacement(phi, out=None):
    """max |sampling position - own voxel| of a deformation `phi` (N,d,...) in voxels -> 1-element device tensor (`out`: a
    ZEROED 1-element tensor to accumulate into)."""
    if out is None:
        out = torch.zeros(1, device=phi.device, dtype=torch.float32)
    _lib.check(_lib.load().advchain_max_displacement(_ptr(phi), _ptr(out), phi.shape[0], phi.dim() - 2,
                                                     _lib.dims_array(phi.shape[2:]), _stream()), "max_displacement")
    return out


def raw_slot_rows_max(slots, reset=False, out=None):
    """Row maxima of a (rows, slots) displacement accumulator (torch.max(dim=1) semantics incl. NaN); `reset` zeroes the
    accumulator behind the read (a persistent buffer then needs no zero-fill launch per chain)."""
    if out is None:
        out = torch.empty(slots.shape[0], device=slots.device, dtype=torch.float32)
    _lib.check(_lib.load().advchain_slot_rows_max(_ptr(slots), _ptr(out), slots.shape[0], slots.shape[1], int(bool(reset)),
                                                  _stream()), "slot_rows_max")
    return out


_PERSISTENT = {}


def _persistent_zeros(tag, shape, device):
    """A zero-initialised device buffer that lives for the process, keyed by (tag, shape, device, stream): accumulators
    whose CONSUMER kernel zeroes them again (advchain_slot_rows_max / advchain_consistency_finish with reset) -- one
    torch.zeros at first use instead of a fill launch per call.  Stream order makes the reuse safe: the consumer of call
    k runs before the producers of call k + 1 on the same stream."""
    stream = _raw_stream(_raw_device()) if (_raw_stream and _raw_device) else torch.cuda.current_stream().cuda_stream
    key = (tag, tuple(shape), str(device), stream)
    plan = _PLAN
    if plan is not None and plan.is_frozen:
        # a capture keeps its accumulators with its plan.  freeze() made the ones the recorded calls asked for (zero-filled
        # THEN, outside the capture: a torch.zeros met inside a capture is a fill node replayed with every call, for buffers
        # whose consumers leave them zeroed anyway); one that was not asked for before is made here, inside the capture
        key = key[:3]
        buf = plan.persistent.get(key)
        if buf is None:
            buf = plan.persistent[key] = torch.zeros(shape, device=device, dtype=torch.float32)
        return buf
    if plan is not None and plan.recording:
        plan.wanted_zeros.add(key[:3])
    buf = _PERSISTENT.get(key)
    if buf is None:
        if len(_PERSISTENT) > 64:
            _PERSISTENT.clear()
        buf = _PERSISTENT[key] = torch.zeros(shape, device=device, dtype=torch.float32)
    return buf


def _forget_persistent(buf):
    """Drop a persistent accumulator whose producer ran but whose consumer did not (an exception in between): it may hold
    partial sums, and the next user must start from a fresh zero-filled buffer."""
    stores = [_PERSISTENT] + ([_PLAN.persistent] if _PLAN is not None else [])
    for store in stores:
        for k in [k for k, v in store.items() if v is buf]:
            del store[k]


def raw_gauss_small_pair(x, scale, adjoint=False, weights=None):
    """Gaussian of the low-resolution planes of a paired field: forward (N,d,..) -> (2N,d,..) = [G(s x); G(-s x)], adjoint
    (2N,d,..) -> (N,d,..) = G(s x[:N]) - G(s x[N:]).  None when the planes are too large for the one-launch kernel."""
    if x[0, 0].numel() > 4096 or not x.is_contiguous() or (weights is not None and len(weights) != 9):
        return None
    nd = x.dim() - 2
    n_in = x.shape[0]
    n_out = n_in // 2 if adjoint else 2 * n_in
    out = torch.empty((n_out,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    planes = (n_out if adjoint else n_in) * x.shape[1]
    _lib.check(_lib.load().advchain_gauss_small_pair(_ptr(x), _ptr(out), planes, nd, _lib.dims_array(x.shape[2:]),
                                                     weights or _GAUSS9, float(scale), int(bool(adjoint)), _stream()),
               "gauss_small_pair")
    return out


def raw_gauss_small_pair_into(x, out, scale, weights=None):
    """raw_gauss_small_pair(x, scale) (forward form) into a buffer the caller allocated."""
    _lib.check(_lib.load().advchain_gauss_small_pair(_ptr(x), _ptr(out), x.shape[0] * x.shape[1], x.dim() - 2,
                                                     _lib.dims_array(x.shape[2:]), weights or _GAUSS9, float(scale), 0, _stream()),
               "gauss_small_pair")


@_on_tensor_device
def sign_axpy(base, x, a, gate=None, old=None):
    """base + a * sign(x) (base may be None); no autograd (parameter updates, adv_affine.py:186-195).  gate / old: see
    normalized_axpy."""
    x = _dev(x.detach(), "x")
    base = None if base is None else _dev(base.detach(), "base")
    gate, old = _gate_args(gate, old, x)
    out = torch.empty_like(x)
    _lib.check(_lib.load().advchain_sign_axpy(_ptr(base), _ptr(x), _ptr(out), float(a), x.numel(), _ptr(gate), _ptr(old),
                                              _stream()), "sign_axpy")
    return out


@_on_tensor_device
def nonzero_mask(x):
    """(x != 0) as float32 (the validity mask, adv_compose_solver.py:266-268); no autograd."""
    x = _dev(x.detach(), "x")
    out = torch.empty_like(x)
    _lib.check(_lib.load().advchain_nonzero_mask(_ptr(x), _ptr(out), x.numel(), _stream()), "nonzero_mask")
    return out


_ONES = {}


def cached_ones(shape, device):
    """A read-only tensor of ones (the input of the validity-mask warps): filled once per shape, never written."""
    key = (tuple(shape), str(device))
    plan = _PLAN
    store = plan.persistent if (plan is not None and plan.is_frozen) else _ONES
    t = store.get(("ones",) + key) if store is not _ONES else _ONES.get(key)
    if t is None:
        if store is _ONES:
            if len(_ONES) > 16:
                _ONES.clear()
            t = _ONES[key] = torch.ones(shape, device=device, dtype=torch.float32)
        else:
            # read-only: the tensor the recorded calls filled serves the capture as well (the plan keeps it alive); only a
            # shape nobody asked for before is filled under the capture (a fill node replayed with every call)
            t = _ONES.get(key)
            if t is None:
                t = torch.ones(shape, device=device, dtype=torch.float32)
            store[("ones",) + key] = t
    return t


_CLASS_W = {}


def class_weights_device(values, device):
    """The class weights `values` (a tuple of floats) as K device floats, cached per (device, values): one host-device copy at
    the first use of a weight vector, none -- and no synchronisation -- after it.  Read-only.  A capture keeps the tensor it
    read alive with its plan, so that dropping old entries here cannot free what a graph replays."""
    key = (str(device), values)
    t = _CLASS_W.get(key)
    if t is None:
        if len(_CLASS_W) > 64:
            _CLASS_W.clear()
        t = _CLASS_W[key] = torch.tensor(values, dtype=torch.float32, device=device)
    plan = _PLAN
    if plan is not None and plan.is_frozen:
        plan.persistent.setdefault(("class_w",) + key, t)
    return t


def squaring_halo(disp, d):
    """Displacement bound for the backward of one squaring from the MEASURED displacement of its input (voxels).
    Negative = exact (the gather-form adjoint then needs no overflow list): the measurement uses the kernels' own
    arithmetic, so `disp < H` guarantees every sample is within H voxels.  Larger displacements size the tile halo of
    the scatter kernels (a hint: anything beyond it goes through their overflow list)."""
    if not disp == disp:
        return 0                 # NaN field: nothing to tune
    if disp < 0.999:
        return -1
    if d == 3:       # exact bounds of 2..4 voxels: owner-computes march (scatter_march.hip); beyond: window scatter
        return _halo_3d(disp)
    if 16 - 0.001 <= disp < 32 - 0.001:
        # the whole-row scatter of a squaring still beats the window scatter here (58 against 79 us at 24 px, no zero fill,
        # deterministic)
        return -24 if disp < 24 - 0.001 else -32
    return _halo_2d(disp)


def _halo_3d(disp):
    """3D above one voxel: exact bounds of 2..4 voxels (owner-computes march scatter); beyond: a hint for the window
    scatter.  (The C ABI also takes exact bounds of 5..8 voxels -- one march launch per channel -- but on the smooth
    fields of the solver the window scatter is faster there: cfg-5 121.6 against 131.7 ms per call, cfg-4 61.4 against
    63.1; on rougher fields it is the other way round, tools/kernel_bench.py: C=4 681 against 2153 us.  Re-measured in round 4
    with the flat march scatter of round 3 in place, same box, bounds 6 / 8 handed to the march: cfg-5 99.0 against 89.2 ms
    per call -- still a loss.)"""
    for h in (2, 3, 4):
        if disp < h - 0.001:
            return -h
    return 8


def _halo_2d(disp):
    """2D: exact bounds of 2 (gather form / whole rows) and 3 .. 16 pixels (whole-row owner-computes scatter); beyond: a
    hint for the window scatter.  The whole-row kernel takes any bound; a finer ladder than powers of two (round 5) costs
    nothing -- a bound of 3 / 6 / 12 / 24 uses the fixed-point resolution of 4 / 8 / 16 / 32 (its scale is the maximum over
    the rows a workgroup visits, so the two agree to that resolution, not bit for bit) -- and visits 2 .. 16 halo rows less
    (0.7 us each at 64 x 2 x 256 x 256): cfg-2 7.39 -> 7.35 ms launch by launch, 7.50 -> 7.44 replayed."""
    for h in (2, 3, 4, 6, 8, 12, 16):
        if disp < h - 0.001:
            return -h
    return 16


def raw_gauss(x, C, pre=0, post=0, scale=1.0, aux=None, weights=None):
    """Separable 9-tap Gaussian over all spatial axes of x (planes = x.shape[0]*x.shape[1]).  `x` may be a pair of
    tensors (the two halves of a batch, e.g. the gradients of a paired field): the fused x+y launch reads both in place,
    any other route concatenates them first.  `weights`: gauss9(sigma), default sigma = 1."""
    w9 = weights or _GAUSS9
    x_hi = None
    if isinstance(x, (tuple, list)):
        x, x_hi = x
        shape = (x.shape[0] + x_hi.shape[0],) + tuple(x.shape[1:])
    else:
        shape = tuple(x.shape)
    nd = x.dim() - 2
    planes = shape[0] * shape[1]
    dims = _lib.dims_array(x.shape[2:])
    axes = [2, 1, 0][:nd]  # innermost first (padded 3-axis numbering)
    lib = _lib.load()
    if len(w9) != 9:      # another window: the plain per-axis kernel (adv_morph.py:393-398 with sigma outside [0.875, 1.125))
        if post != 0 or pre not in (0, 1):
            raise NotImplementedError("the fused prologue / epilogue of the Gaussian exists for the 9-tap window only")
        cur = torch.cat([x, x_hi], 0) if x_hi is not None else x
        cur = cur if cur.is_contiguous() else cur.contiguous()
        for i, ax in enumerate(axes):
            out = torch.empty_like(cur)
            _lib.check(lib.advchain_gauss_axis_generic(_ptr(cur), _ptr(out), planes, nd, dims, ax, w9, len(w9),
                                                       float(scale) if (pre == 1 and i == 0) else 1.0, _stream()),
                       "gauss_axis_generic")
            cur = out
        return cur
    if x_hi is not None and (x[0, 0].numel() <= 4096 or not (x.is_contiguous() and x_hi.is_contiguous())):
        x, x_hi = torch.cat([x, x_hi], 0), None
    if post == 0 and pre in (0, 1) and x[0, 0].numel() <= 4096:     # low-resolution grids: all axes in one launch
        out = torch.empty_like(x)
        _lib.check(lib.advchain_gauss_small(_ptr(x), _ptr(out), planes, nd, dims, w9, pre, float(scale), _stream()),
                   "gauss_small")
        return out
    cur = x
    # x and y in one launch where the shape allows (advchain_gauss_xy); post belongs to the last axis
    out = torch.empty(shape, device=x.device, dtype=torch.float32)
    gauss_xy = lib.advchain_gauss_xy if GAUSS_XY_LANES else lib.advchain_gauss_xy_staged
    rc = gauss_xy(_ptr(x),_ptr(out), _ptr(aux) if (post == 2 and nd == 2) else None, planes, C, nd, dims, w9,
                               pre, post if nd == 2 else 0, float(scale) if pre == 1 else 1.0, _stream(), _ptr(x_hi),
                               x.shape[0] * x.shape[1])
    if rc == 0:
        if nd == 2:
            return out
        out2 = torch.empty_like(out)
        _lib.check(lib.advchain_gauss_axis(_ptr(out), _ptr(out2), _ptr(aux) if post == 2 else None, planes, C, nd, dims, 0,
                                           w9, 0, post, 1.0, _stream()), "gauss_axis")
        return out2
    if rc != -2:
        _lib.check(rc, "gauss_xy")
    if x_hi is not None:
        x = cur = torch.cat([x, x_hi], 0)
    for i, ax in enumerate(axes):
        out = torch.empty_like(x)
        p = pre if i == 0 else 0
        q = post if i == len(axes) - 1 else 0
        _lib.check(lib.advchain_gauss_axis(_ptr(cur), _ptr(out), _ptr(aux) if q == 2 else None, planes, C, nd, dims, ax,
                                           w9, p, q, float(scale) if p == 1 else 1.0, _stream()), "gauss_axis")
        cur = out
    return cur


def raw_tp_interp(coef, tables, C, add_identity=False, scale=1.0, want_out=True, sumsq=None, disp_out=None, out=None):
    planes = coef.shape[0] * coef.shape[1]
    if want_out and out is None:
        out = torch.empty((coef.shape[0], coef.shape[1]) + tuple(tables.full_dims), device=coef.device,
                          dtype=torch.float32)
    _lib.check(_lib.load().advchain_tp_interp_fwd(_ptr(coef), _ptr(out), _ptr(tables.itab), _ptr(tables.ftab),
                                                  _lib.dims_array(tables.S), _lib.dims_array(tables.g),
                                                  _lib.dims_array(tables.B), planes, C, tables.ndim,
                                                  int(add_identity), float(scale), _ptr(sumsq), _ptr(disp_out),
                                                  _stream()),
               "tp_interp_fwd")
    return out


def field_sumsq(coef, tables, C):
    """Sum of the squares of the field that `raw_tp_interp(coef, tables, C)` interpolates, as a 1-element device tensor; the
    field is not materialised.  It is what the 3D step-count rule (adv_morph.py:159-162) takes the root of: the solver, a
    sharded `reduce_sumsq` and the frozen plan's check all read it here.  Default mode: workgroup partials arrive in 64 slots
    through float atomics (last bits vary run to run).  Deterministic mode: one partial per workgroup and one ordered
    reduction (advchain_tp_interp_sumsq_ordered) -- equal bits for equal inputs, so the count never flips at a threshold."""
    coef = _dev(coef, "coefficients")
    if is_deterministic():
        lib = _lib.load()
        planes = coef.shape[0] * coef.shape[1]
        S = _lib.dims_array(tables.S)
        partials = torch.empty(max(1, lib.advchain_tp_interp_sumsq_partials(S, planes)), device=coef.device, dtype=torch.float32)
        out = torch.empty(1, device=coef.device, dtype=torch.float32)
        _lib.check(lib.advchain_tp_interp_sumsq_ordered(_ptr(coef), _ptr(tables.itab), _ptr(tables.ftab), S,
                                                        _lib.dims_array(tables.g), _lib.dims_array(tables.B), planes, C,
                                                        _ptr(partials), _ptr(out), _stream()), "tp_interp_sumsq_ordered")
        return out
    slots = torch.zeros(64, device=coef.device, dtype=torch.float32)
    raw_tp_interp(coef, tables, C, want_out=False, sumsq=slots)
    return slots.sum().reshape(1)


def raw_tp_adjoint(gfull, tables, gfull2=None, scale=1.0):
    """W^T applied along every axis: (N,C,S...) -> (N,C,g...).  First pass may fuse (a - b) * scale."""
    return _tp_adjoint_passes(gfull, tables, gfull2, scale, (2, 1, 0))


def raw_tp_adjoint_from_t1(t1, tables):
    """The remaining axis passes of raw_tp_adjoint from t1 (N,C,S0,S1,g2 / N,C,S1,g2), the result of its innermost pass."""
    return _tp_adjoint_passes(t1, tables, None, 1.0, (1, 0))


def _tp_adjoint_passes(gfull, tables, gfull2, scale, axes):
    lib = _lib.load()
    N, C = gfull.shape[:2]
    S, g, B = list(tables.S), list(tables.g), list(tables.B)
    Sa, ga, Ba = _lib.dims_array(S), _lib.dims_array(g), _lib.dims_array(B)
    cur, cur2 = gfull, gfull2
    shape = list(S)
    for ax in (2, 1, 0):
        if ax not in axes:
            shape[ax] = g[ax]             # (already reduced)
    first = 2 in axes
    for ax in axes:
        if S[ax] == 1 and g[ax] == 1:
            continue
        outer = N * C
        for a in range(ax):
            outer *= shape[a]
        inner = 1
        for a in range(ax + 1, 3):
            inner *= shape[a]
        shape[ax] = g[ax]
        out = torch.empty((N, C) + tuple(shape[3 - tables.ndim:]), device=gfull.device, dtype=torch.float32)
        rc = -2
        if ax == 2 and inner == 1 and getattr(tables, "dense_inner", None) is not None:
            # the full-resolution pass with the bands densified once per table (same sums, same order)
            wd, lo, WB = tables.dense_inner
            rc = lib.advchain_band_reduce_rows_dense(_ptr(cur), _ptr(cur2), _ptr(out), _ptr(wd), _ptr(lo), outer, S[2], g[2], WB,
                                                     float(scale) if first else 1.0, _stream())
            if rc != -2:
                _lib.check(rc, "band_reduce_rows_dense")
        if rc == -2:
            _lib.check(lib.advchain_band_reduce_axis(_ptr(cur), _ptr(cur2), _ptr(out), _ptr(tables.itab), _ptr(tables.ftab),
                                                     Sa, ga, Ba, ax, outer, inner, float(scale) if first else 1.0,
                                                     _stream()), "band_reduce_axis")
        cur, cur2, first = out, None, False
    if first and 2 in axes:  # degenerate: nothing to reduce
        cur = (gfull - gfull2 if gfull2 is not None else gfull) * scale
    return cur


def raw_axpy(x, y, a):
    out = torch.empty_like(y)
    _lib.check(_lib.load().advchain_axpy(_ptr(x), _ptr(y), _ptr(out), float(a), y.numel(), _stream()), "axpy")
    return out


def _gate_args(gate, old, like):
    """(gate pointer, old pointer) of the NaN-gated parameter updates: `gate` a 0-dim / 1-element device tensor (the loss of
    the step), `old` what the output falls back to when the gate is not finite."""
    if gate is None:
        return None, None
    gate = _dev(gate.detach().reshape(1), "gate")
    old = _dev(old.detach(), "old")
    if old.shape != like.shape:
        raise RuntimeError("gated update: `old` must have the shape of the result")
    return gate, old


@_on_tensor_device
def normalized_axpy(base, x, step=1.0, gate=None, old=None):
    """base + step * x / (||x||_2 per sample + 1e-20); base may be None.  No autograd (parameter updates).  With `gate` (a
    device scalar) the result is `old` whenever the gate is NaN / inf: the solver's NaN guard without a host read-back."""
    x = _dev(x.detach(), "x")
    base = None if base is None else _dev(base.detach(), "base")
    gate, old = _gate_args(gate, old, x)
    N = x.shape[0]
    M = x.numel() // max(N, 1)
    lib = _lib.load()
    ws = torch.empty(max(1, lib.advchain_norm_workspace(N, M)), device=x.device, dtype=torch.float32)
    out = torch.empty_like(x)
    _lib.check(lib.advchain_norm_axpy_gated(_ptr(base), _ptr(x), _ptr(out), _ptr(ws), float(step), N, M, _ptr(gate), _ptr(old),
                                            _stream()), "norm_axpy")
    return out


# ------------------------------------------------------------------------------------------------
# autograd Functions
# ------------------------------------------------------------------------------------------------
FUSED_UPDATE = True   # the parameter updates of an ascent step as ONE launch (advchain_update_multi); False: one per transform


@_on_tensor_device
def update_multi(items, gate=None):
    """The parameter updates of one ascent step in one launch.  items: [(base or None, x, step, kind, old)] with kind 0 =
    base + step * x / (||x||_2 per sample + 1e-20), kind 1 = base + step * sign(x); `gate` (a device scalar): a non-finite gate
    keeps `old`.  Returns the new tensors (no autograd: parameter updates)."""
    lib = _lib.load()
    descs = (_lib.UpdateDesc * len(items))()
    outs, keep = [], []
    g = None if gate is None else _dev(gate.detach().reshape(1), "gate")
    for d, (base, x, step, kind, old) in zip(descs, items):
        x = _dev(x.detach(), "x")
        base = None if base is None else _dev(base.detach(), "base")
        old = None if old is None else _dev(old.detach(), "old")
        if g is not None and (old is None or old.shape != x.shape):
            raise RuntimeError("gated update: `old` must have the shape of the result")
        if base is not None and base.shape != x.shape:
            raise RuntimeError("update_multi: base and x differ in shape")
        out = torch.empty_like(x)
        N = x.shape[0]
        d.base, d.x, d.out, d.old = _ptr(base), _ptr(x), _ptr(out), _ptr(old)
        d.N, d.M, d.kind, d.step = N, x.numel() // max(N, 1), int(kind), float(step)
        outs.append(out)
        keep.extend((x, base, old))
    _lib.check(lib.advchain_update_multi(ctypes.byref(descs), len(items), _ptr(g), _stream()), "update_multi")
    return outs


class _Readback:
    """A few device floats copied to pinned host memory right where they are produced, with an event recorded behind
    the copy.  `values()` waits on THAT event only: by the time the backward asks, the copy finished long ago, so the
    read does not drain the kernels queued since (a `.item()` would enqueue its copy behind all of them)."""

    def __init__(self, dev_tensor):
        self.host = torch.empty(dev_tensor.shape, dtype=dev_tensor.dtype, pin_memory=True)
        self.host.copy_(dev_tensor, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(_stream_obj())
        self._vals = None

    def values(self):
        if self._vals is None:
            self.event.synchronize()
            self._vals = self.host.tolist()
        return self._vals



# ------------------------------------------------------------------------------------------------
# launch plans: the kernel selection of one solver call, recorded and then frozen (hipGraph replay)
# ------------------------------------------------------------------------------------------------
# The backward kernels are chosen from displacement bounds that the forward MEASURES and the host reads back (squaring_halo,
# warp_halo); the 3D chain reads a whole-batch norm for the reference's step rule.  A captured hipGraph cannot read anything
# back: a LaunchPlan records what those sites read during ordinary (eager) calls, freezes the values with a margin, and the
# capture takes every selection from the frozen plan.  Each site then enqueues advchain_bounds_check on what the replay
# measures against the interval its frozen selection is exact for; a raised flag tells the caller (the solver) to run
# that call again the ordinary way.  Results of a replay whose flag stays down are those of the ordinary path with the
# same selection (every formulation is tested against every other; the selection never changes values beyond that).
_PLAN = None


class PlanMismatch(RuntimeError):
    """The launch sequence met during a capture is not the recorded one."""


class _FrozenBounds(object):
    """Stands in for a _Readback when the plan is frozen: the bounds are host numbers known before the launch."""

    class _Done(object):
        @staticmethod
        def query():
            return True

        @staticmethod
        def synchronize():
            return None

    event = _Done

    def __init__(self, vals):
        self._vals = [float(v) for v in vals]

    def values(self):
        return self._vals


def _halo_threshold(h):
    """The displacement below which the bound `h` (squaring_halo / warp_halo) is exact; inf for a hint."""
    if h == -1:
        return 0.999
    if h < 0:
        return -h - 0.001
    return float("inf")


def _warp_halo_of(est, d):
    if not est == est:
        return 0
    if d == 3:
        return -1 if est < 0.999 else _halo_3d(est)
    return _halo_2d(est)


class LaunchPlan(object):
    """recording: sites append what they read (note); end_record() turns the read-backs into numbers and merges them with
    the calls recorded before (element-wise max).  freeze(): numbers x margin -> per-site selections + device intervals.
    frozen: take() hands the sites out in call order, check() enqueues the premise check."""

    def __init__(self, margin=1.3):
        # margin: the recorded maxima x margin pick the frozen selection.  Displacements vary with the random initial
        # parameters (cfg-2, second ascent step: 0.886 px over two recorded calls, 1.107 px in the third), and the levels of a
        # chain double, so every level sits at the same relative distance from ITS power-of-two threshold: a margin that is
        # too small is violated on all of them at once.  1.1 was (one call in five re-run the ordinary way); what a wide
        # margin costs is one formulation up on the levels within its reach of a threshold (+0.1 ms per cfg-2 call at 1.25)
        self.margin = float(margin)
        self.recording = True
        self.pending = []        # this call's sites while recording: (kind, payload)
        self.recorded = None     # merged: list of (kind, dict of numbers)
        self.calls = 0
        self.unstable = False    # two recorded calls did not visit the same sites
        self.frozen = None
        self.cursor = 0
        self.flag = None
        self.persistent = {}
        self.wanted_zeros = set()  # (tag, shape, device) of the persistent accumulators the recorded calls asked for
        self.violated = []       # diagnostics: which frozen bound a violated replay exceeded (filled by the recorded re-run)

    @property
    def is_frozen(self):
        return self.frozen is not None and not self.recording

    # -- recording
    def begin_record(self):
        """An ordinary call is about to be recorded.  A frozen selection stays in place (a captured graph keeps replaying it
        after this call); whatever an interrupted call left pending is dropped."""
        self.recording = True
        self.pending = []

    def thaw(self):
        """Drop the frozen selection (a new capture will freeze the merged record again)."""
        self.frozen = None
        self.persistent = {}

    def note(self, kind, **payload):
        self.pending.append((kind, payload))

    def end_record(self):
        sites = []
        for kind, pl in self.pending:
            if kind == "chain":
                sites.append((kind, {"n": pl["n"], "d": pl["d"], "vals": [float(v) for v in pl["rb"].values()]}))
            elif kind == "nsteps":
                sites.append((kind, {"n": pl["n"], "n_base": pl["n_base"]}))
            elif kind == "warp":
                sites.append((kind, {"d": pl["d"], "vals": [float(pl["rb"].values()[pl["idx"]])]}))
        self.pending = []
        # a recorded call that follows a violated replay measured what that replay measured: say which bound gave way
        last = self.frozen
        if last is not None and len(last) == len(sites):
            for i, (fz, (kind, rec)) in enumerate(zip(last, sites)):
                if "vals" in rec and fz["kind"] == kind:
                    his = fz["hi"].tolist()
                    for j, v in enumerate(rec["vals"]):
                        if j < len(his) and not (v < his[j]):
                            self.violated.append({"site": i, "kind": kind, "row": j, "measured": round(v, 4), "bound": round(his[j], 4),
                                                  "frozen_from": round(fz["bounds"].values()[j], 4)})
            del self.violated[:-64]
        if self.recorded is None:
            self.recorded = sites
        elif [(k, v.get("n"), v.get("d")) for k, v in sites] != [(k, v.get("n"), v.get("d")) for k, v in self.recorded]:
            self.unstable = True          # (another step count, another number of sites): the latest call wins
            self.recorded = sites
        else:
            for (_, old), (_, new) in zip(self.recorded, sites):
                if "vals" in old:
                    old["vals"] = [b if (b != b or b > a) else a for a, b in zip(old["vals"], new["vals"])]
        self.calls += 1
        self.recording = False

    # -- freezing
    def freeze(self, device):
        import numpy as np
        los, his, sites = [], [], []
        for kind, rec in self.recorded:
            if kind == "chain":
                n, d = rec["n"], rec["d"]
                vals = [v * self.margin if v == v else v for v in rec["vals"]]
                thr = [_halo_threshold(squaring_halo(vals[m], d)) for m in range(n)]
                thr.append(_halo_threshold(_warp_halo_of(vals[n], d)))
                thr += [float("inf")] * (len(vals) - n - 1)
                site = {"kind": kind, "n": n, "d": d, "bounds": _FrozenBounds(vals), "off": len(los), "len": len(thr)}
                los += [-float("inf")] * len(thr)
                his += thr
            elif kind == "nsteps":
                n, nb = rec["n"], rec["n_base"]
                # the rule of adv_morph.py:159-162 on sqrt(sum u^2): n is the smallest count >= n_base with norm / 2^n <= 0.5
                # (norm in (2^(n-2), 2^(n-1)]; as the half-open interval [lo, hi) of fp32 numbers the check kernel takes)
                up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))
                hi = up(2.0 ** (n - 1))
                lo = up(2.0 ** (n - 2)) if n > nb else -float("inf")
                site = {"kind": kind, "n": n, "n_base": nb, "off": len(los), "len": 1}
                los.append(lo)
                his.append(hi)
            else:
                d = rec["d"]
                est = rec["vals"][0] * self.margin
                site = {"kind": kind, "d": d, "bounds": _FrozenBounds([est]), "off": len(los), "len": 1}
                los.append(-float("inf"))
                his.append(_halo_threshold(_warp_halo_of(est, d)))
            sites.append(site)
        f32 = torch.float32
        lo_t = torch.tensor(los or [0.0], dtype=f32).clamp(-3.0e38, 3.0e38).to(device)
        hi_t = torch.tensor(his or [0.0], dtype=f32).to(device)      # (inf stays inf: x < inf holds for every finite x)
        for sdict in sites:
            sdict["lo"] = lo_t[sdict["off"]:sdict["off"] + sdict["len"]]
            sdict["hi"] = hi_t[sdict["off"]:sdict["off"] + sdict["len"]]
        self.flag = torch.zeros(1, device=device, dtype=torch.int32)
        # what a replay measures, site after site, in ONE buffer (the producers write straight into their site's slice): one
        # check launch at the end of the replay instead of one per site (finish())
        self.measured = torch.zeros(max(1, len(los)), device=device, dtype=f32)
        self._lo_t, self._hi_t, self._deferred = lo_t, hi_t, 0
        self.frozen = sites
        self.recording = False
        self.cursor = 0
        self.persistent = {k: torch.zeros(k[1], device=device, dtype=f32) for k in sorted(self.wanted_zeros, key=repr) if k[2] == str(device)}

    # -- frozen
    def rewind(self):
        """Before the frozen sites are walked again (a capture; a launch-by-launch run of the frozen selection): the first
        site again, the measurement slots zeroed (the warp sites accumulate a maximum into theirs)."""
        self.cursor = 0
        self._deferred = 0
        self.measured.zero_()

    def slot(self, site):
        """Where the producer of this site's measurement writes it (a view of `measured`)."""
        return self.measured[site["off"]:site["off"] + site["len"]]

    def finish(self):
        """The premise check of everything measured into the slots since rewind(): one launch."""
        if self._deferred:
            n = self.measured.numel()
            _lib.check(_lib.load().advchain_bounds_check(_ptr(self.measured), _ptr(self._lo_t), _ptr(self._hi_t), n,
                                                         ctypes.c_void_p(self.flag.data_ptr()), _stream()), "bounds_check")
            self._deferred = 0

    def take(self, kind, **expect):
        if self.cursor >= len(self.frozen):
            raise PlanMismatch("launch plan: more %s sites than recorded" % kind)
        site = self.frozen[self.cursor]
        self.cursor += 1
        if site["kind"] != kind or any(site.get(k) != v for k, v in expect.items()):
            raise PlanMismatch("launch plan: met a %s site %r where a %s site was recorded" % (kind, expect, site["kind"]))
        return site

    def check(self, values, site):
        if values.numel() != site["len"]:
            raise PlanMismatch("launch plan: %d measured values for a site of %d" % (values.numel(), site["len"]))
        if values.data_ptr() == self.measured.data_ptr() + 4 * site["off"]:      # written into its slot: checked by finish()
            self._deferred += 1
            return
        _lib.check(_lib.load().advchain_bounds_check(_ptr(values), _ptr(site["lo"]), _ptr(site["hi"]), site["len"],
                                                     ctypes.c_void_p(self.flag.data_ptr()), _stream()), "bounds_check")


def grid_displacement(grid):
    """Max displacement (voxels) of a sampling grid, measured once per grid tensor (the entry -- a 1-float device tensor
    and, after the first read-back, its host value -- rides on the tensor object: the same deformation warps the image
    and then the prediction)."""
    hit = getattr(grid, "_advchain_disp", None)
    if hit is None or hit[2] != grid._version:
        plan = _PLAN
        key = (str(grid.device),) + tuple(grid.shape[2:])
        if plan is not None and plan.is_frozen:        # frozen plan: the recorded bound, and the premise check on the measured one
            site = plan.take("warp", d=grid.dim() - 2)
            plan.check(raw_max_displacement(grid.detach(), out=plan.slot(site)), site)
            hit = [site["bounds"], None, grid._version, 0, None]
        else:
            hit = [_Readback(raw_max_displacement(grid.detach())), None, grid._version, 0, key]
            if plan is not None:
                plan.note("warp", rb=hit[0], idx=0, d=grid.dim() - 2)
        grid._advchain_disp = hit
    return hit


def forward_hint(grid):
    """Displacement estimate (voxels) for the FORWARD warp by `grid`, without waiting for anything: the bound riding on
    the grid if its read-back has already arrived, else the last bound read for a grid of this shape (the deformation of
    the previous ascent step), else None.  Picks the forward kernel only."""
    hit = getattr(grid, "_advchain_disp", None)
    if hit is not None and hit[2] == grid._version:
        if hit[1] is None and hit[0].event.query():
            hit[1] = float(hit[0].values()[hit[3]])
            if len(hit) > 4 and hit[4] is not None:
                _WARP_HINTS[hit[4]] = hit[1]
        if hit[1] is not None:
            return hit[1]
    return _WARP_HINTS.get((str(grid.device),) + tuple(grid.shape[2:]))


def warp_halo(entry, d):
    """Displacement bound for the backward of a warp from the measured value (one 4-byte read-back per grid);
    negative = exact (see squaring_halo)."""
    if entry[1] is None:
        entry[1] = float(entry[0].values()[entry[3]])
    est = entry[1]
    if len(entry) > 4 and entry[4] is not None:
        _WARP_HINTS[entry[4]] = est
    return _warp_halo_of(est, d)


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, grid, interp, padding, clamp_grid, disp, hint=None, ride=None, ride_nonzero=False):
        inp, grid = _dev(inp, "input"), _dev(grid, "grid")
        ctx.save_for_backward(inp, grid)
        ctx.cfg = (interp, padding, clamp_grid)
        ctx.disp = disp
        if ride is None:
            return raw_grid_sample_fwd(inp, grid, interp, padding, clamp_grid, hint)
        # a one-channel rider (the solver's validity mask) through the same grid: second output, no gradient
        out, rout = raw_grid_sample_fwd_ride(inp, grid, _dev(ride, "rider"), interp, padding, clamp_grid, ride_nonzero, hint)
        ctx.mark_non_differentiable(rout)
        ctx.set_materialize_grads(False)     # (or the engine fills a zero gradient for the rider on every backward)
        return out, rout

    @staticmethod
    def backward(ctx, gout, _grider=None):
        inp, grid = ctx.saved_tensors
        interp, padding, clamp_grid = ctx.cfg
        need_in, need_grid = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gout is None or not (need_in or need_grid):
            return (None,) * 9
        halo = warp_halo(ctx.disp, inp.dim() - 2) if (ctx.disp is not None and need_in) else 0
        gin, ggrid = raw_grid_sample_bwd(_dev(gout, "grad"), inp, grid, interp, padding, clamp_grid, need_in, need_grid,
                                         halo)
        return (gin, ggrid) + (None,) * 7


@_on_tensor_device
def grid_sample(inp, grid, interp="bilinear", padding_mode="zeros", clamp_grid=False, ride=None, ride_nonzero=False):
    """F.grid_sample(inp, grid^T, mode, padding_mode, align_corners=True) with a PLANAR grid (N,d,...).
    ride: a one-channel tensor (N,1,...) warped through the same grid in the same call (linear / nearest only) -> returns
    (out, ride_out); ride_out carries no gradient; ride_nonzero: ride_out = (warp(ride) != 0) as 0 / 1."""
    code = interp_code(interp)
    nd = inp.dim() - 2
    if nd not in (2, 3) or grid.dim() != inp.dim() or grid.shape[1] != nd:
        raise RuntimeError("grid_sample(): expected a planar grid of shape (N, %d, ...) for a %d-D input, got %s"
                           % (nd, inp.dim(), tuple(grid.shape)))
    if grid.shape[0] != inp.shape[0]:
        raise RuntimeError("grid_sample(): expected grid and input to have same batch size, but got input with sizes "
                           "%s and grid with sizes %s" % (list(inp.shape), list(grid.shape)))
    _same_device(inp, grid)
    if code == 2:
        if nd != 2:      # F.grid_sample's own message for 5-D input
            raise RuntimeError("grid_sampler(): bicubic interpolation only supports 4D input")
        if ride is not None:
            raise NotImplementedError("grid_sample(): no rider with bicubic interpolation")
        return _GridSampleBicubic.apply(inp, torch.clamp(grid, -1, 1) if clamp_grid else grid, pad_code(padding_mode))
    disp = None
    if (ADAPTIVE_HALO and code == 0 and torch.is_grad_enabled() and inp.requires_grad and grid.is_cuda
            and inp.shape[2:] == grid.shape[2:] and grid.dtype == torch.float32 and grid.is_contiguous()):
        disp = grid_displacement(grid)       # the backward sizes its halo / picks the gather form from it
    hint = forward_hint(grid) if (code == 0 and nd == 3 and grid.is_cuda) else None
    if ride is not None:
        if tuple(ride.shape) != (inp.shape[0], 1) + tuple(inp.shape[2:]):
            raise RuntimeError("grid_sample(): the rider must be (N, 1, ...) of the input's size, got %s" % (tuple(ride.shape),))
        _same_device(inp, ride)
        return _GridSample.apply(inp, grid, code, pad_code(padding_mode), bool(clamp_grid), disp, hint, ride.detach(),
                                 bool(ride_nonzero))
    return _GridSample.apply(inp, grid, code, pad_code(padding_mode), bool(clamp_grid), disp, hint)


class _GridSampleBicubic(torch.autograd.Function):
    """F.grid_sample(inp, grid^T, mode='bicubic', padding_mode, align_corners=True) with a PLANAR grid (N,2,OH,OW); 2D only
    (adv_morph.py:255-258,546-557 with forward_interp / backward_interp = 'bicubic')."""

    @staticmethod
    def forward(ctx, inp, grid, padding):
        inp, grid = _dev(inp, "input"), _dev(grid, "grid")
        N, C = inp.shape[:2]
        out = torch.empty((N, C) + tuple(grid.shape[2:]), device=inp.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_grid_sample_bicubic2d_fwd(_ptr(inp), _ptr(grid), _ptr(out), N, C,
                                                                  _lib.dims_array(inp.shape[2:]), _lib.dims_array(grid.shape[2:]),
                                                                  padding, _stream()), "grid_sample_bicubic2d_fwd")
        ctx.save_for_backward(inp, grid)
        ctx.padding = padding
        return out

    @staticmethod
    def backward(ctx, gout):
        inp, grid = ctx.saved_tensors
        need_in, need_grid = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_in or need_grid):
            return None, None, None
        gin = torch.empty_like(inp) if need_in else None
        ggrid = torch.empty_like(grid) if need_grid else None
        N, C = inp.shape[:2]
        if need_in and is_deterministic():      # grad_in through the int64 image instead of float atomics
            lib = _lib.load()
            ws = torch.empty(max(1, lib.advchain_bicubic2d_det_workspace(N, C, _lib.dims_array(inp.shape[2:]))),
                             device=inp.device, dtype=torch.int32)
            _lib.check(lib.advchain_grid_sample_bicubic2d_bwd_det(_ptr(_dev(gout, "grad")), _ptr(inp), _ptr(grid), _ptr(gin),
                                                                  _ptr(ggrid), _ptr(ws), N, C, _lib.dims_array(inp.shape[2:]),
                                                                  _lib.dims_array(grid.shape[2:]), ctx.padding, _stream()),
                       "grid_sample_bicubic2d_bwd_det")
            return gin, ggrid, None
        _lib.check(_lib.load().advchain_grid_sample_bicubic2d_bwd(_ptr(_dev(gout, "grad")), _ptr(inp), _ptr(grid), _ptr(gin), _ptr(ggrid),
                                                                  N, C, _lib.dims_array(inp.shape[2:]), _lib.dims_array(grid.shape[2:]),
                                                                  ctx.padding, _stream()), "grid_sample_bicubic2d_bwd")
        return gin, ggrid, None


class _AffineGrid2D(torch.autograd.Function):
    """F.affine_grid(theta, (N, C, H, W), align_corners=True) as a planar grid (N,2,H,W) (bicubic affine warps only: the
    linear / nearest ones never materialise the grid)."""

    @staticmethod
    def forward(ctx, theta, H, W):
        theta = _dev(theta, "theta")
        N = theta.shape[0]
        grid = torch.empty((N, 2, H, W), device=theta.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_affine_grid2d_fwd(_ptr(theta), _ptr(grid), N, _lib.dims_array((H, W)), _stream()),
                   "affine_grid2d_fwd")
        ctx.dims = (H, W)
        return grid

    @staticmethod
    def backward(ctx, ggrid):
        H, W = ctx.dims
        ggrid = _dev(ggrid, "grad")
        N = ggrid.shape[0]
        lib = _lib.load()
        dims = _lib.dims_array((H, W))
        ws = torch.empty(max(1, lib.advchain_affine_grid2d_bwd_workspace(N, dims)), device=ggrid.device, dtype=torch.float32)
        gth = torch.empty((N, 2, 3), device=ggrid.device, dtype=torch.float32)
        _lib.check(lib.advchain_affine_grid2d_bwd(_ptr(ggrid), _ptr(gth), _ptr(ws), N, dims, _stream()), "affine_grid2d_bwd")
        return gth, None, None


class _AffineWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, theta, interp, padding, ride=None, ride_nonzero=False):
        inp, theta = _dev(inp, "input"), _dev(theta, "theta")
        N, C = inp.shape[:2]
        nd = inp.dim() - 2
        out = torch.empty_like(inp)
        ctx.save_for_backward(inp, theta)
        ctx.cfg = (interp, padding)
        if ride is not None:     # a one-channel rider (the solver's validity mask) under the same theta: no gradient
            ride = _dev(ride, "rider")
            rout = torch.empty_like(ride)
            _lib.check(_lib.load().advchain_affine_warp_fwd_ride(_ptr(inp), _ptr(theta), _ptr(out), _ptr(ride), _ptr(rout), N, C,
                                                                 nd, _lib.dims_array(inp.shape[2:]), interp, padding,
                                                                 int(bool(ride_nonzero)), _stream()), "affine_warp_fwd_ride")
            ctx.mark_non_differentiable(rout)
            ctx.set_materialize_grads(False)     # (or the engine fills a zero gradient for the rider on every backward)
            return out, rout
        _lib.check(_lib.load().advchain_affine_warp_fwd(_ptr(inp), _ptr(theta), _ptr(out), N, C, nd,
                                                        _lib.dims_array(inp.shape[2:]), interp, padding, _stream()),
                   "affine_warp_fwd")
        return out

    @staticmethod
    def backward(ctx, gout, _grider=None):
        inp, theta = ctx.saved_tensors
        interp, padding = ctx.cfg
        need_in, need_th = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gout is None or not (need_in or need_th):
            return (None,) * 6
        lib = _lib.load()
        N, C = inp.shape[:2]
        nd = inp.dim() - 2
        dims = _lib.dims_array(inp.shape[2:])
        gin = torch.empty_like(inp) if need_in else None
        gth = torch.empty_like(theta) if need_th else None
        ws = torch.empty(max(1, lib.advchain_affine_warp_bwd_workspace(N, nd, dims)), device=inp.device,
                         dtype=torch.float32)
        # Deterministic mode: the calls advchain_affine_warp_bwd answers by zeroing grad_in and scattering every sample with
        # float atomics take the fixed-point twin.  C <= 8 with linear / zeros keeps its atomic-free gather (C <= 4: the box
        # tiles); the samples that gather flags as degenerate keep today's scatter -- the remainder the mode does not cover.
        if need_in and is_deterministic() and (C > 8 or (C > 4 and (interp != 0 or padding != 0))):
            dws = _det_warp_workspace(N, C, inp.shape[2:], inp.device)
            _lib.check(lib.advchain_affine_warp_bwd_det(_ptr(_dev(gout, "grad")), _ptr(inp), _ptr(theta), _ptr(gin), _ptr(gth),
                                                        _ptr(ws), _ptr(dws), N, C, nd, dims, interp, padding, _stream()),
                       "affine_warp_bwd_det")
            return gin, gth, None, None, None, None
        _lib.check(lib.advchain_affine_warp_bwd(_ptr(_dev(gout, "grad")), _ptr(inp), _ptr(theta), _ptr(gin), _ptr(gth),
                                                _ptr(ws), N, C, nd, dims, interp, padding, _stream()), "affine_warp_bwd")
        return gin, gth, None, None, None, None


@_on_tensor_device
def affine_warp(inp, theta, interp="bilinear", padding_mode="zeros", ride=None, ride_nonzero=False):
    """F.grid_sample(inp, F.affine_grid(theta, inp.size(), align_corners=True), ..., align_corners=True).
    ride / ride_nonzero: as for grid_sample -> returns (out, ride_out)."""
    nd = inp.dim() - 2
    if tuple(theta.shape) != (inp.shape[0], nd, nd + 1):
        raise RuntimeError("Expected a batch of %dD affine matrices of shape Nx%dx%d for size %s. Got %s."
                           % (nd, nd, nd + 1, list(inp.shape), list(theta.shape)))
    _same_device(inp, theta)
    code = interp_code(interp)
    if code == 2:
        if nd != 2:
            raise RuntimeError("grid_sampler(): bicubic interpolation only supports 4D input")
        if ride is not None:
            raise NotImplementedError("affine_warp(): no rider with bicubic interpolation")
        grid = _AffineGrid2D.apply(theta, int(inp.shape[2]), int(inp.shape[3]))
        return _GridSampleBicubic.apply(inp, grid, pad_code(padding_mode))
    if ride is not None:
        if tuple(ride.shape) != (inp.shape[0], 1) + tuple(inp.shape[2:]):
            raise RuntimeError("affine_warp(): the rider must be (N, 1, ...) of the input's size, got %s" % (tuple(ride.shape),))
        _same_device(inp, ride)
        return _AffineWarp.apply(inp, theta, code, pad_code(padding_mode), ride.detach(), bool(ride_nonzero))
    return _AffineWarp.apply(inp, theta, code, pad_code(padding_mode))


class _AffineTheta(torch.autograd.Function):
    @staticmethod
    def forward(ctx, param, cfg, param_scale, nd):
        param = _dev(param, "param")
        N = param.shape[0]
        theta = torch.empty((N, nd, nd + 1), device=param.device, dtype=torch.float32)
        theta_inv = torch.empty_like(theta)
        cfg_arr = _lib.float_array(cfg)
        _lib.check(_lib.load().advchain_affine_theta_fwd(_ptr(param), cfg_arr, float(param_scale), _ptr(theta),
                                                         _ptr(theta_inv), N, nd, _stream()), "affine_theta_fwd")
        ctx.save_for_backward(param)
        ctx.cfg = (cfg_arr, float(param_scale), nd)
        return theta, theta_inv

    @staticmethod
    def backward(ctx, gtheta, gtheta_inv):
        (param,) = ctx.saved_tensors
        cfg_arr, scale, nd = ctx.cfg
        gparam = torch.empty_like(param)
        gtheta = None if gtheta is None else _dev(gtheta, "grad_theta")
        gtheta_inv = None if gtheta_inv is None else _dev(gtheta_inv, "grad_theta_inv")
        _lib.check(_lib.load().advchain_affine_theta_bwd(_ptr(param), cfg_arr, scale, _ptr(gtheta), _ptr(gtheta_inv),
                                                         _ptr(gparam), param.shape[0], nd, _stream()),
                   "affine_theta_bwd")
        return gparam, None, None, None


@_on_tensor_device
def affine_theta(param, cfg, param_scale, nd):
    """(N,5|9) bounded parameters -> (theta, theta^-1), each (N, nd, nd+1)."""
    return _AffineTheta.apply(param, tuple(float(c) for c in cfg), float(param_scale), int(nd))


class _Axpy(torch.autograd.Function):
    """out = x + a * y  (AdvNoise.forward, adv_noise.py:81-84)."""

    @staticmethod
    def forward(ctx, x, y, a):
        ctx.a = a
        return raw_axpy(_dev(x, "x"), _dev(y, "y"), a)

    @staticmethod
    def backward(ctx, g):
        g = _dev(g, "grad")
        gx = g if ctx.needs_input_grad[0] else None
        # (a == 1: 1.0 * g is g, bit for bit -- no launch; the notebook's epsilon for AdvNoise)
        gy = (g if ctx.a == 1.0 else raw_axpy(None, g, ctx.a)) if ctx.needs_input_grad[1] else None
        return gx, gy, None


@_on_tensor_device
def axpy(x, y, a):
    """x + a * y with torch's broadcasting rules (the reference writes ``data + epsilon * param``)."""
    if x.shape != y.shape:
        x, y = torch.broadcast_tensors(x, y)      # raises like torch when the shapes do not broadcast
    _same_device(x, y)
    return _Axpy.apply(x, y, float(a))


class _BiasApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cp, data, tables, eps, use_log, cp_scale):
        cp, data = _dev(cp, "control points"), _dev(data, "data")
        N, C = data.shape[:2]
        out = torch.empty_like(data)
        field = torch.empty((N, 1) + tuple(data.shape[2:]), device=data.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_bias_field_fwd(_ptr(cp), _ptr(data), _ptr(out), _ptr(field), _ptr(tables.itab),
                                                       _ptr(tables.ftab), _lib.dims_array(tables.S),
                                                       _lib.dims_array(tables.g), _lib.dims_array(tables.B), N, C,
                                                       float(eps), int(use_log), float(cp_scale), _stream()),
                   "bias_field_fwd")
        ctx.save_for_backward(cp, data)
        ctx.cfg = (tables, float(eps), int(use_log), float(cp_scale))
        ctx.mark_non_differentiable(field)
        ctx.set_materialize_grads(False)      # (the engine would otherwise zero-fill a full-size gradient for `field`)
        return out, field

    @staticmethod
    def backward(ctx, gout, _gfield):
        cp, data = ctx.saved_tensors
        tables, eps, use_log, cp_scale = ctx.cfg
        need_cp, need_data = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gout is None or not (need_cp or need_data):
            return None, None, None, None, None, None
        N, C = data.shape[:2]
        gdata = torch.empty_like(data) if need_data else None
        dense = getattr(tables, "dense_inner", None)
        if need_cp and BIAS_REDUCED and dense is not None:
            # the x pass of the adjoint inside the backward: one launch, no full-resolution gradient of the field in memory
            wd, lo, WB = dense
            t1 = torch.empty((N, 1) + tuple(data.shape[2:-1]) + (int(tables.g[2]),), device=data.device, dtype=torch.float32)
            rc = _lib.load().advchain_bias_field_bwd_reduced(_ptr(cp), _ptr(data), _ptr(_dev(gout, "grad")), _ptr(t1),
                                                             _ptr(gdata), _ptr(tables.itab), _ptr(tables.ftab),
                                                             _lib.dims_array(tables.S), _lib.dims_array(tables.g),
                                                             _lib.dims_array(tables.B), N, C, eps, use_log, cp_scale,
                                                             _ptr(wd), _ptr(lo), WB, 0, _stream())
            if rc != -2:
                _lib.check(rc, "bias_field_bwd_reduced")
                return raw_tp_adjoint_from_t1(t1, tables).reshape(cp.shape), gdata, None, None, None, None
        gL = torch.empty((N, 1) + tuple(data.shape[2:]), device=data.device, dtype=torch.float32) if need_cp else None
        _lib.check(_lib.load().advchain_bias_field_bwd(_ptr(cp), _ptr(data), _ptr(_dev(gout, "grad")), _ptr(gL),
                                                       _ptr(gdata), _ptr(tables.itab), _ptr(tables.ftab),
                                                       _lib.dims_array(tables.S), _lib.dims_array(tables.g),
                                                       _lib.dims_array(tables.B), N, C, eps, use_log, cp_scale,
                                                       _stream()), "bias_field_bwd")
        gcp = raw_tp_adjoint(gL, tables).reshape(cp.shape) if need_cp else None
        return gcp, gdata, None, None, None, None


@_on_tensor_device
def bias_apply(cp, data, tables, eps, use_log=True, cp_scale=1.0):
    """(data * clipped_bias_field(cp), clipped_bias_field)."""
    if cp.shape[0] != data.shape[0] or tuple(data.shape[2:]) != tuple(tables.full_dims) \
            or tuple(cp.shape[2:]) != tuple(int(g) for g in tables.g[3 - tables.ndim:]):
        raise RuntimeError("bias field: control points %s / data %s do not match the configured lattice %s -> image %s"
                           % (list(cp.shape), list(data.shape), list(tables.g[3 - tables.ndim:]),
                              list(tables.full_dims)))
    _same_device(cp, data)
    return _BiasApply.apply(cp, data, tables, eps, use_log, cp_scale)


@_on_tensor_device
def bias_field_only(cp, tables, eps, use_log=True, cp_scale=1.0):
    cp = _dev(cp.detach(), "control points")
    N = cp.shape[0]
    field = torch.empty((N, 1) + tuple(tables.full_dims), device=cp.device, dtype=torch.float32)
    _lib.check(_lib.load().advchain_bias_field_fwd(_ptr(cp), None, None, _ptr(field), _ptr(tables.itab),
                                                   _ptr(tables.ftab), _lib.dims_array(tables.S),
                                                   _lib.dims_array(tables.g), _lib.dims_array(tables.B), N, 1,
                                                   float(eps), int(use_log), float(cp_scale), _stream()),
               "bias_field_fwd")
    return field


class _DemonsField(torch.autograd.Function):
    """Low-res velocity -> un-clamped sampling grid (DemonsCompose, adv_morph.py:454-491).

    forward:  gauss(scale*v) -> linear upsample -> phi0 = id + u/2^n -> n x (phi <- phi o phi)
              -> pos = (phi_n - phi0) + id -> gauss(border_identity(pos) - id) + id
    The final clamp(-1,1) (adv_morph.py:490, 304-305) is applied by the sampler on load.
    backward: the hand-written adjoint of the same chain (saved: phi_0..phi_{n-1}, pos).

    opts = (num_steps, smooth_iter, sigma, positions_only[, taps]) -- the attributes of AdvMorph the reference reads in
    DemonsCompose (adv_morph.py:236-242,461-471): defaults (8, 1, 1.0, False); taps = the Gaussian window length when it
    is not the rule's 2 * int(4 sigma + 0.5) + 1 (a gaussian_ks above it, adv_morph.py:393-398).  positions_only returns `pos` itself (the
    caller composes it with an initial deformation other than the identity and / or skips the final smoothing)."""

    @staticmethod
    def forward(ctx, vel, scale, tables, nsteps_rule, reduce_sumsq, pair=False, opts=None):
        vel = _dev(vel, "velocity")
        ctx.pair = bool(pair)
        n_base, smooth_iter, sigma, pos_only = (tuple(opts) + (None,))[:4] if opts is not None else (8, 1, 1.0, False)
        w9 = gauss9(sigma, opts[4] if (opts is not None and len(opts) > 4) else None)
        if len(w9) != 9 and not pos_only:
            raise NotImplementedError("the fused final smoothing exists for the 9-tap window only: ask for the positions")
        ctx.opts = (int(smooth_iter), w9, bool(pos_only))
        s1 = None
        # 2D paired fields with the default options: ONE C call enqueues the whole direction (advchain_demons_compose_pair_fwd:
        # the launches of the separate calls below, in their order)
        composite = (COMPOSITE and pair and vel.shape[1] == 2 and not nsteps_rule and int(smooth_iter) == 1 and not pos_only
                     and len(w9) == 9 and vel.is_contiguous() and vel[0, 0].numel() <= 4096
                     and getattr(tables, "dense_inner", None) is not None)
        ctx.composite = composite
        if pair and not composite:      # the batch [v; -v]: both fields of a solver step from one chain; returns (field(+v), field(-v))
            s1 = raw_gauss_small_pair(vel, scale, weights=w9)         # the negated copy is never materialised
            if s1 is None:
                vel = torch.cat([vel, -vel], 0)
        d = vel.shape[1]
        if composite:
            s1 = torch.empty((2 * vel.shape[0],) + tuple(vel.shape[1:]), device=vel.device, dtype=torch.float32)
        elif s1 is None:
            s1 = raw_gauss(vel, d, pre=1, scale=scale, weights=w9)
        for _ in range(int(smooth_iter) - 1):      # smooth_iter > 1 (adv_morph.py:386-387): the same window again
            s1 = raw_gauss(s1, d, weights=w9)
        N = s1.shape[0]
        n = int(n_base)
        plan = _PLAN
        frozen = plan is not None and plan.is_frozen
        norm_rb = None
        if nsteps_rule:  # 3D: whole-batch Frobenius norm of u / 2^n must not exceed 0.5 (adv_morph.py:159-162)
            # pair: the batch is [v; -v] -- the rule is the reference's, over ONE field's batch (both halves agree)
            ss = field_sumsq(s1[:N // 2] if pair else s1, tables, d)
            if reduce_sumsq is not None:
                ss = reduce_sumsq(ss)
            if frozen:       # the recorded count; the replay checks on the device that the rule still gives it
                site = plan.take("nsteps", n_base=n)
                n = site["n"]
                plan.check(torch.sqrt(ss, out=plan.slot(site)), site)
            else:
                # no `.item()` (round 5): the norm travels to the host behind an event of its own while the chain is
                # enqueued with the count the previous field of this shape needed; the count is verified below, once the
                # chain is queued -- the wait is for a kernel at the HEAD of the queue, so it drains nothing -- and only a
                # count that changed (the first call of a shape, an ascent that crosses a power of two) enqueues the chain
                # a second time.  The results are those of the reference's rule either way.
                nkey = (str(s1.device), tuple(s1.shape), int(n_base), HINT_SLOT)
                norm_rb = _Readback(ss.sqrt())
                n = max(n, _NSTEPS_HINT.get(nkey, n))
        mark = None if plan is None else len(plan.pending)
        while True:
            out = _DemonsField._enqueue_chain(ctx, vel, s1, tables, d, n, scale, w9, pos_only, composite, plan, frozen, pair)
            if norm_rb is None:
                break
            norm, want = float(norm_rb.values()[0]), int(n_base)
            while norm / (2.0 ** want) > 0.5:
                want += 1
            norm_rb = None
            _NSTEPS_HINT[nkey] = want
            NSTEPS_STATS["chains"] += 1
            if plan is not None:         # (a frozen plan meets the count first, then the chain: keep that order in the record)
                if want != n:
                    del plan.pending[mark:]
                plan.pending.insert(mark, ("nsteps", dict(n=want, n_base=int(n_base))))
            if want == n:
                break
            NSTEPS_STATS["respeculated"] += 1
            n = want
        return out

    @staticmethod
    def _enqueue_chain(ctx, vel, s1, tables, d, n, scale, w9, pos_only, composite, plan, frozen, pair):
        N = s1.shape[0]
        inv = 1.0 / (2.0 ** n)
        # row m of `disp`: max-slots for the displacement of phis[m], written by the kernel that produces it; row n: the
        # sampling positions `pos`, which bound the returned grid (clipping to [-1,1] and the normalised Gaussian only
        # shrink a displacement).  Read back once (asynchronously): the backward sizes every step exactly from it.
        # (row n + 1, slot 0: the flag of the fused 2D squarings -- 1 when a window moved too far for them and the ordinary
        # launches ran instead; zeroed with the rest by the row-maxima kernel below)
        disp = _persistent_zeros("disp", (n + 2, DISP_SLOTS), vel.device) if ADAPTIVE_HALO else None
        row = (lambda m: None) if disp is None else (lambda m: disp[m])
        # what the squarings of the PREVIOUS field of this shape measured (a field changes little between two ascent
        # steps): picks the forward kernel per squaring, nothing else
        # ... of the same POSITION in the caller's trajectory when it says so (the solver numbers its ascent steps: the field
        # of step i resembles step i of the previous call -- 0.14 / 0.20 / 0.24 / 0.32 px after steps 1..4 at cfg-2 against 0.03
        # for a fresh draw -- far better than it resembles step i - 1 of this call)
        key = (str(s1.device), tuple(s1.shape), n, HINT_SLOT)
        site = None
        if frozen:           # every selection of this chain from the plan (its own recorded displacements, with the margin)
            if disp is None:
                raise PlanMismatch("launch plan: a frozen chain needs the measured displacements (ops.ADAPTIVE_HALO is off)")
            site = plan.take("chain", n=n, d=d)
            hints = site["bounds"].values()
        else:
            pend = _PENDING_BOUNDS.pop(key, None)      # a chain whose backward never ran (the final pass): its read-back, if it has arrived
            if pend is not None and pend.event.query():
                _note_chain_bounds(key, pend.values(), n)
            hints = _CHAIN_HINTS.get(key)
        full = (N, d) + tuple(tables.full_dims)
        phi0 = torch.empty(full, device=vel.device, dtype=torch.float32) if composite else \
            raw_tp_interp(s1, tables, d, add_identity=True, scale=inv, disp_out=row(0))
        # the n squarings: one C call (advchain_expo_chain_fwd), phi_1..phi_{n-1} in one stacked buffer
        fields = torch.empty((n - 1,) + tuple(phi0.shape), device=phi0.device, dtype=torch.float32)
        pos = torch.empty_like(phi0)
        harr = None if hints is None else (ctypes.c_int32 * n)(*[(_hint_bits(hints[m]) >> 8) | (_fine_bits(hints[m]) << 8)
                                                                 for m in range(n)])
        if COUNT_FUSED and harr is not None and disp is not None and FUSE_2D:      # (tests: which formulation the chain takes)
            FUSE_STATS["fused_levels"] += _lib.load().advchain_expo_chain_fused_levels(phi0.shape[0], d, _lib.dims_array(phi0.shape[2:]), n, harr)
        try:
            rows_max = rc = None
            if composite:
                q = torch.empty_like(phi0)
                rows_max = None if disp is None else (plan.slot(site) if site is not None else
                                                      torch.empty(disp.shape[0], device=vel.device, dtype=torch.float32))
                rc = _lib.load().advchain_demons_compose_pair_fwd(
                    _ptr(vel), _ptr(s1), _ptr(phi0), _ptr(fields), _ptr(pos), _ptr(q), _ptr(disp), _ptr(rows_max), _ptr(tables.itab),
                    _ptr(tables.ftab), _lib.dims_array(tables.S), _lib.dims_array(tables.g), _lib.dims_array(tables.B),
                    vel.shape[0], d, n, harr, w9, float(scale), float(inv), int(bool(FUSE_2D)), _stream())
                if rc == -2:        # (a launch would not take the shape; nothing was enqueued: the separate calls)
                    composite = ctx.composite = False
                    raw_gauss_small_pair_into(vel, s1, scale, w9)
                    raw_tp_interp(s1, tables, d, add_identity=True, scale=inv, disp_out=row(0), out=phi0)
                else:
                    _lib.check(rc, "demons_compose_pair_fwd")
            if not composite:
                _lib.check(_lib.load().advchain_expo_chain_fwd(_ptr(phi0), _ptr(fields), _ptr(pos), phi0.shape[0], d,
                                                               _lib.dims_array(phi0.shape[2:]), n, _ptr(disp), harr,
                                                               None if (disp is None or not FUSE_2D) else _ptr(disp[n + 1]), _stream()),
                           "expo_chain_fwd")
                q = pos if pos_only else raw_gauss(pos, d, pre=2, post=1, weights=w9)
                rows_max = None if disp is None else raw_slot_rows_max(disp, reset=True, out=None if site is None else plan.slot(site))
        except BaseException:
            # (the slots, the fused-chain flag and its barrier counter may hold partial state: the next chain starts from a
            # fresh zero-filled accumulator)
            if disp is not None:
                _forget_persistent(disp)
            raise
        ctx.save_for_backward(pos, phi0, fields)
        ctx.frozen = site is not None
        if site is not None:
            plan.check(rows_max, site)
            ctx.disp = site["bounds"]
        else:
            ctx.disp = None if rows_max is None else _Readback(rows_max)
            if ctx.disp is not None:
                _PENDING_BOUNDS[key] = ctx.disp
                if plan is not None:
                    plan.note("chain", rb=ctx.disp, n=n, d=d)
        global _LAST_FIELD_BOUND
        _LAST_FIELD_BOUND = None if ctx.disp is None else (ctx.disp, n)
        ctx.cfg = (scale, tables, inv, d)
        ctx.nsteps = n
        ctx.hint_key = key
        if pair:
            return q[:N // 2], q[N // 2:]
        return q

    @staticmethod
    def backward(ctx, *grads):
        pos, phi0, fields = ctx.saved_tensors
        scale, tables, inv, d = ctx.cfg
        # pair: one contiguous gradient for the batch [v; -v] (autograd's own route -- two slice_backward zero-fills of
        # the whole batch, two copies and an add per chain -- cost more than the concatenation)
        smooth_iter, w9, pos_only = ctx.opts
        gq = tuple(_dev(g, "grad") for g in grads) if ctx.pair else _dev(grads[0], "grad")
        composite = (ctx.composite and TILED_SCATTER and ctx.pair and gq[0].is_contiguous() and gq[1].is_contiguous()
                     and gq[0].shape == gq[1].shape)
        if composite:
            gpos = torch.empty_like(pos)
        elif pos_only:
            gpos = torch.cat(gq, 0) if ctx.pair else gq.contiguous()
        else:
            gpos = raw_gauss(gq, d, post=2, aux=pos, weights=w9)          # adjoint of gauss(border_identity(.) - id) + id
        g = gpos                                          # d/d phi_n
        ws = _scatter_workspace(gpos.shape[0], gpos.shape[2:], gpos.device) if TILED_SCATTER else None
        # squaring m composes a field whose displacement is ~2^(m-n) of the total: the early steps are sub-voxel and
        # take the gather-form adjoint.  The bound is a performance hint only (larger displacements stay correct
        # through the overflow list); it comes from the displacement measured in forward (one 4-byte read-back).
        n = ctx.nsteps
        if ctx.disp is not None:
            dm = ctx.disp.values()
            if not ctx.frozen:
                _PENDING_BOUNDS.pop(ctx.hint_key, None)
                _note_chain_bounds(ctx.hint_key, dm, n)
            halos = [squaring_halo(dm[m], d) for m in range(n - 1, -1, -1)]
        else:
            big = 2 if d == 3 else 16
            halos = [big, big, max(1, big // 2)] + [1 if d == 3 else 2] * n
        halos = halos[:n]
        if composite:      # ONE C call for the whole direction (advchain_demons_compose_pair_bwd: the launches of the calls below)
            N2 = gpos.shape[0]
            S, gg = list(tables.S), list(tables.g)
            g, scratch = torch.empty_like(gpos), torch.empty_like(gpos)
            t1 = torch.empty((N2, d, S[1], gg[2]), device=gpos.device, dtype=torch.float32)
            gs1 = torch.empty((N2, d, gg[1], gg[2]), device=gpos.device, dtype=torch.float32)
            gvel = torch.empty((N2 // 2, d, gg[1], gg[2]), device=gpos.device, dtype=torch.float32)
            wd, wlo, WB = tables.dense_inner
            rc = _lib.load().advchain_demons_compose_pair_bwd(
                _ptr(gq[0]), _ptr(gq[1]), _ptr(pos), _ptr(phi0), _ptr(fields), _ptr(gpos), _ptr(g), _ptr(scratch), _ptr(ws), _ptr(t1),
                _ptr(gs1), _ptr(gvel), (ctypes.c_int32 * n)(*[int(h) for h in halos]), _ptr(tables.itab), _ptr(tables.ftab), _ptr(wd),
                _ptr(wlo), int(WB), _lib.dims_array(S), _lib.dims_array(gg), _lib.dims_array(tables.B), N2 // 2, d, n, w9, float(scale),
                float(inv), _stream())
            if rc != -2:
                _lib.check(rc, "demons_compose_pair_bwd")
                return gvel, None, None, None, None, None, None
            gpos = raw_gauss(gq, d, post=2, aux=pos, weights=w9)       # (nothing was enqueued: the separate calls)
            g = gpos
        if ws is None:     # (global-atomic A/B path: per-step calls with zero-filled outputs)
            phis = [phi0] + list(fields.unbind(0))
            for i, phi in enumerate(reversed(phis)):
                g = raw_compose_self_bwd(g, phi, None, chain=False, halo=halos[i])
        else:
            g, scratch = torch.empty_like(gpos), torch.empty_like(gpos)
            _lib.check(_lib.load().advchain_expo_chain_bwd(_ptr(gpos), _ptr(phi0), _ptr(fields), _ptr(g), _ptr(scratch), _ptr(ws),
                                                           (ctypes.c_int32 * n)(*[int(h) for h in halos]), gpos.shape[0], d,
                                                           _lib.dims_array(gpos.shape[2:]), n, _stream()), "expo_chain_bwd")
        # phi0 also enters through '- phi0' (Q1 aliasing): total = g - gpos ; u = (phi0 - id) * 2^n
        gs1 = raw_tp_adjoint(g, tables, gfull2=gpos, scale=inv)
        for _ in range(smooth_iter - 1):           # (the zero-padded symmetric window is its own adjoint)
            gs1 = raw_gauss(gs1, d, weights=w9)
        gvel = raw_gauss_small_pair(gs1, scale, adjoint=True, weights=w9) if ctx.pair else None
        if gvel is None:
            gvel = raw_gauss(gs1, d, pre=1, scale=scale, weights=w9)
            if ctx.pair:
                h = gvel.shape[0] // 2
                gvel = gvel[:h] - gvel[h:]
        return gvel, None, None, None, None, None, None


_LAST_FIELD_BOUND = None
HINT_SLOT = 0      # set by the solver: which step of its loop the next chain belongs to (keys the kernel-selection hints)
FUSE_STATS = {"chains": 0, "refused": 0, "fused_levels": 0}     # chains whose backward read its bounds / whose fused forward squarings fell back / (COUNT_FUSED) squarings the forward chains ran fused
COUNT_FUSED = False   # tests: ask advchain_expo_chain_fused_levels what every forward chain takes (one host call per chain)


class _HintCache(dict):
    """A small bounded map (kernel-selection hints keyed by device and shape; cleared when it outgrows its cap)."""
    CAP = 256

    def __setitem__(self, key, value):
        if len(self) >= self.CAP and key not in self:
            self.clear()
        dict.__setitem__(self, key, value)


_NSTEPS_HINT = _HintCache()    # (device, smoothed velocity shape, n_base) -> the step count the 3D rule gave the last field of that shape
NSTEPS_STATS = {"chains": 0, "respeculated": 0}      # 3D chains enqueued with a guessed count / enqueued again with the right one
_PENDING_BOUNDS = _HintCache()  # chain key -> the read-back of the last forward of that key, until somebody looks at it


def _note_chain_bounds(key, dm, n):
    """The displacements phi_0..phi_n (+ the deficit of the fused 2D squarings) a chain measured become the kernel-selection
    hints of the next chain with the same key."""
    FUSE_STATS["chains"] += 1
    if len(dm) > n + 1 and dm[n + 1] > 0:      # some window could not do all the levels the hints promised
        FUSE_STATS["refused"] += 1
    _CHAIN_HINTS[key] = list(dm)


_CHAIN_HINTS = _HintCache()     # (device, velocity shape, n, slot) -> displacement of phi_0..phi_n measured by the last backward of such a chain
_WARP_HINTS = _HintCache()      # (device, spatial dims) -> displacement of the last grid of that shape whose bound was read


def _ride_key(rb, q):
    """Key of the global warp-hint table for a bound riding on grid `q` (None: a frozen plan's bound is not a measurement)."""
    return None if isinstance(rb, _FrozenBounds) else (str(q.device),) + tuple(q.shape[2:])


@_on_tensor_device
def demons_field(vel, scale, tables, nsteps_rule, reduce_sumsq=None, opts=None):
    global _LAST_FIELD_BOUND
    _LAST_FIELD_BOUND = None
    q = _DemonsField.apply(vel, float(scale), tables, bool(nsteps_rule), reduce_sumsq, False, opts)
    if opts is not None and opts[3]:       # positions only: no bound rides on them (the caller composes them further)
        _LAST_FIELD_BOUND = None
        return q
    if _LAST_FIELD_BOUND is not None:      # the displacement bound rides on the grid: no second measurement by the warps
        rb, idx = _LAST_FIELD_BOUND
        q._advchain_disp = [rb, None, q._version, idx, _ride_key(rb, q)]
        _LAST_FIELD_BOUND = None
    return q


class _GaussSmooth(torch.autograd.Function):
    """x -> G * x, the zero-padded separable 9-tap Gaussian of every (n, c) plane (depthwise conv of adv_morph.py:377-452);
    the symmetric window is its own adjoint."""

    @staticmethod
    def forward(ctx, x, sigma, taps=None):
        x = _dev(x, "field")
        ctx.w9 = gauss9(sigma, taps)
        return raw_gauss(x, x.shape[1], weights=ctx.w9)

    @staticmethod
    def backward(ctx, g):
        g = _dev(g, "grad")
        return raw_gauss(g, g.shape[1], weights=ctx.w9), None, None


@_on_tensor_device
def gauss_smooth(x, sigma=1.0, taps=None):
    return _GaussSmooth.apply(x, float(sigma), taps)


class _UpsampleField(torch.autograd.Function):
    """Low-resolution velocity (N,d,g...) -> id + scale * F.interpolate(v, size, linear, align_corners=False)
    (adv_morph.py:464 + 111): the banded tensor-product kernel and its adjoint as one differentiable operator (the fused
    chain calls the same kernels directly)."""

    @staticmethod
    def forward(ctx, coef, tables, scale):
        coef = _dev(coef, "velocity")
        ctx.tables, ctx.scale = tables, float(scale)
        return raw_tp_interp(coef, tables, coef.shape[1], add_identity=True, scale=float(scale))

    @staticmethod
    def backward(ctx, g):
        return raw_tp_adjoint(_dev(g, "grad").contiguous(), ctx.tables, scale=ctx.scale), None, None


@_on_tensor_device
def upsample_field(coef, tables, scale):
    return _UpsampleField.apply(coef, tables, float(scale))


@_on_tensor_device
def demons_field_pair(vel, scale, tables, nsteps_rule, reduce_sumsq=None, opts=None):
    """(field(+scale * vel), field(-scale * vel)): the deformation and its approximate inverse, which one solver step
    always needs together (adv_morph.py:285-331), integrated as ONE batch [v; -v] -- half the launches, each twice the
    size (the 2D kernels of a 32-image batch are too small to fill 256 CUs).  Per sample the arithmetic is that of two
    separate calls: -(s*v) == (-s)*v exactly, so the results are bit-identical to demons_field(vel, +-scale)."""
    global _LAST_FIELD_BOUND
    _LAST_FIELD_BOUND = None
    qp, qm = _DemonsField.apply(vel, float(scale), tables, bool(nsteps_rule), reduce_sumsq, True, opts)
    if _LAST_FIELD_BOUND is not None:      # one bound for both halves (the max over the pair: still exact)
        rb, idx = _LAST_FIELD_BOUND
        qp._advchain_disp = [rb, None, qp._version, idx, _ride_key(rb, qp)]
        qm._advchain_disp = [rb, None, qm._version, idx, _ride_key(rb, qm)]
        _LAST_FIELD_BOUND = None
    return qp, qm


def _aligned16(*tensors):
    return int(all(t is None or t.data_ptr() % 16 == 0 for t in tensors))


@functools.lru_cache(maxsize=256)
def _ordered_stride(family, N, K, shape, *flags):
    """The family's host-only *_fwd_partials query (per shape: asked once)."""
    fn = getattr(_lib.load(), "advchain_consistency_%s_partials" % family)
    return int(fn(N, K, len(shape), _lib.dims_array(shape), *flags))


def _ordered_partials(n, what, device):
    """The [4][stride] partial buffer of a *_fwd_ord entry and the host array that receives the rows' counts.  An ordinary
    temporary: inside a hip-graph capture it comes from the capture's allocations.  Nothing to clear."""
    if n < 0:
        raise ValueError("bad loss shape for %s" % what)
    stride = max(1, int(n))
    return torch.empty(4 * stride, device=device, dtype=torch.float32), stride, (ctypes.c_int32 * 4)()


class _Consistency(torch.autograd.Function):
    """c_mse * S0 + c_a * SA + c_b * SB + c_kl * SKL  with  S0 = sum((P m - T m)^2), SA/SB = masked edge energies,
    SKL = sum m T' (log T' - log P)  (advchain/common/loss.py:55-79,102-220,223-249).  Differentiable w.r.t. the
    prediction logits (one launch of the forward family's own backward entry) and w.r.t. the reference (one launch of
    advchain_consistency_ref_bwd, csrc/loss_ref.hip, for two fp32 operands without weights; the lp / cw family's own ref_bwd
    entry otherwise); each is launched only when its operand needs a gradient.  A reference given as probabilities
    (ref_is_prob) enters 'mse' and 'contour' as it is and 'kl' through a where() that cuts the graph: with 'kl' alone its
    gradient is None and nothing is launched.  The mask is a constant.
    class_w (a tuple of K floats, or None): constant class weights inside S0, SA/SB (object classes) and SKL -- the cw entries
    of csrc/loss_lp.hip for every K and either storage type; None runs the unweighted families."""

    @staticmethod
    def forward(ctx, pred, ref, mask, coef, ref_is_prob, want_edges, class_w=None):
        pred, ref = _dev_logits(pred, "pred"), _dev_logits(ref, "reference")
        if class_w is not None and len(class_w) != pred.shape[1]:
            raise ValueError("class_w must have %d entries (one per class), got %d" % (pred.shape[1], len(class_w)))
        typed = class_w is not None or pred.dtype != torch.float32 or ref.dtype != torch.float32
        if typed and isinstance(mask, torch.Tensor) and mask.dtype in (torch.bfloat16, torch.float16, torch.float64):
            mask = mask.float()           # (small: the kernels read an fp32 mask)
        mask = None if mask is None else _dev(mask, "mask")
        N, K = pred.shape[:2]
        if typed or K >= WIDE_LOSS_MIN_K:      # run-time K: per-voxel softmax statistics of both operands instead of P and D
            return _Consistency._forward_lp(ctx, pred, ref, mask, coef, ref_is_prob, want_edges, class_w)
        nd = pred.dim() - 2
        dims = _lib.dims_array(pred.shape[2:])
        mch = 1 if mask is None else mask.shape[1]
        need_pred, need_ref = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_grad = need_pred or need_ref
        want_kl = coef[3] != 0.0
        R = None
        if need_grad and want_edges and K > 1:
            R = torch.empty((N, 2 * (K - 1)) + tuple(pred.shape[2:]), device=pred.device, dtype=torch.float32)
        # every output exists before the producer runs, and a failure between producer and consumer (the finisher zeroes
        # the slots again) evicts the shared accumulator instead of leaving partial sums for the next evaluation
        sums = torch.empty(4, device=pred.device, dtype=torch.float32)
        value = torch.empty((), device=pred.device, dtype=torch.float32)
        lib = _lib.load()
        if is_deterministic():
            # the value in a fixed order: the same kernels store one partial per workgroup, the ordered finisher adds them
            # (include/advchain_hip.h, the *_fwd_ord entries); everything the backward reads is what the default mode saves
            args = (N, K, nd, dims, mch, int(ref_is_prob), int(want_edges), int(want_kl), _stream())
            shape = tuple(pred.shape[2:])
            fused = False
            P = D = None
            nf = _ordered_stride("fused_fwd", N, K, shape, int(mask is not None), mch, int(want_edges),
                                 _aligned16(pred, ref, mask, R)) if FUSED_LOSS else -2
            if nf != -2:
                part, stride, counts = _ordered_partials(nf, "consistency_fused_fwd_ord", pred.device)
                rc = lib.advchain_consistency_fused_fwd_ord(_ptr(pred), _ptr(ref), _ptr(mask), _ptr(R), _ptr(part), stride,
                                                            counts, *args)
                fused = rc != -2
                if fused:
                    _lib.check(rc, "consistency_fused_fwd_ord")
            if not fused:
                P = torch.empty_like(pred)
                D = torch.empty_like(pred)
                part, stride, counts = _ordered_partials(_ordered_stride(
                    "fwd", N, K, shape, mch, int(want_edges), _aligned16(pred, ref, mask, P, D, R)), "consistency_fwd_ord",
                    pred.device)
                _lib.check(lib.advchain_consistency_fwd_ord(_ptr(pred), _ptr(ref), _ptr(mask), _ptr(P), _ptr(D), _ptr(R),
                                                            _ptr(part), stride, counts, *args), "consistency_fwd_ord")
            _lib.check(lib.advchain_consistency_finish_ord(_ptr(part), stride, counts, _lib.float_array(coef), _ptr(sums),
                                                           _ptr(value), _stream()), "consistency_finish_ord")
            return _Consistency._save_fp32(ctx, value, sums, pred, ref, mask, R, P, D, fused, coef, mch, ref_is_prob,
                                           want_edges)
        slots = _persistent_zeros("loss", (4, 64), pred.device)   # per-workgroup partials, 64 slots per sum; zeroed by the finisher
        try:
            # f2 fused: one marching kernel straight from the logits, nothing saved but R (K = 2..4, rows of 4j <= 256 voxels)
            rc = lib.advchain_consistency_fused_fwd(_ptr(pred), _ptr(ref), _ptr(mask), _ptr(R), _ptr(slots), N, K, nd, dims, mch,
                                                    int(ref_is_prob), int(want_edges), int(want_kl), _stream()) if FUSED_LOSS else -2
            fused = rc != -2
            if fused:
                _lib.check(rc, "consistency_fused_fwd")
                P = D = None
            else:
                P = torch.empty_like(pred)
                D = torch.empty_like(pred)
                _lib.check(lib.advchain_consistency_fwd(_ptr(pred), _ptr(ref), _ptr(mask), _ptr(P), _ptr(D), _ptr(R),
                                                        _ptr(slots), N, K, nd, dims, mch, int(ref_is_prob),
                                                        int(want_edges), int(want_kl), _stream()), "consistency_fwd")
            _lib.check(lib.advchain_consistency_finish(_ptr(slots), _lib.float_array(coef), _ptr(sums), _ptr(value), 1,
                                                       _stream()), "consistency_finish")
        except BaseException:
            _forget_persistent(slots)
            raise
        return _Consistency._save_fp32(ctx, value, sums, pred, ref, mask, R, P, D, fused, coef, mch, ref_is_prob, want_edges)

    @staticmethod
    def _save_fp32(ctx, value, sums, pred, ref, mask, R, P, D, fused, coef, mch, ref_is_prob, want_edges):
        """What the backward of the K <= 16 fp32 families needs -- the same in both modes."""
        K = pred.shape[1]
        need_pred, need_ref = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_grad = need_pred or need_ref
        if need_grad:
            if fused:
                ctx.save_for_backward(pred, ref, R, mask)
            elif need_ref:
                # the reference side reads the operands themselves (references to the inputs, not copies)
                ctx.save_for_backward(P if need_pred else None, D if need_pred else None, R, mask, pred, ref)
            else:
                ctx.save_for_backward(P, D, R, mask)
        # ref_is_prob: 'kl' sees the reference through a where() -- without 'mse' or 'contour' it has no gradient
        ctx.ref_grad = need_ref and not (ref_is_prob and coef[0] == 0.0 and not (want_edges and K > 1))
        ctx.fused = fused
        ctx.cfg = (coef, mch, int(ref_is_prob))
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)      # (no zero tensor for the gradient of `sums`)
        return value, sums

    @staticmethod
    def _forward_lp(ctx, pred, ref, mask, coef, ref_is_prob, want_edges, class_w=None):
        """At least one operand stored in bf16, class weights, or K >= WIDE_LOSS_MIN_K (csrc/loss_lp.hip): the run-time-K scheme
        for every K, each operand read in its own storage type."""
        N, K = pred.shape[:2]
        nd = pred.dim() - 2
        dims = _lib.dims_array(pred.shape[2:])
        mch = 1 if mask is None else mask.shape[1]
        need_pred, need_ref = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_grad = need_pred or need_ref
        want_kl = coef[3] != 0.0
        R = None
        if need_grad and want_edges and K > 1:
            R = torch.empty((N, 2 * (K - 1)) + tuple(pred.shape[2:]), device=pred.device, dtype=torch.float32)
        sums = torch.empty(4, device=pred.device, dtype=torch.float32)
        value = torch.empty((), device=pred.device, dtype=torch.float32)
        stats = torch.empty((N, 4) + tuple(pred.shape[2:]), device=pred.device, dtype=torch.float32)
        lib = _lib.load()
        cw = None if class_w is None else class_weights_device(class_w, pred.device)
        operands = (_ptr(pred), int(pred.dtype == torch.bfloat16), _ptr(ref), int(ref.dtype == torch.bfloat16), _ptr(mask),
                    _ptr(stats), _ptr(R))
        args = (N, K, nd, dims, mch, int(ref_is_prob), int(want_edges), int(want_kl))
        if is_deterministic():
            # the value in a fixed order (see forward); the ord entry takes class_w (NULL: the unweighted loss)
            part, stride, counts = _ordered_partials(_ordered_stride("lp_fwd", N, K, tuple(pred.shape[2:]), int(want_edges)),
                                                     "consistency_lp_fwd_ord", pred.device)
            slots = None
            name, sums_args, weights = "consistency_lp_fwd_ord", (_ptr(part), stride, counts), (_ptr(cw),)
        else:
            slots = _persistent_zeros("loss", (4, 64), pred.device)
            name, sums_args = "consistency_%s_fwd" % ("lp" if cw is None else "cw"), (_ptr(slots),)
            weights = () if cw is None else (_ptr(cw),)      # (the cw entry: class_w in front of the stream)
        try:
            _lib.check(getattr(lib, "advchain_" + name)(*(operands + sums_args + args + weights + (_stream(),))), name)
            if slots is None:
                _lib.check(lib.advchain_consistency_finish_ord(_ptr(part), stride, counts, _lib.float_array(coef), _ptr(sums),
                                                               _ptr(value), _stream()), "consistency_finish_ord")
            else:
                _lib.check(lib.advchain_consistency_finish(_ptr(slots), _lib.float_array(coef), _ptr(sums), _ptr(value), 1,
                                                           _stream()), "consistency_finish")
        except BaseException:
            if slots is not None:
                _forget_persistent(slots)
            raise
        if need_grad:
            ctx.save_for_backward(pred, ref, R, mask, stats)
        ctx.ref_grad = need_ref and not (ref_is_prob and coef[0] == 0.0 and not (want_edges and K > 1))
        ctx.lp = True
        ctx.cw = cw                 # (a constant of the cache, not an autograd input)
        ctx.cfg = (coef, mch, int(ref_is_prob))
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)
        return value, sums

    @staticmethod
    def _backward_lp(ctx, gloss):
        coef, mch, is_gt = ctx.cfg
        need_pred, need_ref = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.ref_grad
        gs = _dev(gloss.reshape(1), "grad")
        lib = _lib.load()
        pred, ref, R, mask, stats = ctx.saved_tensors
        N, K = pred.shape[:2]
        gpred = gref = None
        cw = ctx.cw
        family = "lp" if cw is None else "cw"
        weights = () if cw is None else (_ptr(cw),)         # (the cw entries: class_w in front of the stream)
        fp32 = cw is None and pred.dtype == torch.float32 and ref.dtype == torch.float32
        for need, side in ((need_pred, "bwd"), (need_ref, "ref_bwd")):
            if not need:
                continue
            out = torch.empty_like(pred if side == "bwd" else ref)     # (the operand's dtype)
            tail = (_ptr(stats), _ptr(R), _ptr(mask), _ptr(gs), _ptr(out), float(coef[0]), float(coef[1]), float(coef[2]),
                    float(coef[3]), is_gt, N, K, pred.dim() - 2, _lib.dims_array(pred.shape[2:]), mch)
            if fp32 and side == "ref_bwd":
                # two fp32 operands, no weights: the kernel of csrc/loss_ref.hip parks its intermediate in the fp32 output, where
                # k_lp_ref_grad recomputes it (438 against 299 us at 32 x 20 x 256 x 256, profiles/r18/loss_fold/summary.md)
                name = "consistency_ref_bwd"
                lib.advchain_set_ref_grad_reg_max_k(int(REF_GRAD_REG_MAX_K))
                rc = lib.advchain_consistency_ref_bwd(_ptr(pred), _ptr(ref), *(tail + (_stream(),)))
            else:
                name = "consistency_%s_%s" % (family, side)
                rc = getattr(lib, "advchain_" + name)(_ptr(pred), int(pred.dtype == torch.bfloat16), _ptr(ref),
                                                      int(ref.dtype == torch.bfloat16), *(tail + weights + (_stream(),)))
            _lib.check(rc, name)
            if side == "bwd":
                gpred = out
            else:
                gref = out
        return gpred, gref, None, None, None, None, None

    @staticmethod
    def backward(ctx, gloss, _gsums):
        if gloss is None:
            return None, None, None, None, None, None, None
        if getattr(ctx, "lp", False):
            return _Consistency._backward_lp(ctx, gloss)
        coef, mch, is_gt = ctx.cfg
        need_pred, need_ref = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.ref_grad
        gs = _dev(gloss.reshape(1), "grad")
        lib = _lib.load()
        gpred = gref = None
        saved = ctx.saved_tensors
        P, D, R, mask = saved[:4]                      # (fused: pred, ref, R, mask)
        pred, ref = (P, D) if ctx.fused else (saved[4:6] if len(saved) > 4 else (None, None))
        if need_pred:
            N, K = P.shape[:2]
            gpred = torch.empty_like(P)
            entry = lib.advchain_consistency_fused_bwd if ctx.fused else lib.advchain_consistency_bwd
            _lib.check(entry(_ptr(P), _ptr(D), _ptr(R), _ptr(mask), _ptr(gs), _ptr(gpred),
                             float(coef[0]), float(coef[1]), float(coef[2]), float(coef[3]),
                             is_gt, N, K, P.dim() - 2, _lib.dims_array(P.shape[2:]), mch, _stream()),
                       "consistency_fused_bwd" if ctx.fused else "consistency_bwd")
        if need_ref:
            N, K = ref.shape[:2]
            gref = torch.empty_like(ref)
            lib.advchain_set_ref_grad_reg_max_k(int(REF_GRAD_REG_MAX_K))      # (process-wide in the library: the knob of this module)
            _lib.check(lib.advchain_consistency_ref_bwd(
                _ptr(pred), _ptr(ref), None, _ptr(R), _ptr(mask), _ptr(gs), _ptr(gref),
                float(coef[0]), float(coef[1]), float(coef[2]), float(coef[3]), is_gt, N, K, ref.dim() - 2,
                _lib.dims_array(ref.shape[2:]), mch, _stream()), "consistency_ref_bwd")
        return gpred, gref, None, None, None, None, None


@_on_tensor_device
def consistency_sums(pred, ref, mask, coef, ref_is_prob=False, want_edges=True, class_w=None):
    """Returns (coef . sums, sums) with sums = [S_mse, S_edgeA, S_edgeB, S_kl] (device tensor, raw sums); `coef` has 3
    (no 'kl' term) or 4 entries.  class_w: K finite, non-negative host numbers used as given inside the sums (S_mse and S_kl:
    w_k per class; the edge energies: w_i per object class, w_0 unused), or None for the unweighted loss."""
    coef = tuple(float(c) for c in coef)
    if len(coef) == 3:
        coef = coef + (0.0,)
    if class_w is not None:
        class_w = tuple(float(w) for w in class_w)
    return _Consistency.apply(pred, ref, mask, coef, bool(ref_is_prob), bool(want_edges), class_w)


# ---- supervised segmentation losses (csrc/seg_loss.hip) ---------------------------------------------------------------

def _dev_logits(t, name="input"):
    """fp32 or bf16 (a model under autocast) logits; the kernels read bf16 natively."""
    _require_device(t, name)
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.AdvchainHipError("%s must be float32 or bfloat16, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _dev_labels(t, name="target"):
    _require_device(t, name)
    if t.dtype != torch.int64:
        raise RuntimeError("%s: expected labels of scalar type Long (int64), got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _class_weight_tensor(weight, K, device):
    """K class weights (tensor, list or array) as a flat fp32 tensor on `device`; None stays None."""
    if weight is None:
        return None
    if isinstance(weight, torch.Tensor):
        weight = weight.detach().to(device=device, dtype=torch.float32)
    else:
        weight = torch.as_tensor(weight, dtype=torch.float32).to(device)
    weight = weight.reshape(-1).contiguous()
    if weight.numel() != K:
        raise ValueError("weight must have %d entries, got %d" % (K, weight.numel()))
    return weight


def _labels_or_soft(x, target, label_msg, neither_msg):
    """(labels, None) for an int64 label target (N,dims) of the logits x (N,K,dims), (None, soft) for an fp32 soft target of x's
    shape.  label_msg takes (expected shape, shape found); neither_msg is the NotImplementedError of any other rank."""
    if target.dim() == x.dim() - 1:
        want = (x.shape[0],) + tuple(x.shape[2:])
        labels = _dev_labels(target, "target")
        if tuple(labels.shape) != want:
            raise ValueError(label_msg % (want, tuple(labels.shape)))
        return labels, None
    if target.dim() == x.dim():
        _require_device(target, "target")
        soft = _dev(target if target.dtype == torch.float32 else target.float(), "target")
        if soft.shape != x.shape:
            raise ValueError("soft target must have the input's shape %s, got %s" % (tuple(x.shape), tuple(soft.shape)))
        return None, soft
    raise NotImplementedError(neither_msg)


def _seg_workspace(N, dims, device):
    n = _lib.load().advchain_seg_loss_workspace(N, len(dims), _lib.dims_array(dims))
    if n < 0:
        raise ValueError("bad loss shape: N=%d, dims=%s" % (N, tuple(dims)))
    return torch.empty(max(int(n), 1), device=device, dtype=torch.float32)


class _CrossEntropy2D(torch.autograd.Function):
    """sum over pixels of -log_softmax(x)_y * w_y (labels) or -sum_c w_c t_c log_softmax(x)_c (soft target), over `denom`
    (advchain/common/loss.py:274-326).  Differentiable w.r.t. the logits and a soft target."""

    @staticmethod
    def forward(ctx, x, labels, soft, weight, denom):
        N, K, H, W = x.shape
        dims = _lib.dims_array((H, W))
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        lse = torch.empty((N, H, W), device=x.device, dtype=torch.float32) if need else None
        ws = _seg_workspace(N, (H, W), x.device)
        value = torch.empty((), device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_ce2d_fwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(soft), _ptr(weight),
                                                 _ptr(lse), _ptr(ws), _ptr(value), N, K, dims, float(denom), _stream()),
                   "ce2d_fwd")
        if need:
            ctx.save_for_backward(x, labels, soft, weight, lse)
        ctx.denom = float(denom)
        return value

    @staticmethod
    def backward(ctx, gloss):
        x, labels, soft, weight, lse = ctx.saved_tensors
        N, K, H, W = x.shape
        gs = _dev(gloss.reshape(1), "grad")
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(soft) if (soft is not None and ctx.needs_input_grad[2]) else None
        if gx is None and gt is None:
            return None, None, None, None, None
        _lib.check(_lib.load().advchain_ce2d_bwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(soft), _ptr(weight),
                                                 _ptr(lse), _ptr(gs), _ptr(gx), _ptr(gt), N, K, _lib.dims_array((H, W)),
                                                 ctx.denom, _stream()), "ce2d_bwd")
        return gx, None, gt, None, None


@_on_tensor_device
def cross_entropy_2d(x, target, weight=None, size_average=True):
    """cross_entropy_2D of advchain/common/loss.py:274-326 on the HIP kernels.  x (N,K,H,W) fp32 / bf16 logits; target (N,H,W)
    int64 labels (-100 ignored) or (N,K,H,W) soft target; weight: K class weights (tensor, list or array) or None.  Returns an
    fp32 scalar."""
    x = _dev_logits(x, "input")
    if x.dim() != 4:
        raise ValueError("cross_entropy_2D takes 4-D input (N,C,H,W), got %d-D" % x.dim())
    N, K, H, W = x.shape
    labels, soft = _labels_or_soft(x, target, "label target must be (N,H,W) = %s, got %s",
                                   "cross_entropy_2D: target must be (N,H,W) labels or (N,C,H,W) soft targets")
    weight = _class_weight_tensor(weight, K, x.device)
    _same_device(x, labels, soft, weight)
    denom = float(N * H * W) if size_average else 1.0
    return _CrossEntropy2D.apply(x, labels, soft, weight, denom)


@_on_tensor_device
def cross_entropy_3d(x, target, weight=None, size_average=True):
    """cross_entropy_2D for (N,K,D,H,W) logits: the kernels only use the plane size, so the volume runs as the (N,K,D,H*W)
    view of itself (no copy, no kernel for the view or its gradient).  target: (N,D,H,W) int64 labels or a (N,K,D,H,W) soft
    target."""
    x = _dev_logits(x, "input")
    if x.dim() != 5:
        raise ValueError("cross_entropy_3D takes 5-D input (N,C,D,H,W), got %d-D" % x.dim())
    _require_device(target, "target")
    N, K, D, H, W = x.shape
    if target.dim() == 4:
        if tuple(target.shape) != (N, D, H, W):
            raise ValueError("label target must be (N,D,H,W) = %s, got %s" % ((N, D, H, W), tuple(target.shape)))
        target = target.contiguous().view(N, D, H * W)
    elif target.dim() == 5:
        if target.shape != x.shape:
            raise ValueError("soft target must have the input's shape %s, got %s" % (tuple(x.shape), tuple(target.shape)))
        target = (target if target.dtype == torch.float32 else target.float()).contiguous().view(N, K, D, H * W)
    else:
        raise NotImplementedError("cross_entropy_3D: target must be (N,D,H,W) labels or (N,C,D,H,W) soft targets")
    return cross_entropy_2d(x.view(N, K, D, H * W), target, weight=weight, size_average=size_average)


# ---- soft Dice and fused Dice + cross entropy (csrc/seg_dice.hip) --------------------------------------------------------

class _Dice(torch.autograd.Function):
    """dice_w * soft Dice + ce_w * cross entropy of (N,K,dims) logits (include/advchain_hip.h: advchain_dice_fwd).
    Differentiable w.r.t. the logits and a soft target; three launches forward, one backward."""

    @staticmethod
    def forward(ctx, x, labels, soft, weight, cfg):
        flags, smooth, dice_w, ce_w = cfg
        N, K = x.shape[:2]
        sp = tuple(x.shape[2:])
        dims = _lib.dims_array(sp)
        lib = _lib.load()
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        lse = torch.empty((N,) + sp, device=x.device, dtype=torch.float32) if need else None
        coef = torch.empty((N, K, 2), device=x.device, dtype=torch.float32) if need else None
        n = lib.advchain_dice_workspace(N, K, len(sp), dims)
        if n < 0:
            raise ValueError("bad loss shape: N=%d, K=%d, dims=%s" % (N, K, sp))
        ws = torch.empty(int(n), device=x.device, dtype=torch.float32)
        value = torch.empty((), device=x.device, dtype=torch.float32)
        _lib.check(lib.advchain_dice_fwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(soft), _ptr(weight),
                                         _ptr(lse), _ptr(coef), _ptr(ws), _ptr(value), N, K, len(sp), dims, flags, smooth,
                                         dice_w, ce_w, _stream()), "dice_fwd")
        if need:
            ctx.save_for_backward(x, labels, soft, weight, lse, coef)
        ctx.cfg = cfg
        return value

    @staticmethod
    def backward(ctx, gloss):
        x, labels, soft, weight, lse, coef = ctx.saved_tensors
        _, _, dice_w, ce_w = ctx.cfg
        N, K = x.shape[:2]
        sp = tuple(x.shape[2:])
        gs = _dev(gloss.reshape(1), "grad")
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(soft) if (soft is not None and ctx.needs_input_grad[2]) else None
        if gx is None and gt is None:
            return None, None, None, None, None
        _lib.check(_lib.load().advchain_dice_bwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(soft), _ptr(weight),
                                                 _ptr(lse), _ptr(coef), _ptr(gs), _ptr(gx), _ptr(gt), N, K, len(sp),
                                                 _lib.dims_array(sp), dice_w, ce_w, _stream()), "dice_bwd")
        return gx, None, gt, None, None


@_on_tensor_device
def dice_loss(x, target, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5, dice_weight=1.0, ce_weight=0.0):
    """dice_weight * soft Dice + ce_weight * cross entropy (size_average) on the HIP kernels; ce_weight == 0 is the pure Dice
    loss.  x (N,K,H,W) or (N,K,D,H,W) fp32 / bf16 logits; target: int64 labels (N,dims) (-100: left out of the Dice sums) or a
    soft target of x's shape; weight: K class weights (tensor, list or array) or None.  Returns an fp32 scalar."""
    x = _dev_logits(x, "input")
    if x.dim() not in (4, 5):
        raise ValueError("dice_loss takes 4-D (N,C,H,W) or 5-D (N,C,D,H,W) input, got %d-D" % x.dim())
    _require_device(target, "target")
    N, K = x.shape[:2]
    labels, soft = _labels_or_soft(x, target, "label target must be %s, got %s",
                                   "dice_loss: target must be (N,dims) labels or (N,C,dims) soft targets")
    weight = _class_weight_tensor(weight, K, x.device)
    _same_device(x, labels, soft, weight)
    flags = (1 if ignore_background else 0) | (2 if batch_dice else 0)
    return _Dice.apply(x, labels, soft, weight, (flags, float(smooth), float(dice_weight), float(ce_weight)))


# ---- soft skeletons and the soft-clDice loss (csrc/seg_skeleton.hip) ---------------------------------------------------------

_SKELETON_ROUTES = {None: 0, "fused": 1, "levels": 2}


def _skeleton_route(route, iterations):
    if route not in _SKELETON_ROUTES:
        raise ValueError("route must be None, 'fused' or 'levels', got %r" % (route,))
    if route == "fused" and iterations > SKELETON_FUSED_MAX_ITERATIONS:
        raise ValueError("the fused route takes at most %d iterations, got %d" % (SKELETON_FUSED_MAX_ITERATIONS, iterations))
    return _SKELETON_ROUTES[route]


def _skeleton_workspace(N, K, sp, iterations, what, device):
    n = _lib.load().advchain_skeleton_workspace(N, K, len(sp), _lib.dims_array(sp), iterations, what)
    if n < 0:
        raise ValueError("bad skeleton shape: N=%d, C=%d, dims=%s, iterations=%d" % (N, K, tuple(sp), iterations))
    return torch.empty(max(int(n), 4), device=device, dtype=torch.float32)


class _SoftSkeleton(torch.autograd.Function):
    """Soft skeleton of every plane of (N,C,dims) fp32 maps (include/advchain_hip.h: advchain_soft_skeleton_fwd)."""

    @staticmethod
    def forward(ctx, x, iterations, route):
        N, C = x.shape[:2]
        sp = tuple(x.shape[2:])
        ws = _skeleton_workspace(N, C, sp, iterations, 0, x.device)
        out = torch.empty_like(x)
        _lib.check(_lib.load().advchain_soft_skeleton_fwd(_ptr(x), _ptr(out), _ptr(ws), N, C, len(sp), _lib.dims_array(sp),
                                                          iterations, route, _stream()), "soft_skeleton_fwd")
        ctx.save_for_backward(x)
        ctx.iterations = iterations
        return out

    @staticmethod
    def backward(ctx, gout):
        x, = ctx.saved_tensors
        N, C = x.shape[:2]
        sp = tuple(x.shape[2:])
        g = _dev(gout, "grad")
        ws = _skeleton_workspace(N, C, sp, ctx.iterations, 1, x.device)
        gx = torch.empty_like(x)
        _lib.check(_lib.load().advchain_soft_skeleton_bwd(_ptr(x), _ptr(g), _ptr(gx), _ptr(ws), N, C, len(sp),
                                                          _lib.dims_array(sp), ctx.iterations, _stream()), "soft_skeleton_bwd")
        return gx, None, None


@_on_tensor_device
def soft_skeletonize(maps, iterations=3, route=None):
    """Soft skeleton (iterated min / max pooling, clDice) of every plane of (N,C,H,W) or (N,C,D,H,W) fp32 maps, the bits of the
    published torch composition in fp32; differentiable.  `route` (tests and tools): None, 'fused' or 'levels'."""
    x = _dev(maps, "maps")
    if x.dim() not in (4, 5):
        raise ValueError("soft_skeletonize takes 4-D (N,C,H,W) or 5-D (N,C,D,H,W) maps, got %d-D" % x.dim())
    return _SoftSkeleton.apply(x, int(iterations), _skeleton_route(route, int(iterations)))


class _ClDice(torch.autograd.Function):
    """soft-clDice of (N,K,dims) logits (include/advchain_hip.h: advchain_cldice_fwd); differentiable w.r.t. the logits."""

    @staticmethod
    def forward(ctx, x, labels, soft, weight, cfg):
        iterations, route, flags, smooth = cfg
        N, K = x.shape[:2]
        sp = tuple(x.shape[2:])
        dims = _lib.dims_array(sp)
        need = ctx.needs_input_grad[0]
        ws = _skeleton_workspace(N, K, sp, iterations, 2, x.device)
        lse = torch.empty((N,) + sp, device=x.device, dtype=torch.float32)
        skel_t = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        coef = torch.empty((N, K, 3), device=x.device, dtype=torch.float32) if need else None
        value = torch.empty((), device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_cldice_fwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(soft), _ptr(weight),
                                                   _ptr(lse), _ptr(skel_t), _ptr(coef), _ptr(ws), _ptr(value), N, K, len(sp), dims,
                                                   iterations, route, flags, smooth, _stream()), "cldice_fwd")
        if need:
            ctx.save_for_backward(x, labels, soft, lse, skel_t, coef)
        ctx.iterations = iterations
        return value

    @staticmethod
    def backward(ctx, gloss):
        x, labels, soft, lse, skel_t, coef = ctx.saved_tensors
        N, K = x.shape[:2]
        sp = tuple(x.shape[2:])
        gs = _dev(gloss.reshape(1), "grad")
        ws = _skeleton_workspace(N, K, sp, ctx.iterations, 3, x.device)
        gx = torch.empty_like(x)
        _lib.check(_lib.load().advchain_cldice_bwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(soft), _ptr(lse),
                                                   _ptr(skel_t), _ptr(coef), _ptr(gs), _ptr(gx), _ptr(ws), N, K, len(sp),
                                                   _lib.dims_array(sp), ctx.iterations, _stream()), "cldice_bwd")
        return gx, None, None, None, None


@_on_tensor_device
def cldice_loss(x, target, iterations=3, weight=None, ignore_background=True, batch=False, smooth=1.0, route=None):
    """soft-clDice loss on the HIP kernels.  x (N,K,H,W) or (N,K,D,H,W) fp32 / bf16 logits; target: int64 labels (N,dims) (-100:
    masked out of the sums) or a constant fp32 soft target of x's shape; weight: K class weights or None.  Returns an fp32
    scalar.  `route` (tests and tools): None, 'fused' or 'levels'."""
    x = _dev_logits(x, "input")
    if x.dim() not in (4, 5):
        raise ValueError("cldice_loss takes 4-D (N,C,H,W) or 5-D (N,C,D,H,W) input, got %d-D" % x.dim())
    _require_device(target, "target")
    N, K = x.shape[:2]
    labels, soft = _labels_or_soft(x, target, "label target must be %s, got %s",
                                   "cldice_loss: target must be (N,dims) labels or (N,C,dims) soft targets")
    if soft is not None:
        soft = soft.detach()
    weight = _class_weight_tensor(weight, K, x.device)
    _same_device(x, labels, soft, weight)
    flags = (1 if ignore_background else 0) | (2 if batch else 0)
    return _ClDice.apply(x, labels, soft, weight, (int(iterations), _skeleton_route(route, int(iterations)), flags, float(smooth)))


# ---- Euclidean distance transform, signed distance maps (csrc/edt.hip) and the boundary loss (csrc/seg_boundary.hip) -----------

_MASK_KINDS = {torch.bool: 1, torch.uint8: 1, torch.int64: 2, torch.float32: 3}


def _sampling_array(sampling, ndim):
    return None if sampling is None else _lib.float_array([float(s) for s in sampling])


def _edt_check(rc, what, sp):
    if rc == -2:
        raise NotImplementedError("%s: spatial shape %s is too large for the distance fields (%s)"
                                  % (what, tuple(sp), _lib.load().advchain_last_error().decode()))
    _lib.check(rc, what)


@_on_tensor_device
def distance_transform_edt(mask, sampling=None, squared=False):
    """Exact Euclidean distance transform of every leading entry of mask (B,H,W) / (B,D,H,W) (bool, uint8, int64 or fp32;
    nonzero is foreground): fp32 distance to the nearest zero voxel (include/advchain_hip.h: advchain_edt)."""
    _require_device(mask, "mask")
    if mask.dtype not in _MASK_KINDS:
        raise _lib.AdvchainHipError("mask must be bool, uint8, int64 or float32, got %s" % mask.dtype)
    mask = mask.detach()
    mask = mask if mask.is_contiguous() else mask.contiguous()
    sp = tuple(mask.shape[1:])
    out = torch.empty(mask.shape, device=mask.device, dtype=torch.float32)
    if mask.numel() == 0:
        raise ValueError("distance_transform_edt: empty mask %s" % (tuple(mask.shape),))
    _edt_check(_lib.load().advchain_edt(_ptr(mask), _MASK_KINDS[mask.dtype], _sampling_array(sampling, len(sp)), int(bool(squared)),
                                        _ptr(out), mask.shape[0], len(sp), _lib.dims_array(sp), _stream()), "edt", sp)
    return out


@_on_tensor_device
def signed_distance_maps(labels, num_classes, sampling=None):
    """(N,dims) int64 labels -> (N,K,dims) fp32 signed Euclidean distance maps, positive outside a class and negative inside
    (include/advchain_hip.h: advchain_signed_maps)."""
    labels = _dev_labels(labels.detach() if isinstance(labels, torch.Tensor) else labels, "target")
    N, K = labels.shape[0], int(num_classes)
    sp = tuple(labels.shape[1:])
    lib = _lib.load()
    dims = _lib.dims_array(sp)
    n = lib.advchain_signed_maps_workspace(N, K, len(sp), dims)
    if n < 0:
        raise NotImplementedError("signed_distance_maps: N=%d, K=%d, spatial shape %s is too large for the distance fields (an axis "
                                  "above 32767 -- 8192 for the leading axes -- or a squared diagonal of 2^30 or more)" % (N, K, sp))
    ws = torch.empty(int(n), device=labels.device, dtype=torch.float32)
    out = torch.empty((N, K) + sp, device=labels.device, dtype=torch.float32)
    _edt_check(lib.advchain_signed_maps(_ptr(labels), _sampling_array(sampling, len(sp)), _ptr(out), _ptr(ws), N, K, len(sp), dims,
                                        _stream()), "signed_maps", sp)
    return out


SurfaceMetrics = collections.namedtuple("SurfaceMetrics", ["hausdorff", "hausdorff_percentile", "assd", "directed", "surface_voxels",
                                                          "max_squared", "overlap", "dice"])


@_on_tensor_device
def surface_distance_metrics(pred, target, num_classes, sampling=None, percentile=95.0):
    """(N,dims) int64 label maps -> SurfaceMetrics of (N,K,...) device tensors: Hausdorff distance, its percentile, the average
    symmetric surface distance, the directed values, counts and Dice of every class (include/advchain_hip.h:
    advchain_surface_metrics).  No gradient."""
    pred = _dev_labels(pred.detach() if isinstance(pred, torch.Tensor) else pred, "pred")
    target = _dev_labels(target.detach() if isinstance(target, torch.Tensor) else target, "target")
    _same_device(pred, target)
    if pred.shape != target.shape:
        raise ValueError("surface_distance_metrics: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    N, K = pred.shape[0], int(num_classes)
    sp = tuple(pred.shape[1:])
    lib = _lib.load()
    dims = _lib.dims_array(sp)
    n = lib.advchain_surface_metrics_workspace(N, K, len(sp), dims)
    if n < 0:
        raise NotImplementedError("surface_distance_metrics: N=%d, K=%d, spatial shape %s is too large for the distance fields (an "
                                  "axis above 32767 -- 8192 for the leading axes -- or a squared diagonal of 2^30 or more)" % (N, K, sp))
    dev = pred.device
    ws = torch.empty(int(n), device=dev, dtype=torch.float32)
    f32 = [torch.empty(s, device=dev, dtype=torch.float32) for s in ((N, K), (N, K), (N, K), (N, K, 2, 3))]
    voxels = torch.empty((N, K, 2), device=dev, dtype=torch.int64)
    max_squared = torch.empty((N, K, 2), device=dev, dtype=torch.float64)
    overlap = torch.empty((N, K, 3), device=dev, dtype=torch.int64)
    dice = torch.empty((N, K), device=dev, dtype=torch.float32)
    _edt_check(lib.advchain_surface_metrics(_ptr(pred), _ptr(target), _sampling_array(sampling, len(sp)), float(percentile),
                                            _ptr(f32[0]), _ptr(f32[1]), _ptr(f32[2]), _ptr(f32[3]), _ptr(voxels), _ptr(max_squared),
                                            _ptr(overlap), _ptr(dice), _ptr(ws), N, K, len(sp), dims, _stream()),
               "surface_metrics", sp)
    return SurfaceMetrics(f32[0], f32[1], f32[2], f32[3], voxels, max_squared, overlap, dice)


# ---- surface Dice at a tolerance (csrc/seg_surface.hip: k_surface_ball, k_surface_within) ---------------------------------------

SurfaceDice = collections.namedtuple("SurfaceDice", ["surface_dice", "within", "surface_voxels"])
# The widest owned tile of the ball kernel by number of spatial axes; a tile that does not fit in LDS with its halo is halved
# along the leading axes (kBallTiles2 / kBallTiles3 of the source): every seam of this tile is a seam of the narrower ones, which
# add seams of their own at the multiples of their sizes (tests/test_surface_dice_gpu.py runs each of them).
SURFACE_DICE_TILE = {2: (32, 64), 3: (8, 8, 32)}
_DICE_ROUTES = {None: 0, "ball": 1, "fields": 2}
_DICE_THRESHOLDS = {}


def surface_dice_tolerances(name, tolerance, num_classes):
    """`tolerance` -- one finite real number >= 0 (a Python or numpy scalar, not a bool), or num_classes of them as a list, a
    tuple, a 1-D numpy array or a 1-D tensor -- as a tuple of num_classes floats, or ValueError.  (A tensor is read on the host:
    pass numbers where the call must not synchronise.)"""
    K = int(num_classes)
    rule = "tolerance must be one finite real number >= 0 or a list, tuple or 1-D array / tensor of %d of them" % K
    if isinstance(tolerance, (torch.Tensor, np.ndarray)):
        boolean = tolerance.dtype == (torch.bool if isinstance(tolerance, torch.Tensor) else np.dtype(bool))
        if tolerance.ndim != 1 or boolean:
            raise ValueError("%s: %s, got a %s array of shape %s" % (name, rule, tolerance.dtype, tuple(tolerance.shape)))
        tolerance = tolerance.detach().cpu().tolist() if isinstance(tolerance, torch.Tensor) else tolerance.tolist()
    scalar = not isinstance(tolerance, (list, tuple))
    vals = [tolerance] if scalar else list(tolerance)
    if not scalar and len(vals) != K:
        raise ValueError("%s: tolerance has the wrong length: %d numbers for %d classes" % (name, len(vals), K))
    for v in vals:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
            raise ValueError("%s: %s, got %r" % (name, rule, tolerance))
    return tuple(float(v) for v in vals) * (K if scalar else 1)


def surface_dice_threshold_words(tolerances, unit):
    """The 32-bit word per class that the kernels compare squared distances with.  Unit spacing: the integer
    min(floor(tau * tau), 2^30 - 1), taken in float64.  With a sampling: the bits of tau * tau rounded to fp32 once (at most
    1e29)."""
    words = []
    for t in tolerances:
        t2 = float(t) * float(t)
        if unit:
            words.append(2 ** 30 - 1 if t2 >= 2 ** 30 - 1 else int(math.floor(t2)))
        else:
            words.append(struct.unpack("<I", struct.pack("<f", min(t2, 1.0e29)))[0])
    return tuple(words)


def surface_dice_thresholds_device(words, device):
    """The K threshold words as K int32 on the device, cached per (device, words) the way class weights are: one host-device
    copy at the first use, none after it.  Read-only.  The cache holds the 64 vectors used last and drops the oldest one for a
    new one; a frozen plan keeps the tensor its capture read alive, a bare torch.cuda.graph capture does not -- see
    common.metrics.surface_dice."""
    key = (str(device), words)
    t = _DICE_THRESHOLDS.pop(key, None)
    if t is not None:
        _DICE_THRESHOLDS[key] = t                      # (most recently used last)
    else:
        if len(_DICE_THRESHOLDS) >= 64:
            _DICE_THRESHOLDS.pop(next(iter(_DICE_THRESHOLDS)))
        # (words above 2^31 - 1 do not occur: fp32 bits of a non-negative number and integers below 2^30)
        t = _DICE_THRESHOLDS[key] = torch.tensor(words, dtype=torch.int32, device=device)
    plan = _PLAN
    if plan is not None and plan.is_frozen:
        plan.persistent.setdefault(("surface_dice_thr",) + key, t)
    return t


def _surface_dice_refused(N, K, sp, route):
    msg = _lib.load().advchain_last_error().decode()
    if route == "ball":
        return NotImplementedError("surface_dice: N=%d, K=%d, spatial shape %s: %s" % (N, K, tuple(sp), msg))
    return NotImplementedError("surface_dice: N=%d, K=%d, spatial shape %s is too large for the distance fields (an axis above "
                               "32767 -- 8192 for the leading axes -- or a squared diagonal of 2^30 or more)" % (N, K, tuple(sp)))


def surface_dice_route(N, K, spatial_shape, tolerance, sampling=None, route=None):
    """"ball" or "fields": the route surface_dice takes for these sizes (a host-only query of the library, no GPU), or
    NotImplementedError where no route can take them."""
    if route not in _DICE_ROUTES:
        raise ValueError("surface_dice: route must be None, 'ball' or 'fields', got %r" % (route,))
    sp = tuple(int(s) for s in spatial_shape)
    tol = surface_dice_tolerances("surface_dice", tolerance, K)
    lib = _lib.load()
    rc = lib.advchain_surface_dice_route(int(N), int(K), len(sp), _lib.dims_array(sp), _sampling_array(sampling, len(sp)), max(tol),
                                         _DICE_ROUTES[route])
    if rc == -2:
        raise _surface_dice_refused(N, K, sp, route)
    if rc not in (1, 2):
        _lib.check(rc, "surface_dice")
    return "ball" if rc == 1 else "fields"


@_on_tensor_device
def surface_dice(pred, target, num_classes, tolerance, sampling=None, route=None):
    """(N,dims) int64 label maps -> SurfaceDice(surface_dice (N,K) fp32, within (N,K,2) int64, surface_voxels (N,K,2) int64): the
    normalised surface Dice at a tolerance of every class (include/advchain_hip.h: advchain_surface_dice).  `route` (tests and
    tools only): None dispatches, "ball" or "fields" forces a route; a forced ball that is not eligible raises
    NotImplementedError.  No gradient."""
    pred = _dev_labels(pred.detach() if isinstance(pred, torch.Tensor) else pred, "pred")
    target = _dev_labels(target.detach() if isinstance(target, torch.Tensor) else target, "target")
    _same_device(pred, target)
    if pred.shape != target.shape:
        raise ValueError("surface_dice: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    if route not in _DICE_ROUTES:
        raise ValueError("surface_dice: route must be None, 'ball' or 'fields', got %r" % (route,))
    N, K = pred.shape[0], int(num_classes)
    sp = tuple(pred.shape[1:])
    tol = surface_dice_tolerances("surface_dice", tolerance, K)
    lib = _lib.load()
    dims = _lib.dims_array(sp)
    samp = _sampling_array(sampling, len(sp))
    n = lib.advchain_surface_dice_workspace(N, K, len(sp), dims, samp, max(tol), _DICE_ROUTES[route])
    if n < 0:
        rc = lib.advchain_surface_dice_route(N, K, len(sp), dims, samp, max(tol), _DICE_ROUTES[route])
        if rc == -2:
            raise _surface_dice_refused(N, K, sp, route)
        _lib.check(rc, "surface_dice")
    dev = pred.device
    thr = surface_dice_thresholds_device(surface_dice_threshold_words(tol, sampling is None), dev)
    ws = torch.empty(int(n), device=dev, dtype=torch.float32) if n > 0 else None
    out = torch.empty((N, K), device=dev, dtype=torch.float32)
    within = torch.empty((N, K, 2), device=dev, dtype=torch.int64)
    voxels = torch.empty((N, K, 2), device=dev, dtype=torch.int64)
    rc = lib.advchain_surface_dice(_ptr(pred), _ptr(target), samp, _ptr(thr), max(tol), _DICE_ROUTES[route], _ptr(out),
                                   _ptr(within), _ptr(voxels), _ptr(ws), N, K, len(sp), dims, _stream())
    if rc == -2:
        raise _surface_dice_refused(N, K, sp, route)
    _lib.check(rc, "surface_dice")
    return SurfaceDice(out, within, voxels)


# ---- connected components and the filters on them (csrc/seg_components.hip) ------------------------------------------------------

Components = collections.namedtuple("Components", ["labels", "count", "sizes"])
# The tiles the labelling resolves in LDS, by number of spatial axes (kTileY2 / kTileZ3, kTileY3, kTileX of the source): pairs
# that straddle them go through the seam pass.
COMPONENTS_TILE = {2: (32, 64), 3: (4, 8, 64)}


def _components_workspace(name, labels):
    """(labels contiguous, N, spatial shape, dims array, int32 workspace) or NotImplementedError for a refused shape."""
    labels = _dev_labels(labels.detach() if isinstance(labels, torch.Tensor) else labels, "labels")
    N, sp = labels.shape[0], tuple(labels.shape[1:])
    dims = _lib.dims_array(sp)
    n = _lib.load().advchain_components_workspace(N, len(sp), dims)
    if n < 0:
        raise NotImplementedError("%s: N=%d, spatial shape %s is too large (more than 2^31 - 1 voxels in an entry, or a workspace "
                                  "of more than 2^31 - 1 words)" % (name, N, sp))
    return labels, N, sp, dims, torch.empty(int(n), device=labels.device, dtype=torch.int32)


def _components_check(rc, what):
    if rc == -2:
        raise NotImplementedError("%s: %s" % (what, _lib.load().advchain_last_error().decode()))
    _lib.check(rc, what)


@_on_tensor_device
def connected_components(labels, connectivity=1, background=0, num_classes=None, return_sizes=False):
    """(N,dims) int64 labels -> Components(labels int32 (N,dims), count int64 (N,), sizes int32 (N,dims) or None): the connected
    components of every entry, numbered from 1 in the order of their smallest voxel (include/advchain_hip.h:
    advchain_components).  No gradient."""
    labels, N, sp, dims, ws = _components_workspace("connected_components", labels)
    out = torch.empty(labels.shape, device=labels.device, dtype=torch.int32)
    count = torch.empty((N,), device=labels.device, dtype=torch.int64)
    sizes = torch.empty(labels.shape, device=labels.device, dtype=torch.int32) if return_sizes else None
    _components_check(_lib.load().advchain_components(_ptr(labels), _ptr(out), _ptr(count), _ptr(sizes), _ptr(ws), N, len(sp), dims,
                                                      int(connectivity), int(background),
                                                      -1 if num_classes is None else int(num_classes), _stream()), "components")
    return Components(out, count, sizes)


@_on_tensor_device
def keep_largest_component(labels, num_classes, connectivity=1, background=0):
    """(N,dims) int64 labels -> the same with every class but `background` reduced to its largest component per entry
    (include/advchain_hip.h: advchain_keep_largest).  No gradient."""
    labels, N, sp, dims, ws = _components_workspace("keep_largest_component", labels)
    K = int(num_classes)
    out = torch.empty_like(labels)
    winners = torch.empty((N, K), device=labels.device, dtype=torch.int64)
    _components_check(_lib.load().advchain_keep_largest(_ptr(labels), _ptr(out), _ptr(ws), _ptr(winners), N, K, len(sp), dims,
                                                        int(connectivity), int(background), _stream()), "keep_largest")
    return out


@_on_tensor_device
def remove_small_components(labels, min_size, connectivity=1, background=0, num_classes=None):
    """(N,dims) int64 labels -> the same with the components of fewer than min_size voxels set to `background`
    (include/advchain_hip.h: advchain_remove_small).  No gradient."""
    labels, N, sp, dims, ws = _components_workspace("remove_small_components", labels)
    out = torch.empty_like(labels)
    _components_check(_lib.load().advchain_remove_small(_ptr(labels), _ptr(out), _ptr(ws), N, len(sp), dims, int(connectivity),
                                                        int(background), -1 if num_classes is None else int(num_classes),
                                                        int(min_size), _stream()), "remove_small")
    return out


Holes = collections.namedtuple("Holes", ["fill", "count", "voxels"])


def _fill_holes(name, labels, num_classes, connectivity, background, max_size, want_out, want_report):
    labels = _dev_labels(labels.detach() if isinstance(labels, torch.Tensor) else labels, "labels")
    N, sp = labels.shape[0], tuple(labels.shape[1:])
    dims = _lib.dims_array(sp)
    lib = _lib.load()
    n = lib.advchain_fill_holes_workspace(N, len(sp), dims)
    if n < 0:
        raise NotImplementedError("%s: N=%d, spatial shape %s is too large (more than 2^31 - 1 voxels in an entry, or a "
                                  "components workspace of more than 2^31 - 1 words)" % (name, N, sp))
    ws = torch.empty(int(n), device=labels.device, dtype=torch.int32)
    K = int(num_classes)
    out = torch.empty_like(labels) if want_out else None
    fill = torch.empty_like(labels) if want_report else None
    count = torch.empty((N, K), device=labels.device, dtype=torch.int64) if want_report else None
    voxels = torch.empty((N, K), device=labels.device, dtype=torch.int64) if want_report else None
    _components_check(lib.advchain_fill_holes(_ptr(labels), _ptr(out), _ptr(fill), _ptr(count), _ptr(voxels), _ptr(ws), N, K,
                                              len(sp), dims, int(connectivity), int(background),
                                              -1 if max_size is None else int(max_size), _stream()), "fill_holes")
    return out, Holes(fill, count, voxels)


@_on_tensor_device
def fill_holes(labels, num_classes, connectivity=1, background=0, max_size=None):
    """(N,dims) int64 labels -> the same with every hole -- a component of `background` that does not touch the border of its entry
    and is enclosed by one class in [0, num_classes) -- set to that class (include/advchain_hip.h: advchain_fill_holes).  No
    gradient."""
    return _fill_holes("fill_holes", labels, num_classes, connectivity, background, max_size, True, False)[0]


@_on_tensor_device
def find_holes(labels, num_classes, connectivity=1, background=0, max_size=None):
    """(N,dims) int64 labels -> Holes(fill int64 (N,dims): the class a voxel would be filled with, -1 elsewhere; count, voxels
    int64 (N,K): the holes and their voxels per entry and enclosing class).  No gradient."""
    return _fill_holes("find_holes", labels, num_classes, connectivity, background, max_size, False, True)[1]


InstanceMetrics = collections.namedtuple("InstanceMetrics", ["components", "matched", "overlapping", "iou_fixed", "precision",
                                                             "recall", "f1", "sq", "pq", "pred_status", "target_status"])


@_on_tensor_device
def instance_metrics(pred, target, num_classes, iou_threshold=0.5, connectivity=1, background=0, return_maps=False):
    """(N,dims) int64 label maps -> InstanceMetrics: the components of both maps matched per class at IoU > iou_threshold, their
    counts and the detection quotients (include/advchain_hip.h: advchain_instance_match).  No gradient."""
    pred = _dev_labels(pred.detach() if isinstance(pred, torch.Tensor) else pred, "pred")
    target = _dev_labels(target.detach() if isinstance(target, torch.Tensor) else target, "target")
    _same_device(pred, target)
    if pred.shape != target.shape:
        raise ValueError("instance_metrics: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    N, K, sp, dev = pred.shape[0], int(num_classes), tuple(pred.shape[1:]), pred.device
    lib = _lib.load()
    dims = _lib.dims_array(sp)
    n = lib.advchain_instance_match_workspace(N, len(sp), dims)
    if n < 0:
        raise NotImplementedError("instance_metrics: N=%d, spatial shape %s is too large (more than 2^31 - 1 voxels in an entry, or "
                                  "a workspace of more than 2^31 - 1 words)" % (N, sp))
    ws = torch.empty(int(n), device=dev, dtype=torch.int32)
    components = torch.empty((N, K, 2), device=dev, dtype=torch.int64)
    overlapping = torch.empty((N, K, 2), device=dev, dtype=torch.int64)
    matched = torch.empty((N, K), device=dev, dtype=torch.int64)
    iou_fixed = torch.empty((N, K), device=dev, dtype=torch.int64)
    quotients = [torch.empty((N, K), device=dev, dtype=torch.float32) for _ in range(5)]
    status = [torch.empty(pred.shape, device=dev, dtype=torch.uint8) if return_maps else None for _ in range(2)]
    outputs = [components, matched, overlapping, iou_fixed] + quotients + status
    _components_check(lib.advchain_instance_match(_ptr(pred), _ptr(target), *[_ptr(t) for t in outputs], _ptr(ws), N, K, len(sp),
                                                  dims, int(connectivity), int(background), float(iou_threshold), _stream()),
                      "instance_match")
    return InstanceMetrics(*outputs)


Betti = collections.namedtuple("Betti", ["betti", "euler"])
BettiError = collections.namedtuple("BettiError", ["error", "total", "betti", "euler"])


def _betti(name, pred, target, num_classes, connectivity):
    """betti (N,K,M,3), euler (N,K,M), error (N,K,3) or None; M = 1 without a target, else 2 with pred at index 0."""
    pred = _dev_labels(pred.detach() if isinstance(pred, torch.Tensor) else pred, "labels" if target is None else "pred")
    if target is not None:
        target = _dev_labels(target.detach() if isinstance(target, torch.Tensor) else target, "target")
        _same_device(pred, target)
        if pred.shape != target.shape:
            raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(pred.shape), tuple(target.shape)))
    N, K, sp, dev = pred.shape[0], int(num_classes), tuple(pred.shape[1:]), pred.device
    M = 1 if target is None else 2
    lib = _lib.load()
    dims = _lib.dims_array(sp)
    n = lib.advchain_betti_workspace(N, len(sp), dims)
    if n < 0:
        raise NotImplementedError("%s: N=%d, spatial shape %s is too large (more than 2^31 - 1 voxels in an entry, or a workspace "
                                  "of more than 2^31 - 1 words)" % (name, N, sp))
    ws = torch.empty(int(n), device=dev, dtype=torch.int32)
    betti = torch.empty((N, K, M, 3), device=dev, dtype=torch.int64)
    euler = torch.empty((N, K, M), device=dev, dtype=torch.int64)
    error = torch.empty((N, K, 3), device=dev, dtype=torch.int64) if target is not None else None
    _components_check(lib.advchain_betti(_ptr(pred), _ptr(target), _ptr(betti), _ptr(euler), _ptr(error), _ptr(ws), N, K, len(sp),
                                         dims, int(connectivity), _stream()), "betti")
    return betti, euler, error


@_on_tensor_device
def betti_numbers(labels, num_classes, connectivity=1):
    """(N,dims) int64 labels -> Betti(betti int64 (N,K,3): b0, b1, b2; euler int64 (N,K)): the Betti numbers and the Euler
    characteristic of every class in [0, num_classes) (include/advchain_hip.h: advchain_betti).  No gradient."""
    betti, euler, _ = _betti("betti_numbers", labels, None, num_classes, connectivity)
    return Betti(betti.squeeze(2), euler.squeeze(2))


@_on_tensor_device
def betti_error(pred, target, num_classes, connectivity=1):
    """(N,dims) int64 label maps -> BettiError(error int64 (N,K,3): |b_i(pred) - b_i(target)|; total (N,K): its sum over i; betti
    (N,K,2,3) and euler (N,K,2): those of both maps, pred at index 0).  No gradient."""
    betti, euler, error = _betti("betti_error", pred, target, num_classes, connectivity)
    return BettiError(error, error.sum(dim=2), betti, euler)


# ---- confusion matrix and per-class overlap scores, also from logits (csrc/seg_confusion.hip) -----------------------------------

Confusion = collections.namedtuple("Confusion", ["matrix", "pred_only", "target_only", "counted", "labels"])
OverlapMetrics = collections.namedtuple("OverlapMetrics", ["overlap", "counted", "dice", "iou", "precision", "recall", "specificity",
                                                          "labels"])
OverlapScores = collections.namedtuple("OverlapScores", ["overlap", "counted", "dice", "iou", "precision", "recall", "specificity"])
# advchain_confusion_limit(0..4) of the source (tests/test_confusion_cpu.py holds the two sides together)
CONFUSION_TILE = 1024            # voxels a workgroup takes at a time: kTile
CONFUSION_MAX_BLOCKS = 128       # workgroups per entry; from there on a workgroup walks several tiles: kMaxBlocks
CONFUSION_LDS_MAX_K = 127        # the matrix is counted in LDS up to this many classes ((K + 1)^2 words: 64 KB), in global memory above
CONFUSION_MAX_K = 1024           # classes of a matrix (8 MB per entry)
OVERLAP_LDS_MAX_K = 2048         # the 3 K counters of overlap_metrics are in LDS up to this many classes, in global memory above
_PRED_KINDS = {torch.int64: 0, torch.float32: 1, torch.bfloat16: 2}


def confusion_shapes(N, K, reduce_batch):
    """The shapes of Confusion's matrix, pred_only, target_only and counted."""
    lead = () if reduce_batch else (N,)
    return lead + (K, K), lead + (K,), lead + (K,), lead


def _confusion_inputs(name, pred, target, num_classes, return_labels):
    """(pred contiguous, its kind, target contiguous, N, K, spatial shape, dims array, labels or None)."""
    pred = pred.detach() if isinstance(pred, torch.Tensor) else pred
    target = _dev_labels(target.detach() if isinstance(target, torch.Tensor) else target, "target")
    _require_device(pred, "pred")
    if pred.dtype not in _PRED_KINDS:
        raise ValueError("%s: pred must be int64 labels or float32 / bfloat16 logits, got %s" % (name, pred.dtype))
    _same_device(pred, target)
    kind, K = _PRED_KINDS[pred.dtype], int(num_classes)
    N, sp = target.shape[0], tuple(target.shape[1:])
    want = tuple(target.shape) if kind == 0 else (N, K) + sp
    if tuple(pred.shape) != want:
        raise ValueError("%s: pred must have the shape %s for a target %s, got %s" % (name, want, tuple(target.shape), tuple(pred.shape)))
    if return_labels and kind == 0:
        raise ValueError("%s: return_labels needs logits as pred (a label map is its own argmax)" % name)
    pred = pred if pred.is_contiguous() else pred.contiguous()
    labels = torch.empty(target.shape, device=target.device, dtype=torch.int64) if return_labels else None
    return pred, kind, target, N, K, sp, _lib.dims_array(sp), labels


def _confusion_flags(ignore_index, reduce_batch, accumulate=False):
    return (0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index),
            (1 if reduce_batch else 0) | (2 if accumulate else 0))


@_on_tensor_device
def confusion_matrix(pred, target, num_classes, ignore_index=None, reduce_batch=False, out=None, return_labels=False):
    """pred: (N,dims) int64 labels or (N,K,dims) fp32 / bf16 logits; target (N,dims) int64 -> Confusion of int64 device tensors:
    matrix (N,K,K) with rows = truth, pred_only (N,K), target_only (N,K), counted (N,), and labels (N,dims), the argmax map, with
    return_labels (include/advchain_hip.h: advchain_confusion).  out: a Confusion of the same shapes to add into.  No gradient."""
    pred, kind, target, N, K, sp, dims, labels = _confusion_inputs("confusion_matrix", pred, target, num_classes, return_labels)
    if out is None:
        counts = [torch.empty(s, device=target.device, dtype=torch.int64) for s in confusion_shapes(N, K, reduce_batch)]
    else:
        counts = list(out[:4])
        for t, s in zip(counts, confusion_shapes(N, K, reduce_batch)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != s or not t.is_contiguous():
                raise ValueError("confusion_matrix: out must hold contiguous int64 tensors of the shapes %s"
                                 % (confusion_shapes(N, K, reduce_batch),))
        _same_device(target, *counts)
    has_ignore, ignore, flags = _confusion_flags(ignore_index, reduce_batch, out is not None)
    _lib.check(_lib.load().advchain_confusion(_ptr(pred), kind, _ptr(target), _ptr(labels), *[_ptr(t) for t in counts], N, K, len(sp),
                                              dims, has_ignore, ignore, flags, _stream()), "confusion")
    return Confusion(counts[0], counts[1], counts[2], counts[3], labels)


@_on_tensor_device
def overlap_metrics(pred, target, num_classes, ignore_index=None, reduce_batch=False, return_labels=False):
    """pred and target as for confusion_matrix -> OverlapMetrics: overlap (N,K,3) int64 = |A|, |B|, |A n B|, counted (N,) int64,
    dice / iou / precision / recall / specificity (N,K) fp32 and labels (include/advchain_hip.h: advchain_overlap).  No matrix is
    built.  No gradient."""
    pred, kind, target, N, K, sp, dims, labels = _confusion_inputs("overlap_metrics", pred, target, num_classes, return_labels)
    lead, dev = (() if reduce_batch else (N,)), target.device
    overlap = torch.empty(lead + (K, 3), device=dev, dtype=torch.int64)
    counted = torch.empty(lead, device=dev, dtype=torch.int64)
    scores = [torch.empty(lead + (K,), device=dev, dtype=torch.float32) for _ in range(5)]
    has_ignore, ignore, flags = _confusion_flags(ignore_index, reduce_batch)
    _lib.check(_lib.load().advchain_overlap(_ptr(pred), kind, _ptr(target), _ptr(labels), _ptr(overlap), _ptr(counted),
                                            *[_ptr(t) for t in scores], N, K, len(sp), dims, has_ignore, ignore, flags, _stream()),
               "overlap")
    return OverlapMetrics(overlap, counted, *scores, labels)


@_on_tensor_device
def overlap_scores(matrix):
    """(...,K,K) int64 count matrices, rows = truth, taken as complete -> OverlapScores with the leading shape: overlap (...,K,3)
    int64, counted (...) int64 and the five fp32 scores (...,K) (include/advchain_hip.h: advchain_overlap_scores).  No gradient."""
    matrix = _dev_labels(matrix.detach() if isinstance(matrix, torch.Tensor) else matrix, "matrix")
    lead, K = tuple(matrix.shape[:-2]), matrix.shape[-1]
    R = 1
    for s in lead:
        R *= s
    overlap = torch.empty(lead + (K, 3), device=matrix.device, dtype=torch.int64)
    counted = torch.empty(lead, device=matrix.device, dtype=torch.int64)
    scores = [torch.empty(lead + (K,), device=matrix.device, dtype=torch.float32) for _ in range(5)]
    _lib.check(_lib.load().advchain_overlap_scores(_ptr(matrix), _ptr(overlap), _ptr(counted), *[_ptr(t) for t in scores], R, K,
                                                   _stream()), "overlap_scores")
    return OverlapScores(overlap, counted, *scores)


# ---- erosion, dilation, opening and closing with a Euclidean ball (csrc/seg_morph.hip) -----------------------------------------

# The tiles of the morphology kernels by number of spatial axes; None: the axis is not tiled (k_morph_axis stages whole lines).
# Along x the row kernel works in ballots of 64 voxels and the column kernel in tiles of 32 x or a power of two below: every
# multiple of 64 is a seam of both.
MORPH_TILE = {2: (None, 64), 3: (None, None, 64)}
_MORPH_OPS = {"erosion": 0, "dilation": 1, "opening": 2, "closing": 3}


def _morph(name, labels, radius, num_classes, sampling, background):
    labels = _dev_labels(labels.detach() if isinstance(labels, torch.Tensor) else labels, "labels")
    N, K, sp = labels.shape[0], int(num_classes), tuple(labels.shape[1:])
    lib = _lib.load()
    dims = _lib.dims_array(sp)
    n = lib.advchain_morph_workspace(_MORPH_OPS[name], N, K, len(sp), dims)
    if n < 0:
        raise NotImplementedError("%s: N=%d, K=%d, spatial shape %s is too large for the distance fields (an axis above 32767 -- 8192 "
                                  "for the leading axes -- or a squared diagonal of 2^30 or more)" % (name, N, K, sp))
    ws = torch.empty(int(n), device=labels.device, dtype=torch.int32)
    out = torch.empty_like(labels)
    _edt_check(lib.advchain_morph(_ptr(labels), _sampling_array(sampling, len(sp)), float(radius), _MORPH_OPS[name], _ptr(out),
                                  _ptr(ws), N, K, int(background), len(sp), dims, _stream()), name, sp)
    return out


@_on_tensor_device
def erosion(labels, radius, num_classes, sampling=None, background=0):
    """(N,dims) int64 labels -> the same with every class voxel that has another label within `radius` set to `background`
    (include/advchain_hip.h: advchain_morph, op 0).  No gradient."""
    return _morph("erosion", labels, radius, num_classes, sampling, background)


@_on_tensor_device
def dilation(labels, radius, num_classes, sampling=None, background=0):
    """(N,dims) int64 labels -> the same with every background voxel within `radius` of a class voxel set to the class of the
    nearest one, the smaller class among equally near (advchain_morph, op 1).  No gradient."""
    return _morph("dilation", labels, radius, num_classes, sampling, background)


@_on_tensor_device
def opening(labels, radius, num_classes, sampling=None, background=0):
    """(N,dims) int64 labels -> the same with every class voxel outside the opening of its class by the ball set to `background`
    (advchain_morph, op 2).  No gradient."""
    return _morph("opening", labels, radius, num_classes, sampling, background)


@_on_tensor_device
def closing(labels, radius, num_classes, sampling=None, background=0):
    """(N,dims) int64 labels -> the same with every background voxel inside the closing of exactly one class set to that class
    (advchain_morph, op 3).  No gradient."""
    return _morph("closing", labels, radius, num_classes, sampling, background)


class _Boundary(torch.autograd.Function):
    """1/(N V) sum omega_k softmax(x)_k maps_k over the counted voxels and classes (include/advchain_hip.h:
    advchain_boundary_fwd).  Differentiable w.r.t. the logits; the maps are a constant.  Two launches forward, one backward."""

    @staticmethod
    def forward(ctx, x, labels, maps, weight, flags):
        N, K = x.shape[:2]
        sp = tuple(x.shape[2:])
        dims = _lib.dims_array(sp)
        lib = _lib.load()
        need = ctx.needs_input_grad[0]
        saved = torch.empty((N, 2) + sp, device=x.device, dtype=torch.float32) if need else None
        n = lib.advchain_boundary_workspace(N, K, len(sp), dims)
        if n < 0:
            raise ValueError("bad loss shape: N=%d, K=%d, dims=%s" % (N, K, sp))
        ws = torch.empty(int(n), device=x.device, dtype=torch.float32)
        value = torch.empty((), device=x.device, dtype=torch.float32)
        _lib.check(lib.advchain_boundary_fwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(maps), _ptr(weight),
                                             _ptr(saved), _ptr(ws), _ptr(value), N, K, len(sp), dims, flags, _stream()),
                   "boundary_fwd")
        if need:
            ctx.save_for_backward(x, labels, maps, weight, saved)
        ctx.flags = flags
        return value

    @staticmethod
    def backward(ctx, gloss):
        x, labels, maps, weight, saved = ctx.saved_tensors
        N, K = x.shape[:2]
        sp = tuple(x.shape[2:])
        gs = _dev(gloss.reshape(1), "grad")
        gx = torch.empty_like(x)
        _lib.check(_lib.load().advchain_boundary_bwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(labels), _ptr(maps), _ptr(weight),
                                                     _ptr(saved), _ptr(gs), _ptr(gx), N, K, len(sp), _lib.dims_array(sp),
                                                     ctx.flags, _stream()), "boundary_bwd")
        return gx, None, None, None, None


@_on_tensor_device
def boundary_loss(x, target=None, weight=None, ignore_background=True, sampling=None, dist_maps=None):
    """The boundary loss on the HIP kernels.  x (N,K,dims) fp32 / bf16 logits; exactly one of target ((N,dims) int64 labels:
    the maps are computed from them) and dist_maps ((N,K,dims) fp32); weight: K class weights (tensor, list or array) or None.
    Returns an fp32 scalar."""
    x = _dev_logits(x, "input")
    if x.dim() not in (4, 5):
        raise ValueError("boundary_loss takes 4-D (N,C,H,W) or 5-D (N,C,D,H,W) input, got %d-D" % x.dim())
    N, K = x.shape[:2]
    sp = tuple(x.shape[2:])
    labels = None
    if target is not None:
        labels = _dev_labels(target, "target")
        if tuple(labels.shape) != (N,) + sp:
            raise ValueError("label target must be %s, got %s" % ((N,) + sp, tuple(labels.shape)))
        _same_device(x, labels)
        maps = signed_distance_maps(labels, K, sampling)
    else:
        maps = _dev(dist_maps.detach() if isinstance(dist_maps, torch.Tensor) else dist_maps, "dist_maps")
        if maps.shape != x.shape:
            raise ValueError("dist_maps must have the input's shape %s, got %s" % (tuple(x.shape), tuple(maps.shape)))
    weight = _class_weight_tensor(weight, K, x.device)
    _same_device(x, labels, maps, weight)
    return _Boundary.apply(x, labels, maps, weight, 1 if ignore_background else 0)


class _Contour(torch.autograd.Function):
    """Edge energy of u = sum_{c in S}(input_c - T_c) (advchain/common/loss.py:102-220, Q14).  Differentiable w.r.t. the
    prediction and a soft target; the mask is a constant."""

    @staticmethod
    def forward(ctx, x, labels, soft, mask, first_class):
        N, K = x.shape[:2]
        sp = tuple(x.shape[2:])
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        R = torch.empty((N, 2) + sp, device=x.device, dtype=torch.float32) if need else None
        ws = _seg_workspace(N, sp, x.device)
        value = torch.empty((), device=x.device, dtype=torch.float32)
        mch = 1 if mask is None else mask.shape[1]
        _lib.check(_lib.load().advchain_contour_fwd(_ptr(x), _ptr(labels), _ptr(soft), _ptr(mask), _ptr(R), _ptr(ws), _ptr(value),
                                                    N, K, len(sp), _lib.dims_array(sp), int(first_class), mch, _stream()),
                   "contour_fwd")
        if need:
            ctx.save_for_backward(R)
        ctx.cfg = (tuple(x.shape), int(first_class), soft is not None)
        return value

    @staticmethod
    def backward(ctx, gloss):
        R, = ctx.saved_tensors
        shape, first_class, has_soft = ctx.cfg
        gs = _dev(gloss.reshape(1), "grad")
        gx = torch.empty(shape, device=R.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        gt = torch.empty(shape, device=R.device, dtype=torch.float32) if (has_soft and ctx.needs_input_grad[2]) else None
        if gx is None and gt is None:
            return None, None, None, None, None
        _lib.check(_lib.load().advchain_contour_bwd(_ptr(R), _ptr(gs), _ptr(gx), _ptr(gt), shape[0], shape[1], len(shape) - 2,
                                                    _lib.dims_array(shape[2:]), first_class, _stream()), "contour_bwd")
        return gx, None, gt, None, None


@_on_tensor_device
def contour_energy(x, target, mask=None, first_class=1, one_hot_target=True):
    """contour_loss of advchain/common/loss.py:102-220 on the HIP kernels.  x (N,K,dims) fp32; target: labels with N*prod(dims)
    entries (one_hot_target) or a soft target of x's shape; mask (N, 1 or >= K - first_class channels, dims) or None."""
    x = _dev(x, "input")
    N, K = x.shape[:2]
    sp = tuple(x.shape[2:])
    labels = soft = None
    if one_hot_target:
        _require_device(target, "target")
        labels = target if target.dtype == torch.int64 else target.long()
        if labels.numel() != N * (x.numel() // max(N * K, 1)):
            raise ValueError("label target of shape %s does not match the input %s" % (tuple(target.shape), tuple(x.shape)))
        labels = labels.reshape(N, -1).contiguous()
    else:
        soft = _dev(target if target.dtype == torch.float32 else target.float(), "target")
        if soft.shape != x.shape:
            raise ValueError("pred size: %s must match target size: %s" % (tuple(x.shape), tuple(soft.shape)))
    if mask is not None:
        _require_device(mask, "mask")
        mask = _dev(mask.detach() if mask.dtype == torch.float32 else mask.detach().float(), "mask")
        if mask.dim() != x.dim() or mask.shape[0] != N or tuple(mask.shape[2:]) != sp:
            raise ValueError("mask must be (N, C', %s), got %s" % (sp, tuple(mask.shape)))
    _same_device(x, labels, soft, mask)
    return _Contour.apply(x, labels, soft, mask, int(first_class))


@_on_tensor_device
def one_hot(labels, depth):
    """(N, V) int64 labels -> (N, depth, V) fp32 planar one-hot (advchain/common/loss.py:252-271); NaN for out-of-range labels."""
    labels = _dev_labels(labels, "labels")
    N = labels.shape[0]
    V = labels.numel() // max(N, 1)
    out = torch.empty((N, int(depth), V), device=labels.device, dtype=torch.float32)
    _lib.check(_lib.load().advchain_one_hot(_ptr(labels), _ptr(out), N, int(depth), max(V, 1), _stream()), "one_hot")
    return out


# ------------------------------------------------------------------------------------------------
# deformation helpers of adv_morph.py:57-202 (deform_diff.hip, the squaring chain, the sampler)
# ------------------------------------------------------------------------------------------------
def _check_planes(x, what):
    """H and W of at least 2: the reference indexes column / row 1 (adv_morph.py:70-75) and raises IndexError below that."""
    for ax in (3, 2):
        if x.shape[ax] < 2:
            raise IndexError("%s: index 1 is out of bounds for dimension %d with size %d" % (what, ax, x.shape[ax]))


class _ImageDiff2D(torch.autograd.Function):
    """images (N,C,H,W) -> (dx, dy) of calculate_image_diff (adv_morph.py:57-77)."""

    @staticmethod
    def forward(ctx, x):
        x = _dev(x, "images")
        N, C, H, W = x.shape
        dx, dy = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().advchain_image_diff2d_fwd(_ptr(x), _ptr(dx), _ptr(dy), N, C, _lib.dims_array((H, W)), _stream()),
                   "image_diff2d_fwd")
        ctx.set_materialize_grads(False)
        ctx.shape = tuple(x.shape)
        return dx, dy

    @staticmethod
    def backward(ctx, gdx, gdy):
        if gdx is None and gdy is None:
            return None
        gdx = None if gdx is None else _dev(gdx, "grad")
        gdy = None if gdy is None else _dev(gdy, "grad")
        N, C, H, W = ctx.shape
        gin = torch.empty(ctx.shape, device=(gdx if gdx is not None else gdy).device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_image_diff2d_bwd(_ptr(gdx), _ptr(gdy), _ptr(gin), N, C, _lib.dims_array((H, W)),
                                                         _stream()), "image_diff2d_bwd")
        return gin


@_on_tensor_device
def image_diff2d(x):
    """calculate_image_diff (adv_morph.py:57-77) of a (N,C,H,W) fp32 GPU tensor: (dx along W, dy along H)."""
    _check_planes(x, "calculate_image_diff")
    return _ImageDiff2D.apply(x)


class _JacobianDet2D(torch.autograd.Function):
    """(N,2,H,W) displacement -> (N,1,H,W) determinant of calculate_jacobian_determinant (adv_morph.py:80-100); the backward
    recomputes the derivatives from the saved field."""

    @staticmethod
    def forward(ctx, field):
        field = _dev(field, "data")
        N, _, H, W = field.shape
        det = torch.empty((N, 1, H, W), device=field.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_jacobian_det2d_fwd(_ptr(field), _ptr(det), N, _lib.dims_array((H, W)), _stream()),
                   "jacobian_det2d_fwd")
        ctx.save_for_backward(field)
        return det

    @staticmethod
    def backward(ctx, g):
        field, = ctx.saved_tensors
        g = _dev(g, "grad")
        N, _, H, W = field.shape
        gfield = torch.empty_like(field)
        _lib.check(_lib.load().advchain_jacobian_det2d_bwd(_ptr(g), _ptr(field), _ptr(gfield), N, _lib.dims_array((H, W)),
                                                           _stream()), "jacobian_det2d_bwd")
        return gfield


@_on_tensor_device
def jacobian_det2d(field):
    _check_planes(field, "calculate_jacobian_determinant")
    return _JacobianDet2D.apply(field)


# ---- 3D differences, the Jacobian determinant in 2D / 3D and its folding statistics (jacobian.hip) ----
JACOBIAN_COLS = 62           # output columns of one wave (diff_stencil.h: kCols)
JACOBIAN_ROWS_MIN = 4        # rows of one wave's strip: 32, halved down to this while the launch has few waves
JACOBIAN_ROWS_MAX = 32
JACOBIAN_POSITIONS, JACOBIAN_CLAMP = 1, 2        # mode bits of include/advchain_hip.h

JacobianStats = collections.namedtuple("JacobianStats", ["neg", "nonpos", "min", "max"])


def _check_axes(x, what):
    """Every spatial axis of at least 2 elements, as `_check_planes`: the one-sided stencils index element 1."""
    for ax in range(x.dim() - 1, 1, -1):
        if x.shape[ax] < 2:
            raise IndexError("%s: index 1 is out of bounds for dimension %d with size %d" % (what, ax, x.shape[ax]))


def _jacobian_mode(positions, clamp):
    if clamp and not positions:
        raise ValueError("clamp=True clamps a sampling grid to [-1, 1]: it needs positions=True")
    return (JACOBIAN_POSITIONS if positions else 0) | (JACOBIAN_CLAMP if clamp else 0)


class _ImageDiff3D(torch.autograd.Function):
    """(N,C,S0,S1,S2) -> (dx along S2, dy along S1, dz along S0), the stencil of calculate_image_diff on every axis."""

    @staticmethod
    def forward(ctx, x):
        x = _dev(x, "images")
        N, C = x.shape[:2]
        dx, dy, dz = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().advchain_image_diff3d_fwd(_ptr(x), _ptr(dx), _ptr(dy), _ptr(dz), N, C,
                                                         _lib.dims_array(x.shape[2:]), _stream()), "image_diff3d_fwd")
        ctx.set_materialize_grads(False)
        ctx.shape = tuple(x.shape)
        return dx, dy, dz

    @staticmethod
    def backward(ctx, gdx, gdy, gdz):
        grads = [None if g is None else _dev(g, "grad") for g in (gdx, gdy, gdz)]
        first = next((g for g in grads if g is not None), None)
        if first is None:
            return None
        N, C = ctx.shape[:2]
        gin = torch.empty(ctx.shape, device=first.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_image_diff3d_bwd(_ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(gin), N, C,
                                                         _lib.dims_array(ctx.shape[2:]), _stream()), "image_diff3d_bwd")
        return gin


@_on_tensor_device
def image_diff3d(x):
    """(dx, dy, dz) of a (N,C,S0,S1,S2) fp32 GPU tensor: x runs along the last axis, z along the first."""
    assert x.dim() == 5, 'image_diff3d takes (N,C,S0,S1,S2)'
    _check_axes(x, "image_diff3d")
    return _ImageDiff3D.apply(x)


class _JacobianDet(torch.autograd.Function):
    """(N,d,...) field -> (N,1,...) determinant, d = 2 or 3; only the field is saved, the backward recomputes."""

    @staticmethod
    def forward(ctx, field, mode):
        field = _dev(field, "data")
        N, nd = field.shape[0], field.dim() - 2
        det = torch.empty((N, 1) + tuple(field.shape[2:]), device=field.device, dtype=torch.float32)
        _lib.check(_lib.load().advchain_jacobian_det_fwd(_ptr(field), _ptr(det), N, nd, _lib.dims_array(field.shape[2:]), mode,
                                                         _stream()), "jacobian_det_fwd")
        ctx.save_for_backward(field)
        ctx.mode = mode
        return det

    @staticmethod
    def backward(ctx, g):
        field, = ctx.saved_tensors
        g = _dev(g, "grad")
        N, nd = field.shape[0], field.dim() - 2
        lib, dims = _lib.load(), _lib.dims_array(field.shape[2:])
        n_ws = int(lib.advchain_jacobian_det_workspace(N, nd, dims))
        ws = torch.empty(n_ws, device=field.device, dtype=torch.float32) if n_ws > 0 else None
        gfield = torch.empty_like(field)
        _lib.check(lib.advchain_jacobian_det_bwd(_ptr(g), _ptr(field), _ptr(gfield), _ptr(ws), N, nd, dims, ctx.mode, _stream()),
                   "jacobian_det_bwd")
        return gfield, None


def _check_field(field, what):
    assert field.dim() in (4, 5) and field.shape[1] == field.dim() - 2, \
        '%s takes a (N,2,H,W) or (N,3,S0,S1,S2) field, got %s' % (what, tuple(field.shape))
    _check_axes(field, what)


@_on_tensor_device
def jacobian_det(field, positions=False, clamp=False):
    """Determinant of the Jacobian of a 2D or 3D field per voxel, (N,1,...).  Displacement: J = I + D f.  positions=True: the
    field is a sampling grid in normalised coordinates (align_corners=True) and J is in voxel units; clamp=True clamps it to
    [-1, 1] as it is read (the grid a clamped warp samples).  Channel 0 runs along the last axis."""
    _check_field(field, "jacobian_det")
    return _JacobianDet.apply(field, _jacobian_mode(positions, clamp))


@_on_tensor_device
def jacobian_stats(field, positions=False, clamp=False):
    """Folding statistics of `jacobian_det(field, ...)` per batch entry without the map: JacobianStats(neg, nonpos, min, max)
    -- int64 counts of det < 0 and of not (det > 0) (zeros and NaN count), fp32 extrema over the determinants that are numbers.
    Four device tensors of N elements; nothing is read back."""
    _check_field(field, "jacobian_stats")
    mode = _jacobian_mode(positions, clamp)
    field = _dev(field.detach(), "data")
    N, nd = field.shape[0], field.dim() - 2
    neg = torch.empty(N, device=field.device, dtype=torch.int64)
    nonpos = torch.empty(N, device=field.device, dtype=torch.int64)
    mn = torch.empty(N, device=field.device, dtype=torch.float32)
    mx = torch.empty(N, device=field.device, dtype=torch.float32)
    lib, dims = _lib.load(), _lib.dims_array(field.shape[2:])
    ws = torch.empty(max(int(lib.advchain_jacobian_stats_workspace(N, nd, dims)), 4), device=field.device, dtype=torch.float32)
    _lib.check(lib.advchain_jacobian_stats(_ptr(field), _ptr(neg), _ptr(nonpos), _ptr(mn), _ptr(mx), _ptr(ws), N, nd, dims, mode,
                                           _stream()), "jacobian_stats")
    return JacobianStats(neg, nonpos, mn, mx)


def raw_expo_start(duv, inv):
    """phi0 = identity + duv * inv (the start field of vectorFieldExponentiation{2,3}D, adv_morph.py:126-130,153-163)."""
    phi0 = torch.empty_like(duv)
    _lib.check(_lib.load().advchain_expo_start(_ptr(duv), _ptr(phi0), float(inv), duv.shape[0], duv.dim() - 2,
                                               _lib.dims_array(duv.shape[2:]), _stream()), "expo_start")
    return phi0


def sum_of_squares(x):
    """sum(x^2) as a 1-element device tensor, reduced in a fixed order (bitwise the same for the same x)."""
    x = _dev(x, "tensor")
    partials = torch.empty(1024, device=x.device, dtype=torch.float32)     # ADVCHAIN_SUMSQ_PARTIALS
    out = torch.empty(1, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().advchain_sumsq_ordered(_ptr(x), x.numel(), _ptr(partials), _ptr(out), _stream()), "sumsq_ordered")
    return out


class _ExpoStart(torch.autograd.Function):
    @staticmethod
    def forward(ctx, duv, inv):
        ctx.inv = inv
        return raw_expo_start(_dev(duv, "duv"), inv)

    @staticmethod
    def backward(ctx, g):
        return raw_axpy(None, _dev(g, "grad"), ctx.inv), None


class _FieldExponential(torch.autograd.Function):
    """Scaling and squaring of vectorFieldExponentiation{2,3}D (adv_morph.py:116-177) with its aliasing quirk (Q1): returns
    phi_n - phi_0, phi_0 = id + duv / 2^n, phi_{m+1} = phi_m o phi_m.  The squarings are advchain_compose_self_fwd calls (no
    hint: the kernel choice does not change the values), the subtraction advchain_axpy.  phi_0 .. phi_{n-1} are kept only when
    a gradient is wanted.  The backward is advchain_expo_chain_bwd with a FIXED halo per squaring (2D: 0, the window scatter;
    3D: 2, the same): nothing measured selects the kernels, and in deterministic mode two backward calls are bitwise equal."""

    @staticmethod
    def forward(ctx, duv, n, keep):
        N, d = duv.shape[:2]
        ctx.n, ctx.inv = n, 2.0 ** (-n)
        phi0 = raw_expo_start(duv, ctx.inv)
        if n <= 0:          # no squaring: phi - grid_wh of one aliased tensor
            return raw_axpy(phi0, phi0, -1.0)
        fields = torch.empty((n - 1,) + tuple(phi0.shape), device=phi0.device, dtype=torch.float32) if keep else None
        lib, dims = _lib.load(), _lib.dims_array(phi0.shape[2:])
        phi = phi0
        for m in range(1, n + 1):
            nxt = fields[m - 1] if (keep and m < n) else torch.empty_like(phi0)
            _lib.check(lib.advchain_compose_self_fwd(_ptr(phi), _ptr(nxt), None, N, d, dims, 0, None, _stream()),
                       "compose_self_fwd")
            phi = nxt
        if keep:
            ctx.save_for_backward(phi0, fields)
        return raw_axpy(phi, phi0, -1.0)

    @staticmethod
    def backward(ctx, g):
        g = _dev(g, "grad")
        n = ctx.n
        if n <= 0:
            return torch.zeros_like(g), None, None
        phi0, fields = ctx.saved_tensors
        N, d = phi0.shape[:2]
        ws = _scatter_workspace(N, phi0.shape[2:], phi0.device)
        gphi0 = torch.empty_like(phi0)
        scratch = torch.empty_like(phi0) if n > 1 else None
        halos = (ctypes.c_int32 * n)(*([0 if d == 2 else 2] * n))
        _lib.check(_lib.load().advchain_expo_chain_bwd(_ptr(g), _ptr(phi0), _ptr(fields) if n > 1 else None, _ptr(gphi0),
                                                       _ptr(scratch), _ptr(ws), halos, N, d, _lib.dims_array(phi0.shape[2:]), n,
                                                       _stream()), "expo_chain_bwd")
        # phi_0 also enters through '- phi_0' (Q1); d phi_0 / d duv = 2^-n
        return raw_axpy(None, raw_axpy(gphi0, g, -1.0), ctx.inv), None, None


def _resolve_device(device, like):
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev != like.device:
        raise RuntimeError("Expected all tensors to be on the same device, but found at least two devices, %s and %s!"
                           % (dev, like.device))


def field_exponentiation(duv, nb_steps, scaling_squaring, device, nd):
    """vectorFieldExponentiation{2,3}D (adv_morph.py:116-177) of a (N,nd,...) fp32 velocity on its GPU.  3D: the step count
    grows while the whole-batch Frobenius norm of duv / 2^n exceeds 0.5 (Q2; one read-back of a fixed-order sum).  Euler steps
    (2D only; the caller raises for 3D) run through the sampler.  `device` ('cuda' = the CURRENT device, as for the reference's
    grid) must be duv's."""
    duv = _dev(duv, "duv")
    if duv.dim() != nd + 2 or duv.shape[1] != nd:
        raise RuntimeError("vectorFieldExponentiation%dD: expected a velocity of shape (N, %d, ...), got %s"
                           % (nd, nd, tuple(duv.shape)))
    _resolve_device(device, duv)
    return _field_exponentiation(duv, nb_steps, scaling_squaring, nd)


@_on_tensor_device
def _field_exponentiation(duv, nb_steps, scaling_squaring, nd):
    n = int(nb_steps)
    if nd == 3:
        nrm = float(np.sqrt(np.float32(sum_of_squares(duv).item()), dtype=np.float32))
        while nrm / (2.0 ** n) > 0.5:
            n += 1
    if not scaling_squaring:       # Euler: phi <- phi_0 o phi, n times (adv_morph.py:136-141)
        phi0 = _ExpoStart.apply(duv, 2.0 ** (-n))
        phi = phi0
        for _ in range(n):
            phi = grid_sample(phi0, phi, "bilinear", "border")
        return axpy(phi, phi0, -1.0)
    keep = torch.is_grad_enabled() and duv.requires_grad
    return _FieldExponential.apply(duv, n, keep)
