"""ctypes binding of ``libadvchain_hip.so`` (the C ABI declared in ``include/advchain_hip.h``).

There is deliberately NO fallback: if the shared library is missing or a call fails, an exception is
raised.  The product path never routes through PyTorch reference ops or the CPU oracle.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libadvchain_hip.so")

_P, _I, _L, _F, _D = c_void_p, c_int, c_int64, c_float, c_double

# name -> (restype, argtypes).  Must list every symbol of include/advchain_hip.h.
PROTOTYPES = {
    "advchain_version": (_I, []),
    "advchain_last_error": (c_char_p, []),
    "advchain_set_deterministic": (None, [_I]),
    "advchain_get_deterministic": (_I, []),
    "advchain_grid_sample_fwd": (_I, [_P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _I, _P]),
    "advchain_grid_sample_fwd_ride": (_I, [_P, _P, _P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _I, _I, _P]),
    "advchain_scatter_workspace": (_L, [_L, _I, _P]),
    "advchain_grid_sample_bwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _I, _I, _P]),
    "advchain_window_stage_workspace": (_L, [_L, _L, _I, _P]),
    "advchain_grid_sample_bwd_staged": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _I, _I, _P, _P]),
    "advchain_last_bwd_route": (_I, []),
    "advchain_det_warp_workspace": (_L, [_L, _L, _I, _P]),
    "advchain_grid_sample_bwd_det": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _I, _P]),
    "advchain_compose_self_fwd": (_I, [_P, _P, _P, _L, _I, _P, _I, _P, _P]),
    "advchain_compose_self_bwd": (_I, [_P, _P, _P, _P, _I, _I, _L, _I, _P, _P]),
    "advchain_affine_warp_fwd": (_I, [_P, _P, _P, _L, _L, _I, _P, _I, _I, _P]),
    "advchain_affine_warp_fwd_ride": (_I, [_P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _P]),
    "advchain_affine_warp_bwd_workspace": (_L, [_L, _I, _P]),
    "advchain_affine_warp_bwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _P]),
    "advchain_affine_warp_bwd_det": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _P]),
    "advchain_affine_theta_fwd": (_I, [_P, _P, _F, _P, _P, _L, _I, _P]),
    "advchain_affine_theta_bwd": (_I, [_P, _P, _F, _P, _P, _P, _L, _I, _P]),
    "advchain_tp_interp_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _F, _P, _P, _P]),
    "advchain_tp_interp_fwd_smoothed_pair": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _F, _P, _P, _F, _P]),
    "advchain_tp_interp_fwd_smoothed_pair_rows": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _F, _P, _P, _F, _I, _P]),
    "advchain_band_reduce_axis": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _L, _L, _F, _P]),
    "advchain_band_reduce_rows_dense": (_I, [_P, _P, _P, _P, _P, _L, _L, _L, _L, _F, _P]),
    "advchain_bias_field_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _F, _I, _F, _P]),
    "advchain_bias_field_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _F, _I, _F, _P]),
    "advchain_bias_rows_per_wg": (_I, [_P, _L]),
    "advchain_set_tp_wide_loads": (None, [_I]),
    "advchain_get_tp_wide_loads": (_I, []),
    "advchain_tp_wide_band": (_I, [_L]),
    "advchain_bias_field_fwd_rows": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _F, _I, _F, _I, _P]),
    "advchain_bias_field_bwd_rows": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _F, _I, _F, _I, _P]),
    "advchain_bias_field_bwd_reduced": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _F, _I, _F, _P, _P, _L, _I, _P]),
    "advchain_gauss_axis": (_I, [_P, _P, _P, _L, _L, _I, _P, _I, _P, _I, _I, _F, _P]),
    "advchain_gauss_axis_generic": (_I, [_P, _P, _L, _I, _P, _I, _P, _I, _F, _P]),
    "advchain_max_displacement": (_I, [_P, _P, _L, _I, _P, _P]),
    "advchain_grid_sample_bicubic2d_fwd": (_I, [_P, _P, _P, _L, _L, _P, _P, _I, _P]),
    "advchain_grid_sample_bicubic2d_bwd": (_I, [_P, _P, _P, _P, _P, _L, _L, _P, _P, _I, _P]),
    "advchain_affine_grid2d_fwd": (_I, [_P, _P, _L, _P, _P]),
    "advchain_affine_grid2d_bwd_workspace": (_L, [_L, _P]),
    "advchain_affine_grid2d_bwd": (_I, [_P, _P, _P, _L, _P, _P]),
    "advchain_slot_rows_max": (_I, [_P, _P, _L, _L, _I, _P]),
    "advchain_demons_compose_pair_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _F, _F, _I, _P]),
    "advchain_demons_compose_pair_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _L,
                                              _I, _I, _P, _F, _F, _P]),
    "advchain_bounds_check": (_I, [_P, _P, _P, _L, _P, _P]),
    "advchain_expo_chain_fused_levels": (_I, [_L, _I, _P, _I, _P]),
    "advchain_expo_chain_fwd": (_I, [_P, _P, _P, _L, _I, _P, _I, _P, _P, _P, _P]),
    "advchain_expo_chain_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _P, _I, _P]),
    "advchain_gauss_xy": (_I, [_P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _F, _P, _P, _L]),
    "advchain_gauss_xy_staged": (_I, [_P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _F, _P, _P, _L]),
    "advchain_gauss_xy_lanes": (_I, [_P, _P, _P, _L, _L, _I, _P, _P, _I, _I, _F, _P, _P, _L, _I, _I]),
    "advchain_gauss_xy_plan": (_I, [_I, _P, _L, _P, _P, _P]),
    "advchain_gauss_small": (_I, [_P, _P, _L, _I, _P, _P, _I, _F, _P]),
    "advchain_gauss_small_pair": (_I, [_P, _P, _L, _I, _P, _P, _F, _I, _P]),
    "advchain_axpy": (_I, [_P, _P, _P, _F, _L, _P]),
    "advchain_sign_axpy": (_I, [_P, _P, _P, _F, _L, _P, _P, _P]),
    "advchain_nonzero_mask": (_I, [_P, _P, _L, _P]),
    "advchain_consistency_finish": (_I, [_P, _P, _P, _P, _I, _P]),
    "advchain_norm_workspace": (_L, [_L, _L]),
    "advchain_norm_axpy": (_I, [_P, _P, _P, _P, _F, _L, _L, _P]),
    "advchain_norm_axpy_gated": (_I, [_P, _P, _P, _P, _F, _L, _L, _P, _P, _P]),
    "advchain_update_multi": (_I, [_P, _I, _P, _P]),
    "advchain_consistency_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P]),
    "advchain_consistency_bwd": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P]),
    "advchain_consistency_fused_fwd": (_I, [_P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P]),
    "advchain_consistency_fused_bwd": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P]),
    "advchain_consistency_wide_fwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P]),
    "advchain_consistency_wide_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P]),
    "advchain_consistency_ref_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P]),
    "advchain_set_ref_grad_reg_max_k": (None, [_I]),
    "advchain_get_ref_grad_reg_max_k": (_I, []),
    "advchain_consistency_lp_fwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P]),
    "advchain_consistency_lp_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P]),
    "advchain_consistency_lp_ref_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P]),
    # (the lp lists with `const float* class_w` in front of the stream)
    "advchain_consistency_cw_fwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P, _P]),
    "advchain_consistency_cw_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P, _P]),
    "advchain_consistency_cw_ref_bwd": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _P, _F, _F, _F, _F, _I, _L, _L, _I, _P, _I, _P, _P]),
    "advchain_consistency_fused_fwd_bf16": (_I, [_P, _P, _P, _P, _P, _L, _L, _I, _P, _P]),
    "advchain_consistency_fused_bwd_bf16": (_I, [_P, _P, _P, _P, _P, _P, _F, _F, _F, _L, _L, _I, _P, _P]),
    "advchain_seg_loss_workspace": (_L, [_L, _I, _P]),
    "advchain_ce2d_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _L, _L, _P, _F, _P]),
    "advchain_ce2d_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _L, _L, _P, _F, _P]),
    "advchain_contour_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _P]),
    "advchain_contour_bwd": (_I, [_P, _P, _P, _P, _L, _L, _I, _P, _I, _P]),
    "advchain_one_hot": (_I, [_P, _P, _L, _L, _L, _P]),
    "advchain_dice_workspace": (_L, [_L, _L, _I, _P]),
    "advchain_dice_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _F, _F, _F, _P]),
    "advchain_dice_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _F, _F, _P]),
    "advchain_skeleton_workspace": (_L, [_L, _L, _I, _P, _I, _I]),
    "advchain_soft_skeleton_fwd": (_I, [_P, _P, _P, _L, _L, _I, _P, _I, _I, _P]),
    "advchain_soft_skeleton_bwd": (_I, [_P, _P, _P, _P, _L, _L, _I, _P, _I, _P]),
    "advchain_cldice_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _F, _P]),
    "advchain_cldice_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _P]),
    "advchain_edt": (_I, [_P, _I, _P, _I, _P, _L, _I, _P, _P]),
    "advchain_signed_maps_workspace": (_L, [_L, _L, _I, _P]),
    "advchain_signed_maps": (_I, [_P, _P, _P, _P, _L, _L, _I, _P, _P]),
    "advchain_surface_metrics_workspace": (_L, [_L, _L, _I, _P]),
    "advchain_surface_metrics": (_I, [_P, _P, _P, _D, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _P]),
    "advchain_surface_dice_route": (_I, [_L, _L, _I, _P, _P, _D, _I]),
    "advchain_surface_dice_workspace": (_L, [_L, _L, _I, _P, _P, _D, _I]),
    "advchain_surface_dice": (_I, [_P, _P, _P, _P, _D, _I, _P, _P, _P, _P, _L, _L, _I, _P, _P]),
    "advchain_components_workspace": (_L, [_L, _I, _P]),
    "advchain_components": (_I, [_P, _P, _P, _P, _P, _L, _I, _P, _I, _L, _L, _P]),
    "advchain_keep_largest": (_I, [_P, _P, _P, _P, _L, _L, _I, _P, _I, _L, _P]),
    "advchain_remove_small": (_I, [_P, _P, _P, _L, _I, _P, _I, _L, _L, _L, _P]),
    "advchain_fill_holes_workspace": (_L, [_L, _I, _P]),
    "advchain_fill_holes": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _L, _L, _P]),
    "advchain_instance_match_workspace": (_L, [_L, _I, _P]),
    "advchain_instance_match": (_I, [_P] * 14 + [_L, _L, _I, _P, _I, _L, _D, _P]),
    "advchain_betti_workspace": (_L, [_L, _I, _P]),
    "advchain_betti": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _P]),
    "advchain_confusion_limit": (_L, [_I]),
    "advchain_confusion": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _L, _I, _P]),
    "advchain_overlap": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _L, _I, _P]),
    "advchain_overlap_scores": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _P]),
    "advchain_morph_workspace": (_L, [_I, _L, _L, _I, _P]),
    "advchain_morph": (_I, [_P, _P, _D, _I, _P, _P, _L, _L, _L, _I, _P, _P]),
    "advchain_boundary_workspace": (_L, [_L, _L, _I, _P]),
    "advchain_boundary_fwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _P]),
    "advchain_boundary_bwd": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _L, _L, _I, _P, _I, _P]),
    "advchain_image_diff2d_fwd": (_I, [_P, _P, _P, _L, _L, _P, _P]),
    "advchain_image_diff2d_bwd": (_I, [_P, _P, _P, _L, _L, _P, _P]),
    "advchain_jacobian_det2d_fwd": (_I, [_P, _P, _L, _P, _P]),
    "advchain_jacobian_det2d_bwd": (_I, [_P, _P, _P, _L, _P, _P]),
    "advchain_expo_start": (_I, [_P, _P, _F, _L, _I, _P, _P]),
    "advchain_image_diff3d_fwd": (_I, [_P, _P, _P, _P, _L, _L, _P, _P]),
    "advchain_image_diff3d_bwd": (_I, [_P, _P, _P, _P, _L, _L, _P, _P]),
    "advchain_jacobian_det_fwd": (_I, [_P, _P, _L, _I, _P, _I, _P]),
    "advchain_jacobian_det_bwd": (_I, [_P, _P, _P, _P, _L, _I, _P, _I, _P]),
    "advchain_jacobian_det_workspace": (_L, [_L, _I, _P]),
    "advchain_jacobian_stats_workspace": (_L, [_L, _I, _P]),
    "advchain_jacobian_stats": (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _P, _I, _P]),
    "advchain_sumsq_ordered": (_I, [_P, _L, _P, _P, _P]),
    "advchain_bicubic2d_det_workspace": (_L, [_L, _L, _P]),
    "advchain_grid_sample_bicubic2d_bwd_det": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _P, _P, _I, _P]),
    "advchain_tp_interp_sumsq_partials": (_L, [_P, _L]),
    "advchain_tp_interp_sumsq_ordered": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _P, _P, _P]),
    # (the *_fwd_ord lists: their family's with `partials, stride, counts` in place of `sums`)
    "advchain_consistency_fwd_partials": (_L, [_L, _L, _I, _P, _I, _I, _I]),
    "advchain_consistency_fwd_ord": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P]),
    "advchain_consistency_fused_fwd_partials": (_L, [_L, _L, _I, _P, _I, _I, _I, _I]),
    "advchain_consistency_fused_fwd_ord": (_I, [_P, _P, _P, _P, _P, _L, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P]),
    "advchain_consistency_wide_fwd_partials": (_L, [_L, _L, _I, _P, _I, _I]),
    "advchain_consistency_wide_fwd_ord": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P]),
    "advchain_consistency_lp_fwd_partials": (_L, [_L, _L, _I, _P, _I]),
    "advchain_consistency_lp_fwd_ord": (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _L, _P, _L, _L, _I, _P, _I, _I, _I, _I, _P, _P]),
    "advchain_consistency_finish_ord": (_I, [_P, _L, _P, _P, _P, _P, _P]),
}

class UpdateDesc(ctypes.Structure):
    """advchain_update_desc of include/advchain_hip.h."""
    _fields_ = [("base", c_void_p), ("x", c_void_p), ("out", c_void_p), ("old", c_void_p), ("N", c_int64), ("M", c_int64),
                ("kind", ctypes.c_int32), ("step", c_float)]


_lib = None


class AdvchainHipError(RuntimeError):
    pass


class _Lib(object):
    """Thin proxy over the ctypes library.  ``timed`` (bench / profiling only) wraps selected entry points with
    a pair of events on the current stream -- the stream the kernels are launched on -- and records
    (name, args, start_event, end_event); everything else is a direct ctypes call."""

    def __init__(self, cdll):
        self._cdll = cdll
        self._raw = {}
        self.records = []

    def _bind(self, name, res, args):
        fn = getattr(self._cdll, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
        self._raw[name] = fn
        setattr(self, name, fn)

    def timed(self, names=None, every=1):
        """Event pairs (on the current stream) around the chosen entry points; `every` = k samples one call in k."""
        import contextlib
        import torch

        @contextlib.contextmanager
        def ctx():
            chosen = [n for n in self._raw if (names is None or n in names) and self._raw[n].restype is c_int
                      and len(self._raw[n].argtypes) > 0]
            for n in chosen:
                raw = self._raw[n]

                count = [0]

                def wrapped(*a, _raw=raw, _n=n, _count=count):
                    _count[0] += 1
                    if _count[0] % every:
                        return _raw(*a)
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = _raw(*a)
                    e1.record()
                    self.records.append((_n, a, e0, e1))
                    return rc
                setattr(self, n, wrapped)
            try:
                yield self
            finally:
                for n in chosen:
                    setattr(self, n, self._raw[n])
        return ctx()


def load():
    """Loads the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdvchainHipError(
            "libadvchain_hip.so not found at %s -- build it with `python -m advchain_amd.build` "
            "(there is no CPU / PyTorch fallback for the advchain_amd kernels)" % LIB_PATH)
    # make sure the HIP runtime PyTorch uses is the one already mapped (same SONAME libamdhip64.so.7)
    import torch  # noqa: F401
    tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tl):
        ctypes.CDLL(tl, mode=ctypes.RTLD_GLOBAL)
    lib = _Lib(ctypes.CDLL(LIB_PATH))
    for name, (res, args) in PROTOTYPES.items():
        lib._bind(name, res, args)
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().advchain_last_error()
        raise AdvchainHipError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))


_DIMS = {}


def dims_array(dims):
    key = tuple(dims)
    arr = _DIMS.get(key)
    if arr is None:
        arr = _DIMS[key] = (c_int64 * len(key))(*[int(d) for d in key])   # read-only for the library: safe to share
    return arr


def float_array(vals):
    return (c_float * len(vals))(*[float(v) for v in vals])
