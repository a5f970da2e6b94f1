"""bf16 logits in the consistency loss, as far as a machine without a GPU can check them: the host-side argument checks of
the three C entries of csrc/loss_lp.hip (no launch) and the operator's gate."""
import ctypes

import pytest
import torch


def test_lp_entries_check_their_arguments_on_the_host():
    """Null pointers, K = 0 and 65536, a storage flag of 2, a bad mask channel count, a bad rank: a negative code and a
    message that names the entry; nothing is launched.  An empty batch returns 0."""
    from advchain_amd import _lib
    lib = _lib.load()
    dims = _lib.dims_array((4, 8))
    buf = (ctypes.c_float * 4096)()          # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    last = lib.advchain_last_error

    def fwd(pred=p, ref=p, stats=p, out=p, K=20, pb=1, rb=1, mask=None, mch=1, nd=2, N=1):
        return lib.advchain_consistency_lp_fwd(pred, pb, ref, rb, mask, stats, None, out, N, K, nd, dims, mch, 0, 1, 0, None)

    def bwd(pred=p, ref=p, stats=p, out=p, K=20, pb=1, rb=1, mask=None, mch=1, nd=2, N=1):
        return lib.advchain_consistency_lp_bwd(pred, pb, ref, rb, stats, None, mask, None, out, 1.0, 0.0, 0.0, 0.0, 0, N, K, nd,
                                               dims, mch, None)

    def ref_bwd(pred=p, ref=p, stats=p, out=p, K=20, pb=1, rb=1, mask=None, mch=1, nd=2, N=1):
        return lib.advchain_consistency_lp_ref_bwd(pred, pb, ref, rb, stats, None, mask, None, out, 1.0, 0.0, 0.0, 0.0, 0, N, K,
                                                   nd, dims, mch, None)
    for call, name in ((fwd, b"consistency_lp_fwd"), (bwd, b"consistency_lp_bwd"), (ref_bwd, b"consistency_lp_ref_bwd")):
        for kw in (dict(pred=None), dict(ref=None), dict(stats=None), dict(out=None), dict(K=0), dict(K=65536), dict(pb=2),
                   dict(rb=2), dict(pb=-1), dict(mask=p, mch=3), dict(nd=4), dict(nd=1), dict(N=65536)):
            assert call(**kw) < 0, (name, kw)
            assert name in last(), (name, kw, last())
        for pb in (0, 1):
            for rb in (0, 1):
                assert call(N=0, pb=pb, rb=rb) == 0, (name, pb, rb)       # an empty batch is fine and launches nothing


def test_a_cpu_bf16_tensor_is_refused_for_its_device_not_its_dtype():
    from advchain_amd import _lib
    from advchain_amd.common.loss import calc_segmentation_consistency, kl_divergence
    x = torch.zeros(1, 4, 8, 8, dtype=torch.bfloat16)
    for a, b in ((x, x), (x.float(), x), (x, x.float())):
        with pytest.raises(_lib.AdvchainHipError, match="no CPU path"):
            calc_segmentation_consistency(a, b, ["mse", "contour"], [1.0, 0.5])
        with pytest.raises(_lib.AdvchainHipError, match="no CPU path"):
            kl_divergence(b, a)

