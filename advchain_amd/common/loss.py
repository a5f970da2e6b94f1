"""Segmentation losses (reference: advchain/common/loss.py): the consistency loss (loss.py:8-249) and the supervised
``contour_loss`` / ``One_Hot`` / ``cross_entropy_2D`` (loss.py:102-220, 252-326, on csrc/seg_loss.hip); ``dice_loss`` /
``dice_ce_loss`` / ``cross_entropy_3D`` (not in the reference; csrc/seg_dice.hip) complete the supervised loss of a 2D or 3D step;
``distance_transform_edt`` / ``signed_distance_maps`` / ``boundary_loss`` (not in the reference; csrc/edt.hip, csrc/seg_boundary.hip)
are the exact Euclidean distance maps of masks and label maps on the device and the boundary loss on them;
``soft_skeletonize`` / ``cldice_loss`` (not in the reference; csrc/seg_skeleton.hip) are the soft skeletons and the soft-clDice loss.

'mse', 'contour' and 'kl' all run in the fused HIP kernels (:func:`advchain_amd.ops.consistency_sums`:
softmax + mask + squared error + KL sum + 3^d edge stencils in two launches forward, one backward per operand that
needs a gradient: the prediction and -- csrc/loss_ref.hip -- the reference).

Batch sharding: ``global_batch`` overrides N in every normaliser -- mse ~ 1/(N^2 K V^2),
contour ~ 1/(N V) -- so that the per-shard values SUM to the whole-batch loss and the mse:contour mix
(hence the ascent direction) does not depend on the shard size."""
import math
import warnings

import torch

from .. import ops

MAX_CLASSES = 65535   # the C ABI's range (include/advchain_hip.h): up to 16 classes run csrc/loss.hip, more csrc/loss_lp.hip
                      # (a bf16 operand: csrc/loss_lp.hip for every class count)


def _check_operands(output, reference):
    """The restrictions of the fused kernels, stated where the user meets them (INTEGRATION.md "Known deviations"): fp32
    or bf16 ROCm tensors, each operand on its own (no CPU path and no float16 -- ops raises), fewer than 65536 channels.
    Both operands are differentiated, as by the reference's torch expression; a gradient has its operand's dtype."""
    if output.size(1) > MAX_CLASSES:
        raise NotImplementedError('the consistency kernels take at most %d classes, got %d'
                                  % (MAX_CLASSES, output.size(1)))


def class_weights_tuple(class_weights, K=None):
    """`class_weights` (a list, tuple, ndarray or tensor of K numbers; a device tensor is read to the host, once) as a tuple
    of floats, or None.  ValueError for anything but one finite, non-negative number per class -- raised before any device
    work, so a CPU caller sees the same errors.  K=None leaves the length to a later call."""
    if class_weights is None:
        return None
    if isinstance(class_weights, torch.Tensor):
        class_weights = class_weights.detach().cpu()
    if hasattr(class_weights, 'tolist'):          # tensor, ndarray
        class_weights = class_weights.tolist()
    if not isinstance(class_weights, (list, tuple)) or any(isinstance(w, (list, tuple)) for w in class_weights):
        raise ValueError('class_weights must be a flat sequence with one number per class')
    w = tuple(float(x) for x in class_weights)
    if K is not None and len(w) != K:
        raise ValueError('class_weights has the wrong length: %d entries for %d classes' % (len(w), K))
    for i, x in enumerate(w):
        if math.isnan(x):
            raise ValueError('class_weights[%d] is NaN' % i)
        if math.isinf(x):
            raise ValueError('class_weights[%d] is infinite (%r)' % (i, x))
        if x < 0:
            raise ValueError('class_weights[%d] is negative (%r)' % (i, x))
    return w


def _weighted(class_weights, K):
    """The keyword that hands validated weights to ops.consistency_sums; without weights the call is today's, argument for
    argument."""
    return {} if class_weights is None else {'class_w': class_weights_tuple(class_weights, K)}


def _pooled(x, scale):
    pool = torch.nn.AvgPool2d if x.dim() == 4 else torch.nn.AvgPool3d
    return pool(2 ** scale)(x)


def _single_channel_mask(mask, K):
    """The solver's validity mask has K identical channels (Q12); stencils and MSE only need what the
    kernel reads: 1 channel, or K distinct ones."""
    if mask is None:
        return None
    if mask.shape[1] not in (1, K):
        raise ValueError('mask must have 1 or %d channels' % K)
    if mask.shape[1] == K and K > 1 and mask.stride(1) == 0:
        return mask[:, :1]          # expanded view of a 1-channel mask
    return mask


def calc_segmentation_consistency(output, reference, divergence_types=['kl', 'contour'],
                                  divergence_weights=[1.0, 0.5], class_weights=None, scales=[0],
                                  mask=None, is_gt=False, global_batch=None):
    """Difference between two predictions (logits), same signature as the reference (loss.py:8-87).  `output` and
    `reference` are fp32 or bf16 (a model under autocast), independently: a bf16 operand is read as it is (csrc/loss_lp.hip),
    all arithmetic is fp32 -- the value is the fp32 loss of the upcast operands, an fp32 scalar -- and the gradient of an
    operand has that operand's dtype (computed in fp32, rounded once).  float16 is refused.

    class_weights (the reference documents the parameter and raises): K finite, non-negative numbers w_k -- list, tuple, ndarray
    or tensor -- used as given, without normalisation; constants (no gradient).  With D = P - T' masked,
    'mse' sums w_k (m_k D_k)^2, 'kl' sums w_k m_k T'_k (log T'_k - log P_k), 'contour' multiplies the edge energy of object
    class i by w_i (w_0 does not enter); every normaliser stays as it is, so w = 1 is the unweighted loss.  Weights run the
    run-time-K kernels (the cw entries of csrc/loss_lp.hip) for every K and dtype pair; None runs the unweighted paths."""
    spatial_dims = output.dim() - 2
    assert spatial_dims == 2 or spatial_dims == 3, 'only support 2d or 3d segmentation'
    assert output.dim() == reference.dim(), 'output and reference must have the same rank'
    K = reference.size(1)
    weighted = _weighted(class_weights, K)
    _check_operands(output, reference)
    if any(scale != 0 for scale in scales):
        # a bf16 operand is upcast ONCE, differentiably, in front of the AvgPool: the pool runs in fp32 (the value stays the
        # fp32 loss of the upcast operands), and the gradients of the scales add up in fp32 and are rounded once, by the cast
        output = output.float() if output.dtype == torch.bfloat16 else output
        reference = reference.float() if reference.dtype == torch.bfloat16 else reference
    dist = 0.
    for scale in scales:
        out_s, ref_s = (output, reference) if scale == 0 else (_pooled(output, scale), _pooled(reference, scale))
        N = out_s.shape[0]
        V = 1
        for s in out_s.shape[2:]:
            V *= s
        Ng = N if global_batch is None else int(global_batch)
        w_mse = sum(w for t, w in zip(divergence_types, divergence_weights) if t == 'mse')
        w_cnt = sum(w for t, w in zip(divergence_types, divergence_weights) if t == 'contour')
        for t in divergence_types:
            if t not in ('kl', 'mse', 'contour'):
                raise NotImplementedError
        has_mse = 'mse' in divergence_types
        has_cnt = 'contour' in divergence_types and K > 1
        has_kl = 'kl' in divergence_types
        m = _single_channel_mask(mask if scale == 0 else (None if mask is None else mask), K)
        if has_mse or has_cnt or has_kl:
            # 'mse': MSELoss(mean) over N*K*V elements, divided again by numel(mask)/K (loss.py:62-64, Q13): N*V for the
            # default all-ones / K-channel mask, N*V/K for a caller's 1-channel mask (an expanded view counts as K)
            mask_ch = K if mask is None else mask.shape[1]
            c_mse = (w_mse / (float(Ng) * K * V * (float(Ng) * mask_ch * V / K))) if has_mse else 0.0
            # 'contour': mean over classes 1..K-1 of  2D 0.5*(MSE_x + MSE_y) | 3D 1/3*(2*MSE_A + MSE_B)  (loss.py:74-79,211-219, Q14)
            if has_cnt:
                if spatial_dims == 2:
                    c_a = c_b = w_cnt * 0.5 / (float(Ng) * V * (K - 1))
                else:
                    c_a = w_cnt * (2.0 / 3.0) / (float(Ng) * V * (K - 1))
                    c_b = w_cnt * (1.0 / 3.0) / (float(Ng) * V * (K - 1))
            else:
                c_a = c_b = 0.0
            # 'kl': mean over the N*V voxels of sum_k m_k p_k (log p_k - log q_k)  (loss.py:244-248)
            w_kl = sum(w for t, w in zip(divergence_types, divergence_weights) if t == 'kl')
            c_kl = (w_kl / (float(Ng) * V)) if has_kl else 0.0
            coef = [(2 ** scale) * c for c in (c_mse, c_a, c_b, c_kl)]
            val, _ = ops.consistency_sums(out_s, ref_s, m, coef, ref_is_prob=is_gt, want_edges=has_cnt, **weighted)
            dist = val if isinstance(dist, float) and dist == 0. else dist + val     # (0. + x is x: no launch for it)
    # (x / 1.0 is x: the reference's division by the number of scales is skipped for its only call, scales = [0])
    return dist if len(scales) == 1 else dist / (1.0 * len(scales))


def kl_divergence(reference, pred, mask=None, is_gt=False, global_batch=None, class_weights=None):
    """KL(P||Q) of two logit maps (loss.py:223-249): the 'kl' term of the fused kernels on its own.  fp32 or bf16 operands
    and class_weights (an extension: class k enters w_k times) as in :func:`calc_segmentation_consistency`."""
    K = pred.size(1)
    weighted = _weighted(class_weights, K)
    _check_operands(pred, reference)
    V = 1
    for s in pred.shape[2:]:
        V *= s
    Ng = pred.shape[0] if global_batch is None else int(global_batch)
    val, _ = ops.consistency_sums(pred, reference, _single_channel_mask(mask, K), [0.0, 0.0, 0.0, 1.0 / (float(Ng) * V)],
                                  ref_is_prob=is_gt, want_edges=False, **weighted)
    return val


def calc_segmentation_mse_consistency(input, target):
    return calc_segmentation_consistency(output=input, reference=target, divergence_types=['mse'],
                                         divergence_weights=[1.0], class_weights=None, mask=None)


def calc_segmentation_kl_consistency(input, target):
    return calc_segmentation_consistency(output=input, reference=target, divergence_types=['kl'],
                                         divergence_weights=[1.0], class_weights=None, mask=None)


# ---- supervised losses (reference: advchain/common/loss.py:102-220, 252-271, 274-326) ----------------------------------

def _require_gpu(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ops._lib.AdvchainHipError("%s must be a CUDA/ROCm tensor: the advchain_amd kernels have no CPU path" % name)


def contour_loss(input, target, use_gpu=True, ignore_background=True, one_hot_target=True, mask=None,
                 device=torch.device("cuda")):
    """Contour loss across object boundaries (loss.py:102-220), same signature.  `use_gpu` and `device` are accepted and
    ignored: the kernels run on the input's device.  The reference's filters sum over the class axis, so the
    loss is the Sobel edge energy of u = sum over the object classes of (input_c - target_c), weighted by the mean of m^2 over
    the first min(#object classes, mask channels) mask channels (its mask[:, :object_classes] slice)."""
    _require_gpu(input, "input")
    if input.dim() not in (4, 5):
        raise NotImplementedError("contour_loss supports 2D (N,C,H,W) and 3D (N,C,D,H,W) input, got %d-D" % input.dim())
    K = input.size(1)
    first = 1 if ignore_background else 0
    oc = K - first
    if oc < 1:
        raise ValueError("contour_loss: no object class left (%d classes, ignore_background=%s)" % (K, ignore_background))
    if mask is not None:
        _require_gpu(mask, "mask")
        if input.dim() == 4 and 1 < mask.shape[1] < oc:     # (3D: the reference's conv output has one channel)
            raise ValueError("mask with %d channels does not broadcast against %d object classes" % (mask.shape[1], oc))
        if torch.is_grad_enabled() and mask.requires_grad:
            warnings.warn('advchain_amd: contour_loss treats the mask as a constant (detach it to silence this warning)',
                          stacklevel=2)
    return ops.contour_energy(input, target, mask=mask, first_class=first, one_hot_target=one_hot_target)


class One_Hot(torch.nn.Module):
    """Integer labels (N x dims or N x 1 x dims) -> float32 one-hot maps N x depth x dims (loss.py:252-271).  `use_gpu` and
    `device` are accepted and ignored: the kernel runs on the labels' device.  Out-of-range labels give NaN channels."""

    def __init__(self, depth, use_gpu=True, device=torch.device("cuda")):
        super(One_Hot, self).__init__()
        self.depth = depth

    def forward(self, X_in):
        _require_gpu(X_in, "X_in")
        if X_in.dim() < 2:
            raise IndexError("One_Hot takes labels of shape N x dims, got %s" % (tuple(X_in.shape),))
        lab = X_in.detach()
        lab = lab if lab.dtype == torch.int64 else lab.long()
        out = ops.one_hot(lab.reshape(lab.shape[0], -1), self.depth)
        # the reference's permute(0, -1, 1, ...).squeeze(dim=2): (N, depth, *X.shape[1:]) without a size-1 third axis
        shape = [X_in.shape[0], self.depth] + list(X_in.shape[1:])
        if shape[2] == 1:
            del shape[2]
        return out.view(shape)

    def __repr__(self):
        return self.__class__.__name__ + "({})".format(self.depth)


def cross_entropy_2D(input, target, weight=None, size_average=True):
    """Cross entropy on 2D images (loss.py:274-326), same signature.  input: (N,C,H,W) fp32 or bf16 logits; target: (N,H,W)
    int64 labels (-100 is ignored but still counted in N*H*W) or (N,C,H,W) soft targets; weight: C class weights (tensor, list
    or array), used as weight / sum(weight) * C; size_average divides by N*H*W.  Returns an fp32 scalar."""
    _require_gpu(input, "input")
    if input.dim() != 4:
        raise ValueError("cross_entropy_2D expects 4-D input (N,C,H,W), got %d-D" % input.dim())
    _require_gpu(target, "target")
    return ops.cross_entropy_2d(input, target, weight=weight, size_average=size_average)


def cross_entropy_3D(input, target, weight=None, size_average=True):
    """:func:`cross_entropy_2D` for volumes: input (N,C,D,H,W) fp32 or bf16 logits; target (N,D,H,W) int64 labels (-100 is ignored
    but still counted in N*D*H*W) or (N,C,D,H,W) soft targets.  The same kernels (they only use the plane size)."""
    if isinstance(input, torch.Tensor) and input.dim() != 5:
        raise ValueError("cross_entropy_3D expects 5-D input (N,C,D,H,W), got %d-D" % input.dim())
    _require_gpu(input, "input")
    _require_gpu(target, "target")
    return ops.cross_entropy_3d(input, target, weight=weight, size_average=size_average)


def _dice_arguments(name, input, target, weight, ignore_background, smooth, factors=()):
    """The host-side checks of the Dice losses, before any device work (a CPU caller sees the same ValueErrors)."""
    if not isinstance(input, torch.Tensor) or input.dim() not in (4, 5):
        raise ValueError("%s expects 4-D (N,C,H,W) or 5-D (N,C,D,H,W) logits" % name)
    K = input.size(1)
    if K > MAX_CLASSES:
        raise NotImplementedError("%s takes at most %d classes, got %d" % (name, MAX_CLASSES, K))
    smooth = float(smooth)
    if not math.isfinite(smooth) or smooth < 0:
        raise ValueError("%s: smooth must be finite and >= 0, got %r" % (name, smooth))
    for f in factors:
        if not math.isfinite(float(f)):
            raise ValueError("%s: dice_weight and ce_weight must be finite, got %r" % (name, f))
    if ignore_background and K == 1:
        raise ValueError("%s: no class left (1 class, ignore_background=True)" % name)
    if weight is not None:
        if isinstance(weight, torch.Tensor):
            n = weight.numel()
        elif hasattr(weight, "__len__"):
            n = len(weight)
        else:
            raise ValueError("%s: weight must be a tensor, list or array with one number per class" % name)
        if n != K:
            raise ValueError("%s: weight has the wrong length: %d entries for %d classes" % (name, n, K))
    _require_gpu(input, "input")
    _require_gpu(target, "target")


def dice_loss(input, target, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5):
    """Soft Dice loss of logits (not in the reference; csrc/seg_dice.hip).  input: (N,K,H,W) or (N,K,D,H,W) fp32 or bf16 logits,
    read as they are, the softmax over K runs inside the kernel (float16 is refused); target: (N,dims) int64 labels or a
    (N,K,dims) fp32 soft target.  With p = softmax(input), t the one-hot labels or the soft target, and sums over the counted
    voxels of batch entry n (batch_dice: over the whole batch, N -> 1)

        I_nk = sum p_k t_k,  P_nk = sum p_k,  T_nk = sum t_k,  dice_nk = (2 I_nk + smooth) / (P_nk + T_nk + smooth)
        loss = 1 - (1/N) sum_n sum_k omega_k dice_nk,   omega_k = w_k / sum of the counted w_j

    A voxel labelled -100 is left out of every sum (its gradient is zero); any other label outside [0, K) makes the value
    NaN.  weight: K numbers (tensor, list or array; constants), normalised on the device over the counted classes -- class 0
    is not counted with ignore_background.  smooth == 0 with a class that is empty on both sides (no probability mass counted
    and no target) gives NaN.  Returns an fp32 scalar, bitwise reproducible; gradients for the logits (their dtype, computed in
    fp32 and rounded once) and for a soft target (fp32); labels get none."""
    _dice_arguments("dice_loss", input, target, weight, ignore_background, smooth)
    return ops.dice_loss(input, target, weight=weight, ignore_background=ignore_background, batch_dice=batch_dice,
                         smooth=smooth, dice_weight=1.0, ce_weight=0.0)


def dice_ce_loss(input, target, weight=None, ignore_background=False, batch_dice=False, smooth=1e-5, dice_weight=1.0,
                 ce_weight=1.0):
    """ce_weight * CE + dice_weight * :func:`dice_loss` in one pass over the logits (the nnU-Net / MONAI default loss).  CE
    is what ``cross_entropy_2D(input, target, weight, size_average=True)`` computes, for 2D and 3D input: the weights enter it
    as weight / sum(weight) * K, a voxel labelled -100 contributes 0 but is counted in N * voxels, and ignore_background
    does not touch it.  Everything else as in :func:`dice_loss`."""
    _dice_arguments("dice_ce_loss", input, target, weight, ignore_background, smooth, (dice_weight, ce_weight))
    return ops.dice_loss(input, target, weight=weight, ignore_background=ignore_background, batch_dice=batch_dice,
                         smooth=smooth, dice_weight=dice_weight, ce_weight=ce_weight)


# ---- soft skeletons and the soft-clDice loss (not in the reference; csrc/seg_skeleton.hip) ---------------------------------------

def _check_iterations(name, iterations):
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= ops.SKELETON_MAX_ITERATIONS:
        raise ValueError("%s: iterations must be an int in [0, %d], got %r" % (name, ops.SKELETON_MAX_ITERATIONS, iterations))


def soft_skeletonize(maps, iterations=3):
    """Soft skeleton of probability maps (Shit et al., clDice, CVPR 2021; csrc/seg_skeleton.hip).  maps: (N,C,H,W) or
    (N,C,D,H,W) fp32; every plane is skeletonised on its own; returns fp32 of the same shape.  With E the minimum over a voxel
    and its in-image face neighbours, D the maximum over the in-image 3x3(x3) box (a position outside the image is nothing):

        skel = relu(x - D(E(x)));  iterations times:  x <- E(x),  delta = relu(x - D(E(x))),  skel <- skel + relu(delta - skel delta)

    each operation rounded once in fp32: bit for bit the published max_pool composition.  iterations: an int in [0, 32].
    Differentiable with respect to maps: the gradient of this composition with relu'(0) = 0 and, among equal window values, the
    first winning (E: centre, then axis by axis, minus before plus; D: centre, then raster order) -- on hard masks this
    differs from torch's tie rules (INTEGRATION.md "Known deviations").  Bitwise reproducible."""
    if not isinstance(maps, torch.Tensor) or maps.dim() not in (4, 5):
        raise ValueError("soft_skeletonize expects 4-D (N,C,H,W) or 5-D (N,C,D,H,W) maps")
    _check_iterations("soft_skeletonize", iterations)
    if maps.dtype != torch.float32:
        raise ValueError("soft_skeletonize: maps must be float32, got %s" % maps.dtype)
    if maps.size(1) > MAX_CLASSES:
        raise NotImplementedError("soft_skeletonize takes at most %d channels, got %d" % (MAX_CLASSES, maps.size(1)))
    _require_gpu(maps, "maps")
    return ops.soft_skeletonize(maps, iterations=iterations)


def cldice_loss(input, target, iterations=3, weight=None, ignore_background=True, batch=False, smooth=1.0):
    """soft-clDice loss of logits (Shit et al., CVPR 2021; csrc/seg_skeleton.hip): the centerline Dice of the soft skeletons
    (:func:`soft_skeletonize`) of prediction and target.  input: (N,K,H,W) or (N,K,D,H,W) fp32 or bf16 logits, read as they are,
    the softmax over K runs inside the kernels (float16 is refused); target: (N,dims) int64 labels or a (N,K,dims) fp32 soft
    target, a constant (one that requires a gradient is refused).  With p = softmax(input), t the one-hot labels (a label
    outside [0, K), -100 included, is in no class) or the soft target, m = 0 where the label is -100 and 1 elsewhere (m masks the
    summands only: those voxels still take part in the neighbourhoods), S^p = skel(p), S^t = skel(t) per plane, and sums over
    the voxels of batch entry n (batch: over the whole batch, N -> 1)

        Tprec_nk = (sum m S^p_k t_k + smooth) / (sum m S^p_k + smooth),  Tsens_nk = (sum m S^t_k p_k + smooth) / (sum m S^t_k + smooth)
        loss = 1 - (1/rows) sum_nk omega_k 2 Tprec_nk Tsens_nk / (Tprec_nk + Tsens_nk),   omega_k = w_k / sum of the counted w_j

    Class 0 is not counted with ignore_background.  With K = 2, ignore_background=True, batch=True and smooth=1 this is the
    published ``soft_cldice`` exactly.  smooth == 0 with an empty skeleton gives NaN.  iterations: an int in [0, 32].  Returns an
    fp32 scalar, bitwise reproducible; the gradient has the logits' dtype (computed in fp32, rounded once) and follows the tie
    rule of :func:`soft_skeletonize`.  Combine with Dice as ``(1 - a) * dice_loss(x, y) + a * cldice_loss(x, y)``."""
    _check_iterations("cldice_loss", iterations)
    if isinstance(input, torch.Tensor) and input.dtype == torch.float16:
        raise ValueError("cldice_loss: logits must be float32 or bfloat16, got torch.float16")
    if isinstance(target, torch.Tensor) and target.is_floating_point() and target.requires_grad and torch.is_grad_enabled():
        raise ValueError("cldice_loss: the target is a constant and gets no gradient (detach it)")
    if isinstance(input, torch.Tensor) and isinstance(target, torch.Tensor) and input.dim() in (4, 5):
        if target.dim() == input.dim() - 1:
            want = (input.shape[0],) + tuple(input.shape[2:])
            if tuple(target.shape) != want:
                raise ValueError("cldice_loss: label target must be %s, got %s" % (want, tuple(target.shape)))
        elif target.dim() == input.dim():
            if target.shape != input.shape:
                raise ValueError("cldice_loss: soft target must have the input's shape %s, got %s"
                                 % (tuple(input.shape), tuple(target.shape)))
        else:
            raise NotImplementedError("cldice_loss: target must be (N,dims) labels or (N,C,dims) soft targets")
    _dice_arguments("cldice_loss", input, target, weight, ignore_background, smooth)
    return ops.cldice_loss(input, target, iterations=iterations, weight=weight, ignore_background=bool(ignore_background),
                           batch=bool(batch), smooth=float(smooth))


# ---- Euclidean distance maps and the boundary loss (not in the reference; csrc/edt.hip, csrc/seg_boundary.hip) -------------------

def _check_sampling(name, sampling, ndim):
    if sampling is None:
        return None
    try:
        vals = [float(s) for s in sampling]
    except TypeError:
        raise ValueError("%s: sampling must be None or one number per spatial axis" % name)
    if len(vals) != ndim:
        raise ValueError("%s: sampling has the wrong length: %d numbers for %d spatial axes" % (name, len(vals), ndim))
    for s in vals:
        if not math.isfinite(s) or s <= 0:
            raise ValueError("%s: sampling must be positive and finite, got %r" % (name, s))
    return tuple(vals)


def distance_transform_edt(mask, sampling=None, squared=False):
    """Exact Euclidean distance transform on the device (csrc/edt.hip), scipy.ndimage.distance_transform_edt's definition.
    mask: (B,H,W) or (B,D,H,W), bool, uint8, int64 or fp32, nonzero is foreground; every leading entry is transformed on its
    own.  Returns fp32 of the same shape: at a foreground voxel the distance to the nearest zero voxel of the same entry, 0 at a
    zero voxel, and +inf at the foreground voxels of an entry that has no zero voxel.  sampling: None (unit spacing) or one
    positive finite number per spatial axis, in axis order (D,) H, W.  squared=True returns the squared distance (with unit
    spacing an exact integer).  With unit spacing the arithmetic is int32 and the result the same bits on every run."""
    if not isinstance(mask, torch.Tensor) or mask.dim() not in (3, 4):
        raise ValueError("distance_transform_edt expects a 3-D (B,H,W) or 4-D (B,D,H,W) mask")
    sampling = _check_sampling("distance_transform_edt", sampling, mask.dim() - 1)
    _require_gpu(mask, "mask")
    return ops.distance_transform_edt(mask, sampling=sampling, squared=bool(squared))


def _check_num_classes(name, K):
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError("%s: num_classes must be a positive integer, got %r" % (name, K))
    if K > MAX_CLASSES:
        raise NotImplementedError("%s takes at most %d classes, got %d" % (name, MAX_CLASSES, K))


def signed_distance_maps(target, num_classes, sampling=None):
    """Signed Euclidean distance maps of a label map, straight from the labels (no one-hot tensor; csrc/edt.hip).  target:
    (N,H,W) or (N,D,H,W) int64 labels.  Returns (N,num_classes,dims) fp32 with

        phi_nk(v) = d(v, F_nk) - d(v, B_nk),   F_nk = {u : target[n,u] == k},  B_nk its complement in entry n

    positive outside the class, negative inside, at least one spacing in magnitude (the symmetric convention: Kervadec's
    one_hot2dist shifts the inside by one voxel).  A label outside [0, num_classes), -100 included, belongs to no class.  A class
    that is absent from entry n, or fills it, has no boundary: its plane is 0.  The maps are a constant (no gradient)."""
    if not isinstance(target, torch.Tensor) or target.dim() not in (3, 4):
        raise ValueError("signed_distance_maps expects 3-D (N,H,W) or 4-D (N,D,H,W) labels")
    _check_num_classes("signed_distance_maps", num_classes)
    sampling = _check_sampling("signed_distance_maps", sampling, target.dim() - 1)
    _require_gpu(target, "target")
    return ops.signed_distance_maps(target, num_classes, sampling=sampling)


def boundary_loss(input, target=None, weight=None, ignore_background=True, sampling=None, dist_maps=None):
    """Boundary (surface) loss of Kervadec et al. (csrc/seg_boundary.hip).  input: (N,K,H,W) or (N,K,D,H,W) fp32 or bf16 logits,
    read as they are, the softmax over K runs inside the kernel (float16 is refused).  Exactly one of target ((N,dims) int64
    labels: their :func:`signed_distance_maps` with `sampling` are computed on the device) and dist_maps ((N,K,dims) fp32, e.g.
    from :func:`signed_distance_maps`, computed once and reused; a constant) supplies the maps phi:

        loss = 1/(N V) sum_n sum_{v counted} sum_{k counted} omega_k p_k(v) phi_nk(v),   omega_k = w_k / sum of the counted w_j

    Class 0 is not counted with ignore_background (the default, as in the paper).  With target, a voxel labelled -100 is not
    counted (zero gradient) but stays in N V; any other label outside [0, K) makes the value and the gradient NaN.  With dist_maps
    every voxel is counted.  weight: K numbers (tensor, list or array; constants), normalised on the device over the counted
    classes.  Returns an fp32 scalar, bitwise reproducible; the gradient has the logits' dtype (computed in fp32, rounded once)."""
    if not isinstance(input, torch.Tensor) or input.dim() not in (4, 5):
        raise ValueError("boundary_loss expects 4-D (N,C,H,W) or 5-D (N,C,D,H,W) logits")
    K = input.size(1)
    if K > MAX_CLASSES:
        raise NotImplementedError("boundary_loss takes at most %d classes, got %d" % (MAX_CLASSES, K))
    sampling = _check_sampling("boundary_loss", sampling, input.dim() - 2)
    if weight is not None:
        if isinstance(weight, torch.Tensor):
            n = weight.numel()
        elif hasattr(weight, "__len__"):
            n = len(weight)
        else:
            raise ValueError("boundary_loss: weight must be a tensor, list or array with one number per class")
        if n != K:
            raise ValueError("boundary_loss: weight has the wrong length: %d entries for %d classes" % (n, K))
    if ignore_background and K == 1:
        raise ValueError("boundary_loss: no class left (1 class, ignore_background=True)")
    if (target is None) == (dist_maps is None):
        raise ValueError("boundary_loss: exactly one of target and dist_maps supplies the distance maps")
    if target is not None:
        if not isinstance(target, torch.Tensor) or tuple(target.shape) != (input.shape[0],) + tuple(input.shape[2:]):
            raise ValueError("boundary_loss: target must be labels of shape %s" % ((input.shape[0],) + tuple(input.shape[2:]),))
    else:
        if not isinstance(dist_maps, torch.Tensor) or dist_maps.shape != input.shape:
            raise ValueError("boundary_loss: dist_maps must have the input's shape %s" % (tuple(input.shape),))
        if sampling is not None:
            raise ValueError("boundary_loss: sampling belongs to the maps; it has no meaning with dist_maps")
        if torch.is_grad_enabled() and dist_maps.requires_grad:
            warnings.warn('advchain_amd: boundary_loss treats dist_maps as a constant (detach it to silence this warning)',
                          stacklevel=2)
    _require_gpu(input, "input")
    _require_gpu(target if target is not None else dist_maps, "target" if target is not None else "dist_maps")
    return ops.boundary_loss(input, target=target, weight=weight, ignore_background=bool(ignore_background), sampling=sampling,
                             dist_maps=dist_maps)
