"""Validation metrics of label maps on the device (not in the reference; csrc/seg_surface.hip on the distance fields of csrc/edt.hip):
``surface_distance_metrics`` / ``hausdorff_distance`` / ``average_surface_distance`` / ``surface_dice``, and (csrc/seg_components.hip)
the instance-wise ``instance_metrics``; its definitions follow those of the voxel-wise metrics below.

Definitions.  pred and target are int64 label maps (N, dims), dims = (H, W) or (D, H, W), K = num_classes.  For entry n and class
k: A = {v : pred[n,v] == k} and B = {v : target[n,v] == k}.  A label outside [0, K), -100 included, belongs to no class (the rule
of signed_distance_maps).  Labels are only compared with class indices; they are never used as an address.

Border.  The border dS of a set S is the voxels of S that have a face neighbour (4 in 2D, 6 in 3D) outside S.  A position outside
the image counts as outside S.  This is S ^ scipy.ndimage.binary_erosion(S) with scipy's defaults, i.e. MONAI's get_mask_edges.
A voxel has one label per map, so "border of its own class" is one predicate per voxel and map: v is a border voxel of class
pred[v] iff some face neighbour is outside the image or carries another label.

Directed distances.  d(a, dB) = min over b in dB of |S (a - b)|, with S = diag(sampling) in axis order (unit spacing when sampling
is None).  Direction 0 is the multiset {d(a, dB) : a in dA}, of size m0 = |dA|; direction 1 is {d(b, dA) : b in dB}, of size
m1 = |dB|.

Per direction: max, mean, percentile.  Let x_(0) <= ... <= x_(m-1) be the sorted distances.  For the percentile q in [0, 100]:
h = (m - 1) * (q / 100) in float64, j = floor(h), g = h - j, and P_q = x_(j) + g * (x_(min(j+1, m-1)) - x_(j)), evaluated in
float64.  This is numpy.percentile's default "linear" rule.

Symmetric values.  hausdorff = max(max0, max1).  hausdorff_percentile = max(P_q of direction 0, P_q of direction 1): MONAI's
definition, not the percentile of the pooled distances.  assd = (sum0 + sum1) / (m0 + m1).

Empty borders.  If both dA and dB are empty (the class is in neither map of the entry), every distance of (n, k) is NaN.  If exactly
one is empty, every distance of (n, k) is +inf.  The counts say which case it is.

Overlap, from the same pass over the labels: the int64 counts |A|, |B|, |A n B|, and dice = 2 |A n B| / (|A| + |B|), NaN when both
are empty.

With unit spacing the squared distances are exact int32, roots, interpolation and means are taken in float64 and rounded to fp32
once; every value is the same bits on every run, nothing is read back to the host, and the call can be captured in a graph.  There
is no gradient: the inputs are detached.

Instance-wise detection (``instance_metrics``).  The metrics above score a class as one set of voxels; lesion, nodule, metastasis
and cell tasks count objects instead (Metrics Reloaded, BraTS-METS, panoptic segmentation): how many were found, missed or
invented, and how well the found ones were segmented.

Components.  ``connectivity``, ``background``, foreground and component are exactly those of
common.postprocess.connected_components(..., num_classes=K): a label outside [0, K), -100 included, or equal to ``background`` is
in no component.  The class of a component is the label of its voxels.

Per entry and class.  For entry n and class k, P is the set of components of class k in pred[n], T the same in target[n],
nP = |P| and nT = |T|.  For a in P and b in T: I = |a n b| and U = |a| + |b| - I.  The pair overlaps when I >= 1.  Components of
different classes never form a pair.

Match rule.  A pair matches when IoU > iou_threshold, evaluated as (double)I > iou_threshold * (double)U: one fp64 product, one
comparison.  iou_threshold is a finite number with 0.5 <= iou_threshold < 1 (Kirillov et al., Panoptic Segmentation; Metrics
Reloaded's "Mask IoU > 0.5").  With the strict inequality and a threshold of at least 0.5 a component matches at most one
partner: I > U / 2 >= |a| / 2, and the components of target are disjoint.  So the matches are a matching, no assignment problem
arises, and TP is well defined.  IoU == 0.5 exactly does not match at the default.  Thresholds below 0.5 need an assignment step
and are refused with a ValueError.

Quantities.  TP is the number of matches, FP = nP - TP and FN = nT - TP.  iou_fixed is the sum over the matches of
floor(2^32 I / U), taken as the integer division (I << 32) / U in unsigned 64-bit: an exact integer that does not depend on any
order, below 2^63 (I < 2^31, fewer than 2^31 components).

Quotients.  Every quotient is taken in float64 from these integers and rounded to fp32 once.  With S = (double)iou_fixed * 2^-32:

    precision  TP / nP             NaN when nP == 0
    recall     TP / nT             NaN when nT == 0
    f1         2 TP / (nP + nT)    NaN when nP + nT == 0     (the recognition quality RQ)
    sq         S / TP              NaN when TP == 0          (the segmentation quality: the mean IoU of the matches)
    pq         2 S / (nP + nT)     NaN when nP + nT == 0     (the panoptic quality, sq * f1)

The class equal to ``background`` has no components, so its row is all zeros and NaN.

Topology (``betti_numbers``, ``betti_error``).  None of the above sees whether a prediction has the right shape: a myocardium
ring that is broken, a vessel with a spurious handle, a false cavity in a hollow organ.  The Betti error of the clDice and
topology-preserving-loss literature does: |b_i(pred) - b_i(target)| per class for the Betti numbers b0 (components), b1 (loops;
holes in 2D) and b2 (cavities).

Sets.  labels is one int64 label map (N, dims).  For entry n and class k, A = {v : labels[n,v] == k}, for every k in [0, K),
class 0 included: there is no ``background`` argument.  A label outside [0, K), -100 included, is in no class and in the
complement of every class; labels are only compared after the range check.  Positions outside the image are in no class.

Adjacency pair.  ``connectivity`` = c is the adjacency of A, in the sense of common.postprocess.connected_components; the
complement of A gets the dual adjacency.  2D: c = 1 means 4-adjacency for A and 8 for the complement, c = 2 means 8 and 4.  3D:
c = 1 means 6 and 26, c = 3 means 26 and 6; c = 2 (18-adjacency) has no such dual in 3D and is refused with a ValueError.  The
default is 1, as everywhere in the package; thin structures (vessels, one voxel wide and running diagonally) want c = ndim.

Euler characteristic chi.  Let p run over the lattice corners [0..D] x [0..H] x [0..W] ([0..H] x [0..W] in 2D).  The window of p is
the voxels p - {0,1}^ndim; the one with coordinate p_a is "high on axis a", the one with p_a - 1 "low".  With [.] = 1 if true:

    c = ndim (voxels are closed cubes)    chi = sum_p sum_{S subset of the axes} (-1)^|S| [some voxel of the window that is high on
                                          every axis of S is in A]: S empty is the vertex at p, |S| = 1 an edge leaving p, |S| = 2
                                          a face, S all axes the voxel p itself
    c = 1 (the dual complex)              chi = sum_p sum_S (-1)^|S| [every voxel p - sum_{a in T} e_a, T subset of S, is in A]:
                                          voxels - face pairs + 2 x 2 squares - 2 x 2 x 2 blocks

Betti numbers.  b0 is the number of components of A under c.  cav is the number of components of the complement of A, under the
dual adjacency, that contain no voxel with a coordinate 0 or size - 1 on any axis.  2D: b1 = b0 - chi and b2 = 0.  3D: b2 = cav
and b1 = b0 + b2 - chi.  This is Euler-Poincare for the adjacency pairs above (Kong and Rosenfeld).  An empty class has
(0, 0, 0) and chi = 0.  betti_error[n,k,i] = |b_i(pred) - b_i(target)|; there are no NaNs, everything is an integer.

Cost.  One labelling of all classes and one streaming pass over the windows per map; in 3D one more labelling per class for the
cavities, 1 + K labellings per map in all (2D needs none: b1 follows from chi).  The workspace is that of one labelling whatever K
is.  Every value is the same bits on every run; integer atomics only, nothing is read back to the host, and the call can be
captured in a graph.  There is no gradient: the inputs are detached.

Confusion matrix and voxel overlap (``confusion_matrix``, ``overlap_metrics``, ``overlap_scores``; csrc/seg_confusion.hip).  The
first numbers of any report: which class is taken for which, and per class Dice, IoU, precision, recall and specificity.

Inputs.  target is an int64 label map (N, dims).  pred is either an int64 label map of the same shape or fp32 / bf16 logits (or
probabilities) (N, K, dims); the prediction is then the argmax over the class axis, taken inside the kernel with the rule of
torch.argmax on the CPU: the first maximal class wins, a NaN is larger than everything (the first NaN wins), a row of -inf gives
class 0.  bf16 values are widened to fp32, which is exact, so they are compared exactly.

Sets.  A_k = {v : pred[v] == k} and B_k = {v : target[v] == k} for every k in [0, K), class 0 included.  A label outside [0, K) is
in no class and is never used as an address.  ``ignore_index`` is None or an int: a voxel whose TARGET equals it is left out of
every count (the "void" label, usually -100); a prediction equal to it means nothing.  With None nothing is left out, and a
target of -100 is a counted voxel of no class: the counts are then exactly those of surface_distance_metrics(...).overlap.

Counts.  matrix[n,t,p] = #{counted v : target = t, pred = p}: rows are the truth, columns the prediction (sklearn's convention).
pred_only[n,k] = #{counted v : pred = k, target outside [0, K)}, target_only[n,k] = #{counted v : target = k, pred outside
[0, K)}, counted[n] = the voxels not left out.  |A_k| = column sum + pred_only[k], |B_k| = row sum + target_only[k], |A_k n B_k|
is the diagonal.  A voxel outside [0, K) in both maps is counted and is in no other number.  With reduce_batch=True the leading N
is dropped and every entry adds into the same counters.

Quotients.  TP = |A n B|, FP = |A| - TP, FN = |B| - TP, TN = counted - TP - FP - FN.  Each quotient is taken in float64 from these
integers and rounded to fp32 once:

    dice         2 TP / (|A| + |B|)       NaN when |A| + |B| == 0
    iou          TP / (|A| + |B| - TP)    NaN when |A| + |B| == 0
    precision    TP / |A|                 NaN when |A| == 0
    recall       TP / |B|                 NaN when |B| == 0      (the sensitivity)
    specificity  TN / (TN + FP)           NaN when TN + FP == 0  (every counted voxel is in B)

Averages over classes or cases (macro, micro, per-case means) are one line of torch on these tensors.  One streaming pass over the
inputs; integer atomics only, every value is the same bits on every run and for every alignment of the storage, nothing is read
back to the host, and the calls can be captured in a graph.  There is no gradient: the inputs are detached."""
import math

import torch

from .. import ops
from ..ops import Betti, BettiError, Confusion, InstanceMetrics, OverlapMetrics, OverlapScores, SurfaceDice, SurfaceMetrics  # noqa: F401
from .loss import _check_num_classes, _check_sampling, _require_gpu
from .postprocess import _check_labels


def _check_maps(name, pred, target, num_classes, sampling):
    for t, what in ((pred, "pred"), (target, "target")):
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4):
            raise ValueError("%s expects 3-D (N,H,W) or 4-D (N,D,H,W) labels as %s" % (name, what))
    if pred.shape != target.shape:
        raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(pred.shape), tuple(target.shape)))
    if pred.numel() == 0:
        raise ValueError("%s: empty label maps %s" % (name, tuple(pred.shape)))
    _check_num_classes(name, num_classes)
    return _check_sampling(name, sampling, pred.dim() - 1)


def _check_percentile(name, q):
    if isinstance(q, bool) or not isinstance(q, (int, float)) or not math.isfinite(q) or q < 0 or q > 100:
        raise ValueError("%s: percentile must be a finite number in [0, 100], got %r" % (name, q))
    return float(q)


def surface_distance_metrics(pred, target, num_classes, sampling=None, percentile=95.0):
    """Surface distance metrics of every class of a pair of label maps in one call (definitions: the module's docstring).
    Returns SurfaceMetrics, a namedtuple of device tensors:

        hausdorff             (N,K)      fp32   symmetric maximum
        hausdorff_percentile  (N,K)      fp32   symmetric percentile
        assd                  (N,K)      fp32   average symmetric surface distance
        directed              (N,K,2,3)  fp32   direction x (max, percentile, mean)
        surface_voxels        (N,K,2)    int64  m0, m1
        max_squared           (N,K,2)    fp64   largest squared distance per direction; an exact integer with unit spacing;
                                                NaN / inf as the distances
        overlap               (N,K,3)    int64  |A|, |B|, |A n B|
        dice                  (N,K)      fp32   Dice overlap

    sampling: None or one positive finite number per spatial axis; percentile: a number in [0, 100]."""
    sampling = _check_maps("surface_distance_metrics", pred, target, num_classes, sampling)
    percentile = _check_percentile("surface_distance_metrics", percentile)
    _require_gpu(pred, "pred")
    _require_gpu(target, "target")
    return ops.surface_distance_metrics(pred, target, num_classes, sampling=sampling, percentile=percentile)


def hausdorff_distance(pred, target, num_classes, sampling=None, percentile=None):
    """(N,K) fp32: `hausdorff` of :func:`surface_distance_metrics`, or `hausdorff_percentile` when a percentile is given."""
    sampling = _check_maps("hausdorff_distance", pred, target, num_classes, sampling)
    q = 95.0 if percentile is None else _check_percentile("hausdorff_distance", percentile)
    _require_gpu(pred, "pred")
    _require_gpu(target, "target")
    m = ops.surface_distance_metrics(pred, target, num_classes, sampling=sampling, percentile=q)
    return m.hausdorff if percentile is None else m.hausdorff_percentile


def average_surface_distance(pred, target, num_classes, sampling=None, symmetric=True):
    """(N,K) fp32: `assd` of :func:`surface_distance_metrics`, or with symmetric=False the mean of direction 0 (from pred's
    border to target's)."""
    sampling = _check_maps("average_surface_distance", pred, target, num_classes, sampling)
    _require_gpu(pred, "pred")
    _require_gpu(target, "target")
    m = ops.surface_distance_metrics(pred, target, num_classes, sampling=sampling)
    return m.assd if symmetric else m.directed[:, :, 0, 2]


def surface_dice(pred, target, num_classes, tolerance, sampling=None):
    """Normalised surface Dice at a tolerance (NSD) of every class of a pair of label maps: the share of border voxels that lie
    within `tolerance` of the other map's border.  A, B, the border dS, the two directions and `sampling` are those of the module's
    docstring.  This is the voxel-count definition of MONAI's compute_surface_dice (Medical Segmentation Decathlon, Metrics
    Reloaded), not DeepMind's surface-area-weighted one.  Returns SurfaceDice, a namedtuple of device tensors:

        surface_dice    (N,K)    fp32   (c0 + c1) / (m0 + m1), taken in float64 and rounded to fp32 once
        within          (N,K,2)  int64  c0 = #{a in dA : d(a, dB) <= tau_k},  c1 = #{b in dB : d(b, dA) <= tau_k}
        surface_voxels  (N,K,2)  int64  m0, m1: the integers surface_distance_metrics returns

    tolerance: one finite number >= 0, or num_classes of them (list, tuple or 1-D tensor; MONAI's class_thresholds), in the units
    of `sampling`.  Empty borders: NaN when m0 + m1 == 0; when exactly one border is empty every distance is +inf, nothing is
    within, and the value is 0 (MONAI's convention).

    The comparison follows the ball rule of common.postprocess.erosion / dilation, so the two agree.  With unit spacing it is
    on exact integers: d^2 <= T_k with T_k = min(floor(tau_k * tau_k), 2^30 - 1), taken in float64 on the host.  tolerance=2
    includes the squared length 4; math.sqrt(3) gives T = 2 (its square is 2.9999999999999996 in float64): pass a hair more than
    a root that is meant to be included.  With a sampling the squared distance is the fp32 value the distance transform
    produces, ((s_x dx)^2 + (s_y dy)^2) + (s_z dz)^2 evaluated in fp32 in that order, compared with tau_k^2 rounded to fp32 once:
    a tolerance equal to a multiple of the spacing (0.7 at a spacing of 0.7, or 1.4) can fall on either side of the comparison.
    Give such a tolerance a hair above the multiple (1.4001).

    Every value is the same bits on every run and on both routes of the kernel (a search inside the ball for small
    tolerances, the distance fields for large ones); integer atomics only, nothing is read back to the host, and the call can
    be captured in a graph after the first use of a tolerance vector (its K words are copied to the device once and cached).
    The cache keeps the 64 vectors per process that were used last: a graph captured outside a frozen plan holds no reference
    of its own to the vector it read, so a program that replays such a graph while it goes through more than 64 other tolerance
    vectors must keep the graph's vector in use (call once with it eagerly) or capture under a plan.
    There is no gradient: the inputs are detached."""
    sampling = _check_maps("surface_dice", pred, target, num_classes, sampling)
    tolerance = ops.surface_dice_tolerances("surface_dice", tolerance, num_classes)
    _require_gpu(pred, "pred")
    _require_gpu(target, "target")
    return ops.surface_dice(pred, target, num_classes, tolerance, sampling=sampling)


def instance_metrics(pred, target, num_classes, iou_threshold=0.5, connectivity=1, background=0, return_maps=False):
    """Instance-wise detection metrics of every class of a pair of label maps: the connected components of both maps are matched
    per class at IoU > ``iou_threshold`` (definitions: the module's docstring).  Returns InstanceMetrics, a namedtuple of device
    tensors:

        components     (N,K,2)   int64   nP, nT
        matched        (N,K)     int64   TP; FP = nP - TP, FN = nT - TP
        overlapping    (N,K,2)   int64   components of P that overlap at least one component of T, and of T that overlap at least
                                         one of P (the "any overlap" detection count of lesion-wise reports)
        iou_fixed      (N,K)     int64   the sum over the matches of floor(2^32 I / U)
        precision, recall, f1, sq, pq    (N,K) fp32 each
        pred_status, target_status       (N,dims) uint8 with return_maps=True, else None: 0 for a voxel in no component, 1 when
                                         its component is matched, 2 when it is unmatched but overlaps a component of its class
                                         in the other map, 3 when it overlaps none

    iou_threshold: a finite number in [0.5, 1); num_classes at most 65535.  This is neither BraTS's lesion-wise Dice (which
    dilates and merges lesions first) nor a Hungarian assignment (which thresholds below 0.5 would need).

    The components are those of common.postprocess.connected_components; the overlaps of all pairs are counted on the device
    in a hash table per entry that cannot overflow.  Every value is the same bits on every run; integer atomics only, nothing
    is read back to the host, and the call can be captured in a graph.  There is no gradient: the inputs are detached."""
    _check_maps("instance_metrics", pred, target, num_classes, None)
    _check_labels("instance_metrics", pred, connectivity, background)
    if isinstance(iou_threshold, bool) or not isinstance(iou_threshold, (int, float)) or not math.isfinite(iou_threshold) \
            or iou_threshold < 0.5 or iou_threshold >= 1:
        raise ValueError("instance_metrics: iou_threshold must be a finite number in [0.5, 1) (a lower one needs an assignment "
                         "step), got %r" % (iou_threshold,))
    _require_gpu(pred, "pred")
    _require_gpu(target, "target")
    return ops.instance_metrics(pred, target, num_classes, iou_threshold=float(iou_threshold), connectivity=connectivity,
                                background=background, return_maps=bool(return_maps))


def _check_topology(name, maps, num_classes, connectivity):
    for t, what in maps:
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4):
            raise ValueError("%s expects 3-D (N,H,W) or 4-D (N,D,H,W) labels as %s" % (name, what))
    first = maps[0][0]
    if len(maps) == 2 and first.shape != maps[1][0].shape:
        raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(first.shape), tuple(maps[1][0].shape)))
    if first.numel() == 0:
        raise ValueError("%s: empty label map %s" % (name, tuple(first.shape)))
    _check_num_classes(name, num_classes)
    nd = first.dim() - 1
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity < 1 or connectivity > nd:
        raise ValueError("%s: connectivity must be an integer in 1..%d for %d spatial axes, got %r" % (name, nd, nd, connectivity))
    if nd == 3 and connectivity == 2:
        raise ValueError("%s: connectivity 2 (18-adjacency) has no dual adjacency for the complement in 3D; use 1 (6 and 26) or 3 "
                         "(26 and 6)" % name)
    for t, what in maps:
        _require_gpu(t, what)


def betti_numbers(labels, num_classes, connectivity=1):
    """Betti numbers and Euler characteristic of every class of a label map (definitions: "Topology" in the module's docstring).
    Returns Betti, a namedtuple of device tensors:

        betti  (N,K,3)  int64   b0 (components), b1 (loops; holes in 2D), b2 (cavities; 0 in 2D)
        euler  (N,K)    int64   chi

    Every k in [0, num_classes) is a class, 0 included.  connectivity: 1 or ndim (2 is refused in 3D)."""
    _check_topology("betti_numbers", [(labels, "labels")], num_classes, connectivity)
    return ops.betti_numbers(labels, num_classes, connectivity=connectivity)


def betti_error(pred, target, num_classes, connectivity=1):
    """Betti error of every class of a pair of label maps (definitions: "Topology" in the module's docstring).  Returns
    BettiError, a namedtuple of device tensors:

        error  (N,K,3)    int64   |b_i(pred) - b_i(target)|, i = 0, 1, 2
        total  (N,K)      int64   the sum of error over i
        betti  (N,K,2,3)  int64   the Betti numbers of both maps; index 0 of the pair axis is pred
        euler  (N,K,2)    int64   chi of both maps

    Both maps go through one call and one workspace; the result equals that of two betti_numbers calls."""
    _check_topology("betti_error", [(pred, "pred"), (target, "target")], num_classes, connectivity)
    return ops.betti_error(pred, target, num_classes, connectivity=connectivity)


def _check_confusion(name, pred, target, num_classes, ignore_index, return_labels):
    """Every ValueError of the confusion family, before any GPU work."""
    if not isinstance(target, torch.Tensor) or target.dim() not in (3, 4):
        raise ValueError("%s expects 3-D (N,H,W) or 4-D (N,D,H,W) labels as target" % name)
    if target.dtype != torch.int64:
        raise ValueError("%s: target must be int64 labels, got %s" % (name, target.dtype))
    if target.numel() == 0:
        raise ValueError("%s: empty label map %s" % (name, tuple(target.shape)))
    _check_num_classes(name, num_classes)
    if not isinstance(pred, torch.Tensor):
        raise ValueError("%s expects a tensor as pred: int64 labels or float32 / bfloat16 logits" % name)
    if pred.dtype == torch.int64:
        if pred.shape != target.shape:
            raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(pred.shape), tuple(target.shape)))
        if return_labels:
            raise ValueError("%s: return_labels needs logits as pred (a label map is its own argmax)" % name)
    elif pred.dtype in (torch.float32, torch.bfloat16):
        want = (target.shape[0], num_classes) + tuple(target.shape[1:])
        if tuple(pred.shape) != want:
            raise ValueError("%s: logits must have the shape (N, num_classes, dims) = %s for a target %s, got %s"
                             % (name, want, tuple(target.shape), tuple(pred.shape)))
    else:
        raise ValueError("%s: pred must be int64 labels or float32 / bfloat16 logits, got %s" % (name, pred.dtype))
    if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)
                                     or not -2 ** 63 <= ignore_index < 2 ** 63):
        raise ValueError("%s: ignore_index must be None or an int (of 64 bits), got %r" % (name, ignore_index))


def confusion_matrix(pred, target, num_classes, ignore_index=None, reduce_batch=False, out=None, return_labels=False):
    """The (target, prediction) count matrix of every entry (definitions: "Confusion matrix and voxel overlap" in the module's
    docstring).  pred: int64 labels (N,dims), or fp32 / bf16 logits (N,K,dims) with K == num_classes whose argmax is taken inside
    the kernel; target: int64 labels (N,dims).  Returns Confusion, a namedtuple of device tensors:

        matrix       (N,K,K)   int64   [n,t,p] = #{counted v : target = t, pred = p}; rows are the truth
        pred_only    (N,K)     int64   #{counted v : pred = k, target outside [0, K)}
        target_only  (N,K)     int64   #{counted v : target = k, pred outside [0, K)}
        counted      (N,)      int64   voxels not left out by ignore_index
        labels       (N,dims)  int64   the argmax map, written in the same pass, with return_labels=True (logits only); else None

    reduce_batch=True drops the leading N: every entry adds into the same counters.  out: a Confusion of exactly the shapes the
    call would return; the call adds into its four count tensors without clearing them and returns it, which accumulates a
    dataset-level matrix over batches of any size with reduce_batch=True.  num_classes is at most 1024 (8 MB of matrix per entry);
    overlap_metrics has the scores for more classes without a matrix."""
    name = "confusion_matrix"
    _check_confusion(name, pred, target, num_classes, ignore_index, return_labels)
    if num_classes > ops.CONFUSION_MAX_K:
        raise ValueError("%s takes at most %d classes (8 MB of matrix per entry), got %d: overlap_metrics has the per-class scores "
                         "for up to 65535 classes without a matrix" % (name, ops.CONFUSION_MAX_K, num_classes))
    if out is not None:
        shapes = ops.confusion_shapes(target.shape[0], num_classes, reduce_batch)
        if not isinstance(out, Confusion):
            raise ValueError("%s: out must be a Confusion, got %s" % (name, type(out).__name__))
        for field, t, s in zip(Confusion._fields, out[:4], shapes):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != s or not t.is_contiguous() \
                    or t.device != target.device:
                raise ValueError("%s: out.%s must be a contiguous int64 tensor of shape %s on the target's device"
                                 % (name, field, s))
    _require_gpu(pred, "pred")
    _require_gpu(target, "target")
    return ops.confusion_matrix(pred, target, num_classes, ignore_index=ignore_index, reduce_batch=bool(reduce_batch), out=out,
                                return_labels=bool(return_labels))


def overlap_metrics(pred, target, num_classes, ignore_index=None, reduce_batch=False, return_labels=False):
    """Per-class voxel overlap scores of every entry without building the matrix (definitions: "Confusion matrix and voxel
    overlap" in the module's docstring).  pred, target, ignore_index, reduce_batch and return_labels as for confusion_matrix;
    num_classes up to 65535.  Returns OverlapMetrics, a namedtuple of device tensors:

        overlap      (N,K,3)   int64   |A|, |B|, |A n B| over the counted voxels
        counted      (N,)      int64   voxels not left out by ignore_index
        dice, iou, precision, recall, specificity   (N,K) fp32 each; NaN when the denominator is 0
        labels       (N,dims)  int64   the argmax map with return_labels=True (logits only); else None

    With ignore_index=None, overlap and dice equal those of surface_distance_metrics bit for bit."""
    _check_confusion("overlap_metrics", pred, target, num_classes, ignore_index, return_labels)
    _require_gpu(pred, "pred")
    _require_gpu(target, "target")
    return ops.overlap_metrics(pred, target, num_classes, ignore_index=ignore_index, reduce_batch=bool(reduce_batch),
                               return_labels=bool(return_labels))


def overlap_scores(matrix):
    """The scores of overlap_metrics from finished count matrices (..., K, K) int64, rows = truth: for example an accumulated
    Confusion.matrix.  The matrix is taken as complete: |A_k| is its column sum, |B_k| its row sum and counted its total (what
    pred_only and target_only hold is not in it).  Returns OverlapScores with the leading shape: overlap (...,K,3) int64, counted
    (...) int64 and dice, iou, precision, recall, specificity (...,K) fp32, through the same finish kernel."""
    if not isinstance(matrix, torch.Tensor) or matrix.dim() < 2 or matrix.shape[-1] != matrix.shape[-2]:
        raise ValueError("overlap_scores expects count matrices (..., K, K)")
    if matrix.dtype != torch.int64:
        raise ValueError("overlap_scores: the matrix must be int64, got %s" % matrix.dtype)
    if matrix.numel() == 0:
        raise ValueError("overlap_scores: empty matrix %s" % (tuple(matrix.shape),))
    _check_num_classes("overlap_scores", int(matrix.shape[-1]))
    _require_gpu(matrix, "matrix")
    return ops.overlap_scores(matrix)
