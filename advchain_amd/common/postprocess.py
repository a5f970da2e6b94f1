"""Post-processing of label maps on the device (not in the reference; csrc/seg_components.hip): ``connected_components``,
``keep_largest_component``, ``remove_small_components`` -- the step between ``argmax`` and
``common.metrics.surface_distance_metrics`` in a validation loop.

Definitions.  labels is an int64 label map (N, dims), dims = (H, W) or (D, H, W).

Adjacency.  ``connectivity`` is an integer in 1 .. ndim with the meaning of scipy's generate_binary_structure(ndim, connectivity):
two voxels of an entry are adjacent when their offsets differ by at most 1 on every axis and on at most ``connectivity`` axes.  1
is faces (4 neighbours in 2D, 6 in 3D), 2 is 8 neighbours in 2D and 18 in 3D, 3 is 26 in 3D.

Foreground.  A voxel equal to ``background`` is background.  With ``num_classes`` = K every label outside [0, K), -100 included, is
background too (the rule of signed_distance_maps).  Two adjacent voxels are connected when they carry the same label and that label
is foreground; a component is a class of the transitive closure.  Components never span batch entries or label values.  Labels
are only compared; keep_largest_component alone uses a label as an index, after the range check.

Numbering.  The components of entry n are numbered 1 .. count[n] in the order of their smallest linear index (C order within the
entry).  This is canonical: it depends on the map alone, not on the order in which anything ran.  scipy.ndimage.label numbers one
binary mask in the same order; here all label values of an entry share one numbering.

Largest component.  For entry n and class k the largest component is the one with the most voxels; among equals the one with the
smaller smallest linear index.

Every value is an integer and the same bits on every run; nothing is read back to the host, and every call can be captured in a
graph.  There is no gradient: the input is detached."""
import torch

from .. import ops
from ..ops import Components  # noqa: F401
from .loss import _check_num_classes, _require_gpu


def _check_labels(name, labels, connectivity, background):
    if not isinstance(labels, torch.Tensor) or labels.dim() not in (3, 4):
        raise ValueError("%s expects 3-D (N,H,W) or 4-D (N,D,H,W) labels" % name)
    if labels.numel() == 0:
        raise ValueError("%s: empty label map %s" % (name, tuple(labels.shape)))
    nd = labels.dim() - 1
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity < 1 or connectivity > nd:
        raise ValueError("%s: connectivity must be an integer in 1..%d for %d spatial axes, got %r" % (name, nd, nd, connectivity))
    if isinstance(background, bool) or not isinstance(background, int) or not -2 ** 63 <= background < 2 ** 63:
        raise ValueError("%s: background must be an integer label, got %r" % (name, background))


def connected_components(labels, connectivity=1, background=0, num_classes=None, return_sizes=False):
    """The connected components of every entry (definitions: the module's docstring).  Returns Components, a namedtuple of device
    tensors:

        labels  (N, dims)  int32   0 on background, else the number of the voxel's component, 1 .. count[n]
        count   (N,)       int64   the number of components of each entry
        sizes   (N, dims)  int32   with return_sizes=True the voxel count of the component of each voxel, 0 on background; else None

    A size filter is one line on top: ``torch.where(c.sizes >= 10, x, 0)``; no output has a data-dependent shape."""
    _check_labels("connected_components", labels, connectivity, background)
    if num_classes is not None:
        _check_num_classes("connected_components", num_classes)
    _require_gpu(labels, "labels")
    return ops.connected_components(labels, connectivity=connectivity, background=background, num_classes=num_classes,
                                    return_sizes=bool(return_sizes))


def keep_largest_component(labels, num_classes, connectivity=1, background=0):
    """int64 (N, dims): for every entry and every class k in [0, num_classes) other than ``background``, a voxel of class k that is
    not in the largest component of class k of its entry becomes ``background``; ties go to the component with the smaller
    smallest linear index.  Every other voxel is copied unchanged, labels outside [0, num_classes) included."""
    _check_labels("keep_largest_component", labels, connectivity, background)
    _check_num_classes("keep_largest_component", num_classes)
    _require_gpu(labels, "labels")
    return ops.keep_largest_component(labels, num_classes, connectivity=connectivity, background=background)


def remove_small_components(labels, min_size, connectivity=1, background=0, num_classes=None):
    """int64 (N, dims): the voxels of components of fewer than ``min_size`` voxels become ``background``; every other voxel is
    copied unchanged.  A label that ``num_classes`` makes background is in no component, so it is copied as well:
    ``min_size=1`` returns the input, whatever ``num_classes`` is."""
    _check_labels("remove_small_components", labels, connectivity, background)
    if isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 1:
        raise ValueError("remove_small_components: min_size must be a positive integer, got %r" % (min_size,))
    if num_classes is not None:
        _check_num_classes("remove_small_components", num_classes)
    _require_gpu(labels, "labels")
    return ops.remove_small_components(labels, min(min_size, 2 ** 62), connectivity=connectivity, background=background,
                                       num_classes=num_classes)
