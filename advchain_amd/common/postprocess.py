"""Post-processing of label maps on the device (not in the reference; csrc/seg_components.hip): ``connected_components``,
``keep_largest_component``, ``remove_small_components``, ``fill_holes``, ``find_holes`` -- the step between ``argmax`` and
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

Holes (``fill_holes``, ``find_holes``: scipy.ndimage.binary_fill_holes per class, MONAI's FillHoles as its docstring has it).
Here ``connectivity`` is the adjacency OF THE BACKGROUND, scipy's ``structure`` argument; the default 1 is scipy's.  A background
component is a class of the transitive closure of "adjacent and both equal to ``background``", within one entry.  It touches
the border when one of its voxels has a coordinate equal to 0 or to size - 1 on any spatial axis.  Its enclosing labels are the
labels of all voxels that are adjacent, under the same connectivity, to a voxel of the component and are not ``background``.  A
hole is a background component that does not touch the border and whose enclosing labels are all one value k with 0 <= k < K =
``num_classes``: its voxels become k.  A component enclosed by two different labels stays background ("enclosed by a single
class"), and so does one adjacent to a label outside [0, K) (-100, K + 3).  Every voxel that is not background is copied
unchanged, labels outside [0, K) included.  With ``max_size`` = m only holes of at most m voxels are filled (skimage's
remove_small_holes).  Consequences: for a map with values in {0, 1}, K = 2 and background 0 the result is
scipy.ndimage.binary_fill_holes(mask, structure=generate_binary_structure(ndim, connectivity)) per entry; the result depends on
the map alone, not on any processing order; fill_holes(fill_holes(x)) == fill_holes(x).  MONAI's implementation, unlike its
docstring, floods ``img != label`` from the border once per label: it overwrites other classes that lie inside a class and
depends on the order of the labels.  That is not reproduced.

Every value is an integer and the same bits on every run; nothing is read back to the host, and every call can be captured in a
graph.  There is no gradient: the input is detached."""
import torch

from .. import ops
from ..ops import Components, Holes  # noqa: F401
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


def _check_holes(name, labels, num_classes, connectivity, background, max_size):
    _check_labels(name, labels, connectivity, background)
    _check_num_classes(name, num_classes)
    if max_size is not None and (isinstance(max_size, bool) or not isinstance(max_size, int) or max_size < 1):
        raise ValueError("%s: max_size must be None or a positive integer, got %r" % (name, max_size))
    _require_gpu(labels, "labels")
    return None if max_size is None else min(max_size, 2 ** 62)


def fill_holes(labels, num_classes, connectivity=1, background=0, max_size=None):
    """int64 (N, dims): the voxels of every hole -- a component of ``background`` under ``connectivity`` that does not touch the
    border of its entry and whose enclosing labels are all one class k in [0, num_classes) -- become k; with ``max_size`` only
    holes of at most that many voxels.  Every other voxel is copied unchanged (definitions: the module's docstring).  Equal to
    ``torch.where(h.fill >= 0, h.fill, labels)`` with h = find_holes(...)."""
    max_size = _check_holes("fill_holes", labels, num_classes, connectivity, background, max_size)
    return ops.fill_holes(labels, num_classes, connectivity=connectivity, background=background, max_size=max_size)


def find_holes(labels, num_classes, connectivity=1, background=0, max_size=None):
    """What fill_holes would fill, and a quality report ("the model left 14 holes in class 2").  Returns Holes, a namedtuple of
    device tensors:

        fill    (N, dims)  int64   the class a voxel would be filled with, -1 where nothing is filled
        count   (N, K)     int64   holes filled, per entry and enclosing class
        voxels  (N, K)     int64   voxels filled, per entry and enclosing class"""
    max_size = _check_holes("find_holes", labels, num_classes, connectivity, background, max_size)
    return ops.find_holes(labels, num_classes, connectivity=connectivity, background=background, max_size=max_size)
