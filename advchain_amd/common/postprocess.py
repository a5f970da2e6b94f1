"""Post-processing of label maps on the device (not in the reference; csrc/seg_components.hip): ``connected_components``,
``keep_largest_component``, ``remove_small_components``, ``fill_holes``, ``find_holes``, and (csrc/seg_morph.hip) ``erosion``,
``dilation``, ``opening``, ``closing`` -- the step between ``argmax`` and ``common.metrics.surface_distance_metrics`` in a
validation loop.

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

Morphology with a Euclidean ball (``erosion``, ``dilation``, ``opening``, ``closing``; all take ``(labels, radius, num_classes,
sampling=None, background=0)``).  K = ``num_classes``; ``background`` is any integer label.  A class voxel carries a label k with
0 <= k < K and k != background; S_k is the set of voxels of entry n with label k.  A background voxel carries exactly
``background``.  Labels outside [0, K) (-100, K + 3) are neither: they are copied, never change, never grow, and count as
"another label".  Labels are only compared, never used as an address.  Nothing crosses batch entries.
The ball is B = {o in Z^nd : sum_a (s_a o_a)^2 <= radius^2} with s = ``sampling`` in axis order (1 when it is None); ``radius`` is
a finite number >= 0.  With unit spacing the test is the integer one, |o|^2 <= R2 with R2 = floor(radius * radius) taken in
float64 on the host and capped at 2^30 - 1, so radius=2 includes the offsets of squared length 4.  With a ``sampling`` the test is
on fp32 fields against radius^2 rounded to fp32.  radius=1 is the face cross; 1.5 is the 3x3 square in 2D and the 18-neighbourhood
in 3D; 1.8 is the 3x3x3 cube.  A ball that holds only the origin makes every function return a copy.
The image border: a position outside the image is nothing.  It is not a member of any class, so dilation gains nothing from it,
and it is not an obstacle, so erosion is not eaten from the image border: scipy's binary_dilation(..., border_value=0) and
binary_erosion(..., border_value=1), the convention of skimage and of MONAI's erode / dilate.  It makes opening anti-extensive
and closing extensive.  It is NOT scipy.ndimage.binary_closing, which erodes from the border with border_value=0.
  erosion   a class voxel v of class k keeps k iff every in-image v + o, o in B, carries k; otherwise it becomes ``background``.
            Equivalently: keep iff e(v) > radius^2, e(v) the squared distance to the nearest in-image voxel with a label other
            than labels[v] (+inf if there is none).  Everything that is not a class voxel is copied.
  dilation  a background voxel v becomes the class of the class voxel u that minimises (|S(v - u)|^2, labels[u]) lexicographically
            among the class voxels with |S(v - u)|^2 <= radius^2: nearest wins, among equally near the smaller class; it stays
            background if there is none.  Every other voxel is copied: classes never overwrite each other.
  opening   per class, E_k = binary erosion of S_k and O_k = {v : d^2(v, E_k) <= radius^2}, a subset of S_k.  A class voxel of
            class k outside O_k becomes ``background``; everything else is copied.  This is not dilation(erosion(x)), where freed
            voxels would be contested between classes.
  closing   per class, D_k = {v in the image : d^2(v, S_k) <= radius^2}, over voxels of any label, and C_k = {v : every in-image
            v + o, o in B, lies in D_k}, a superset of S_k.  A background voxel becomes k iff it lies in C_k for exactly one class
            k; a voxel claimed by two or more classes stays background (fill_holes's rule for a component between two classes:
            the result does not depend on any order).  Everything else is copied.
Consequences: for a map with values in {0, 1}, K = 2 and background 0 each function equals the scipy composition above with the
ball as ``structure``; opening(opening(x)) == opening(x) and closing(closing(x)) == closing(x); opening changes class voxels
only, to background; closing and dilation change background voxels only; the output is a function of the map alone.

Every value is an integer and the same bits on every run; nothing is read back to the host, and every call can be captured in a
graph.  There is no gradient: the input is detached."""
import math

import torch

from .. import ops
from ..ops import Components, Holes  # noqa: F401
from .loss import _check_num_classes, _check_sampling, _require_gpu


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


def _check_morph(name, labels, radius, num_classes, sampling, background):
    _check_labels(name, labels, 1, background)
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not math.isfinite(radius) or radius < 0:
        raise ValueError("%s: radius must be a finite number >= 0, got %r" % (name, radius))
    _check_num_classes(name, num_classes)
    sampling = _check_sampling(name, sampling, labels.dim() - 1)
    _require_gpu(labels, "labels")
    return sampling


def erosion(labels, radius, num_classes, sampling=None, background=0):
    """int64 (N, dims): a class voxel keeps its class iff every voxel of the image within the Euclidean ball of ``radius`` around it
    (``sampling``: the voxel spacing per axis) carries the same label; otherwise it becomes ``background``.  The image border
    does not erode.  Every other voxel is copied unchanged (definitions: the module's docstring).  One distance field whatever
    ``num_classes`` is, every scan bounded by the ball."""
    sampling = _check_morph("erosion", labels, radius, num_classes, sampling, background)
    return ops.erosion(labels, radius, num_classes, sampling=sampling, background=background)


def dilation(labels, radius, num_classes, sampling=None, background=0):
    """int64 (N, dims): a ``background`` voxel within ``radius`` of a class voxel becomes the class of the nearest one, the smaller
    class among equally near.  Every other voxel is copied unchanged: classes never overwrite each other, labels outside
    [0, num_classes) never grow.  One keyed distance field whatever ``num_classes`` is."""
    sampling = _check_morph("dilation", labels, radius, num_classes, sampling, background)
    return ops.dilation(labels, radius, num_classes, sampling=sampling, background=background)


def opening(labels, radius, num_classes, sampling=None, background=0):
    """int64 (N, dims): per class, the voxels that no ball of ``radius`` inside the class covers become ``background`` (thin bridges,
    specks); every other voxel is copied unchanged.  scipy.ndimage.binary_opening per class with the ball as structure, except
    that the image border does not erode."""
    sampling = _check_morph("opening", labels, radius, num_classes, sampling, background)
    return ops.opening(labels, radius, num_classes, sampling=sampling, background=background)


def closing(labels, radius, num_classes, sampling=None, background=0):
    """int64 (N, dims): a ``background`` voxel inside the closing of exactly one class by the ball of ``radius`` becomes that class
    (cracks and gaps that reach the background); one claimed by two classes stays.  Every other voxel is copied unchanged.
    Extensive, unlike scipy.ndimage.binary_closing, which erodes from the image border."""
    sampling = _check_morph("closing", labels, radius, num_classes, sampling, background)
    return ops.closing(labels, radius, num_classes, sampling=sampling, background=background)
