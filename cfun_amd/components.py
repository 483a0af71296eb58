"""Connected components of a class map on the device (include/cfun_cc.h, cfun_amd/csrc/cc.hip): the post-processing step that
sits between ``detect_original`` and the scoring -- keep the largest component of each structure (or of the organ as a whole),
drop the specks below a size.

    label_components   int32 [D,H,W] labels: 0 for background, else 1 + the smallest linear index of the voxel's component
    clean_components   the cleaned uint8 map and the int64 [K,3] statistics, both left on the device
    Postprocess        the four settings as a value object, for ``evaluate.detect_original`` / ``evaluate.run_test``

and the step that follows it (include/cfun_fill.h, cfun_amd/csrc/fill.hip): close the cavities a missed tumour, vessel or
low-contrast patch leaves in an organ mask, in 3-D or slice by slice.

    fill_holes         the filled uint8 map and the int64 [K,2] statistics, both left on the device
    FillHoles          its settings as a value object, optionally after a ``Postprocess``: the same ``postprocess=`` argument

The reference has no such functions: nothing here is pinned by it.  The pin is ``scipy.ndimage.label`` and
``scipy.ndimage.binary_fill_holes`` on the host (tests/cc_ref.py, tests/fill_ref.py) and hand-written known answers
(tests/test_cc_ref.py, tests/test_fill_ref.py).  Nothing in this module synchronises.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr, stream, workspace

MAX_CLASSES = 15          # cfun_cc_filter: K in 1 .. 15
_MODES = {"class": _lib.CC_CLASS, "foreground": _lib.CC_FOREGROUND}


def _check_map(what, pred, connectivity, by):
    if not torch.is_tensor(pred) or pred.dtype != torch.uint8:
        raise ValueError("%s: uint8 class map expected, got %s" % (what, getattr(pred, "dtype", type(pred))))
    if pred.dim() != 3:
        raise ValueError("%s: a [D,H,W] map expected, got shape %s" % (what, tuple(pred.shape)))
    if connectivity not in (6, 26):
        raise ValueError("%s: connectivity must be 6 or 26, got %r" % (what, connectivity))
    if by not in _MODES:
        raise ValueError("%s: by must be 'class' or 'foreground', got %r" % (what, by))
    d, h, w = [int(v) for v in pred.shape]
    if d * h * w >= (1 << 31) - 1:
        raise ValueError("%s: %d voxels, 2^31 - 1 or more" % (what, d * h * w))
    return d, h, w


def _label(lib, pred, dims, connectivity, by, ws):
    labels = torch.empty(dims, dtype=torch.int32, device=pred.device)
    check(lib.cfun_cc_label(ptr(pred), (C.c_int32 * 3)(*dims), connectivity, _MODES[by], ptr(labels), ptr(ws), ws.numel(),
                            stream(pred)), "cc_label")
    return labels


def label_components(pred, connectivity=26, by="class"):
    """pred: dense uint8 [D,H,W] class map on the device (what the un-mold kernels write).  Two non-zero voxels are adjacent when
    they are neighbours under ``connectivity`` -- 6 (faces) or 26 (faces, edges, corners) -- and, ``by="class"``, hold the same
    byte or, ``by="foreground"``, are both non-zero.  Returns the int32 [D,H,W] labels: 0 for a zero voxel, otherwise 1 + the
    smallest linear index ``(z * H + y) * W + x`` of any voxel of its component, so the result depends on the map alone and can
    be compared with ``torch.equal``.  Raises before any launch on a map that is not uint8 [D,H,W], an unknown ``connectivity``
    or ``by``, or 2^31 - 1 voxels or more."""
    dims = _check_map("label_components", pred, connectivity, by)
    lib = _lib.load()
    ws = workspace(lib.cfun_cc_workspace_bytes(*dims, 1), pred)
    return _label(lib, pred, dims, connectivity, by, ws)


def clean_components(pred, num_classes, connectivity=26, by="class", largest_only=True, min_voxels=0):
    """Label ``pred`` (as ``label_components``) and filter it.  The components are taken in groups: one group per class
    1 .. K-1 with ``by="class"``, the one group of all non-zero voxels with ``by="foreground"``.  A voxel keeps its byte iff its
    component holds at least ``min_voxels`` voxels and, with ``largest_only``, is the largest of its group (of several tied for
    largest: the one with the smallest label); every other voxel becomes 0.

    Returns ``(cleaned, stats)``: the uint8 [D,H,W] map and an int64 [K,3] tensor, both on the device, nothing synchronised.
    ``stats[g]`` = (components, voxels of the largest component, voxels removed) of group g: row c is class c with
    ``by="class"`` (row 0 is zero); row 0 is the foreground with ``by="foreground"`` (the other rows are zero).

    Bytes >= K: foreground like any other with ``by="foreground"`` (as ``> 0`` counts them, and as ``SegScores.mask_iou``
    does).  With ``by="class"`` they belong to no group -- they are copied through unchanged and appear in no row of
    ``stats``, the way ``seg_confusion`` keeps such ids in its "other" row instead of guessing a class for them.

    Raises before any launch on what ``label_components`` rejects, a ``num_classes`` outside 1 .. 15 or a negative
    ``min_voxels``."""
    k = int(num_classes)
    if not 1 <= k <= MAX_CLASSES:
        raise ValueError("clean_components: num_classes must lie in 1 .. %d, got %d" % (MAX_CLASSES, k))
    mv = int(min_voxels)
    if mv < 0:
        raise ValueError("clean_components: min_voxels must not be negative, got %d" % mv)
    mv = min(mv, 1 << 31)                                             # (no component is that large: the same filter)
    dims = _check_map("clean_components", pred, connectivity, by)
    lib = _lib.load()
    ws = workspace(lib.cfun_cc_workspace_bytes(*dims, k), pred)
    labels = _label(lib, pred, dims, connectivity, by, ws)
    out = torch.empty(dims, dtype=torch.uint8, device=pred.device)
    stats = torch.empty((k, 3), dtype=torch.int64, device=pred.device)
    check(lib.cfun_cc_filter(ptr(pred), ptr(labels), (C.c_int32 * 3)(*dims), k, _MODES[by], 1 if largest_only else 0, mv, ptr(out),
                             ptr(stats), ptr(ws), ws.numel(), stream(pred)), "cc_filter")
    return out, stats


class Postprocess:
    """The settings of ``clean_components`` as a value: ``Postprocess(connectivity=26, by="class", largest_only=True,
    min_voxels=0)``.  ``pp(pred, num_classes)`` -> ``(cleaned, stats)``."""
    __slots__ = ("connectivity", "by", "largest_only", "min_voxels")

    def __init__(self, connectivity=26, by="class", largest_only=True, min_voxels=0):
        if connectivity not in (6, 26):
            raise ValueError("Postprocess: connectivity must be 6 or 26, got %r" % (connectivity,))
        if by not in _MODES:
            raise ValueError("Postprocess: by must be 'class' or 'foreground', got %r" % (by,))
        if int(min_voxels) < 0:
            raise ValueError("Postprocess: min_voxels must not be negative, got %d" % int(min_voxels))
        self.connectivity, self.by, self.largest_only, self.min_voxels = connectivity, by, bool(largest_only), int(min_voxels)

    def __call__(self, pred, num_classes):
        return clean_components(pred, num_classes, self.connectivity, self.by, self.largest_only, self.min_voxels)

    def __eq__(self, other):
        return isinstance(other, Postprocess) and all(getattr(self, s) == getattr(other, s) for s in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, s) for s in self.__slots__))

    def __repr__(self):
        return "Postprocess(connectivity=%d, by=%r, largest_only=%r, min_voxels=%d)" % (self.connectivity, self.by,
                                                                                        self.largest_only, self.min_voxels)


def _check_fill(what, by, connectivity, axis, fill_value):
    """The settings of a fill, checked; returns (connectivity with its default resolved, fill_value as an int)."""
    if by not in _MODES:
        raise ValueError("%s: by must be 'class' or 'foreground', got %r" % (what, by))
    if axis is not None and axis not in (0, 1, 2):
        raise ValueError("%s: axis must be None, 0, 1 or 2, got %r" % (what, axis))
    allowed = (6, 26) if axis is None else (4, 8)
    if connectivity is None:
        connectivity = allowed[0]
    if connectivity not in allowed:
        raise ValueError("%s: connectivity must be %d or %d with axis=%r, got %r" % (what, allowed[0], allowed[1], axis, connectivity))
    try:
        fv = int(fill_value)
    except (TypeError, ValueError):
        fv = 0
    if not 1 <= fv <= 255 or fv != fill_value:
        raise ValueError("%s: fill_value must be an integer in 1 .. 255, got %r" % (what, fill_value))
    return connectivity, fv


def fill_holes(pred, num_classes, by="class", connectivity=None, axis=None, fill_value=1):
    """Fill the enclosed holes of a class map: ``scipy.ndimage.binary_fill_holes`` per group, written back into the map.

    ``pred``: dense uint8 [D,H,W] on the device, ``K = num_classes`` in 1 .. 15.  Returns ``(filled, stats)``: a new uint8 map
    and an int64 [K,2] tensor, both on the device, nothing synchronised.  Only voxels that are 0 in ``pred`` can change; no
    non-zero byte is ever rewritten.

    Groups.  ``by="class"``: one group per class k = 1 .. K-1; the group's object is ``pred == k`` and its complement is
    ``pred != k`` -- other classes, and bytes >= K, belong to the complement.  ``by="foreground"``: one group; its object is
    ``pred != 0``, bytes >= K included, and its complement is ``pred == 0``.

    Neighbourhood of the complement.  ``axis=None``: ``connectivity`` is 6 (scipy's ``generate_binary_structure(3, 1)``, the
    default of ``binary_fill_holes`` and the default here) or 26 (all ones).  ``axis`` in {0, 1, 2}: the volume is treated as
    independent 2-D planes perpendicular to that axis and ``connectivity`` is 4 (the default) or 8 within the plane;
    ``axis=0`` is the axial CT slice of a [D,H,W] map.  A 3-D cavity with one pinhole to the outside is not a hole in 3-D; it is
    one in nearly every slice.

    Holes.  A component of a group's complement is open when one of its voxels lies on a border: the six faces of the volume
    for ``axis=None``; the four edges of the plane for a planar fill (the two faces perpendicular to ``axis`` do not count).
    Every other component is enclosed, as in ``binary_fill_holes``, whose dilation enters from outside the array.

    Write.  A voxel with ``pred == 0`` in an enclosed component of group k becomes k.  With ``by="class"``, when several groups
    enclose the same voxel the HIGHEST class id wins: in LiTS the tumour (class 2) lies inside the liver (class 1), so a cavity
    inside a tumour ring becomes tumour, not liver.  With ``by="foreground"`` the voxel becomes ``fill_value`` (1 .. 255).

    ``stats[g]`` = (enclosed components of group g, voxels changed to g): row k is class k with ``by="class"`` (row 0 is
    zero); row 0 is the foreground with ``by="foreground"`` (the other rows are zero).  The two columns can differ in either
    direction: an enclosed component made only of other classes' voxels (a tumour wholly inside the liver) changes nothing, and
    a voxel enclosed by two groups is counted for the winner only.

    Raises ``ValueError`` before any launch on a map that is not uint8 [D,H,W], 2^31 - 1 voxels or more, a ``num_classes``
    outside 1 .. 15, an unknown ``by``, an ``axis`` other than None, 0, 1, 2, a ``connectivity`` that does not fit ``axis`` or a
    ``fill_value`` outside 1 .. 255."""
    k = int(num_classes)
    if not 1 <= k <= MAX_CLASSES:
        raise ValueError("fill_holes: num_classes must lie in 1 .. %d, got %d" % (MAX_CLASSES, k))
    connectivity, fv = _check_fill("fill_holes", by, connectivity, axis, fill_value)
    dims = _check_map("fill_holes", pred, 6, by)
    lib = _lib.load()
    ws = workspace(lib.cfun_fill_workspace_bytes(*dims, k), pred)
    out = torch.empty(dims, dtype=torch.uint8, device=pred.device)
    stats = torch.empty((k, 2), dtype=torch.int64, device=pred.device)
    check(lib.cfun_fill_holes(ptr(pred), (C.c_int32 * 3)(*dims), k, _MODES[by], connectivity, -1 if axis is None else axis, fv,
                              ptr(out), ptr(stats), ptr(ws), ws.numel(), stream(pred)), "fill_holes")
    return out, stats


class FillHoles:
    """The settings of ``fill_holes`` as a value: ``FillHoles(by="class", connectivity=None, axis=None, fill_value=1,
    clean=None)``.  ``clean`` is an optional ``Postprocess`` that runs first: keep the largest component, then fill.
    ``fh(pred, num_classes)`` -> ``(map, stats)`` with ``stats`` int64 [K,5]: the three columns of ``clean_components`` (zeros
    when ``clean`` is None) followed by the two of ``fill_holes``.  Usable wherever a ``Postprocess`` is: as the
    ``postprocess=`` argument of ``evaluate.detect_original`` / ``evaluate.run_test``."""
    __slots__ = ("by", "connectivity", "axis", "fill_value", "clean")

    def __init__(self, by="class", connectivity=None, axis=None, fill_value=1, clean=None):
        connectivity, fv = _check_fill("FillHoles", by, connectivity, axis, fill_value)
        if clean is not None and not isinstance(clean, Postprocess):
            raise ValueError("FillHoles: clean must be a Postprocess or None, got %r" % (clean,))
        self.by, self.connectivity, self.axis, self.fill_value, self.clean = by, connectivity, axis, fv, clean

    def __call__(self, pred, num_classes):
        if self.clean is not None:
            pred, clean_stats = self.clean(pred, num_classes)
        filled, fill_stats = fill_holes(pred, num_classes, self.by, self.connectivity, self.axis, self.fill_value)
        if self.clean is None:
            clean_stats = torch.zeros((fill_stats.shape[0], 3), dtype=torch.int64, device=fill_stats.device)
        return filled, torch.cat((clean_stats, fill_stats), dim=1)

    def __eq__(self, other):
        return isinstance(other, FillHoles) and all(getattr(self, s) == getattr(other, s) for s in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, s) for s in self.__slots__))

    def __repr__(self):
        return "FillHoles(by=%r, connectivity=%d, axis=%r, fill_value=%d, clean=%r)" % (self.by, self.connectivity, self.axis,
                                                                                        self.fill_value, self.clean)
