"""Connected components of a class map on the device (include/cfun_cc.h, cfun_amd/csrc/cc.hip): the post-processing step that
sits between ``detect_original`` and the scoring -- keep the largest component of each structure (or of the organ as a whole),
drop the specks below a size.

    label_components   int32 [D,H,W] labels: 0 for background, else 1 + the smallest linear index of the voxel's component
    clean_components   the cleaned uint8 map and the int64 [K,3] statistics, both left on the device
    Postprocess        the four settings as a value object, for ``evaluate.detect_original`` / ``evaluate.run_test``

The reference has no such function: nothing here is pinned by it.  The pin is ``scipy.ndimage.label`` on the host
(tests/cc_ref.py) and hand-written known answers (tests/test_cc_ref.py).  Nothing in this module synchronises.
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
