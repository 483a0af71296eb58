"""Ball morphology of a class map on the device (include/cfun_morph.h, cfun_amd/csrc/morph.hip): the smoothing step between
"keep the largest component / fill the holes" (cfun_amd/components.py) and the scoring -- open a liver mask by 2 mm to shave off
leaks along vessels, close a ventricle by 1.5 mm to bridge a one-voxel gap, erode or dilate one class to build a margin.

    morph                              the map after one op and the int64 [K,2] statistics, both left on the device
    erode, dilate, open_ball, close_ball    the four ops by name
    Morphology                         the settings as a value object, optionally after a ``Postprocess``, ``FillHoles`` or another
                                       ``Morphology``: the same ``postprocess=`` argument of ``evaluate.detect_original`` / ``run_test``

The structuring element is the ball of a physical radius under the voxel spacing: an offset (dz, dy, dx) belongs to it iff
``fl(fl(fl(float(dx*dx)*sx2) + fl(float(dy*dy)*sy2)) + fl(float(dz*dz)*sz2)) <= r2`` in float32, with ``sx2`` the float32 of
the double ``sx * sx`` and ``r2`` that of ``radius * radius``.  It is exact under anisotropic spacing, which no iterated
6 / 26-neighbour element is.

The reference has no such function: nothing here is pinned by it.  The pin is ``scipy.ndimage.binary_erosion`` /
``binary_dilation`` with that ball built explicitly (tests/morph_ref.py), a brute-force restatement and hand-written known
answers (tests/test_morph_ref.py).  Nothing in this module synchronises.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream, workspace
from .components import MAX_CLASSES, _MODES, FillHoles, Postprocess, _check_map
from .evaluate import _spacing2

MAX_DIM = 4096            # cfun_morph_apply: float(k * k) is exact below 2^24
OPS = {"erode": _lib.MORPH_ERODE, "dilate": _lib.MORPH_DILATE, "open": _lib.MORPH_OPEN, "close": _lib.MORPH_CLOSE}


def _check_settings(what, op, radius, spacing, by, classes, outside, fill_value):
    """The settings of a morphological op, checked; returns (r2 as a float32 value, the three spacing squares as a C array,
    classes as a sorted tuple or None, outside with its default resolved, fill_value as an int)."""
    if op not in OPS:
        raise ValueError("%s: op must be 'erode', 'dilate', 'open' or 'close', got %r" % (what, op))
    if by not in _MODES:
        raise ValueError("%s: by must be 'class' or 'foreground', got %r" % (what, by))
    try:
        r = float(radius)
    except (TypeError, ValueError):
        r = float("nan")
    with np.errstate(over="ignore"):
        r2 = float(np.float32(np.float64(r) * np.float64(r)))
    if not (r >= 0.0 and np.isfinite(r2)):
        raise ValueError("%s: radius must be finite and not negative with a finite float32 square, got %r" % (what, radius))
    s2 = _spacing2(what, spacing)
    if classes is not None:
        try:
            cl = (int(classes),) if not isinstance(classes, (tuple, list, set, frozenset)) else tuple(int(c) for c in classes)
            exact = cl == ((classes,) if not isinstance(classes, (tuple, list, set, frozenset)) else tuple(classes))
        except (TypeError, ValueError):
            cl, exact = (), False
        if not exact or any(c < 1 or c > MAX_CLASSES - 1 for c in cl):
            raise ValueError("%s: classes must be None, an int or a tuple of ints in 1 .. K-1, got %r" % (what, classes))
        classes = tuple(sorted(set(cl)))
    if outside is None:
        outside = 1 if op == "close" else 0
    if outside not in (0, 1):
        raise ValueError("%s: outside must be None, 0 or 1, got %r" % (what, outside))
    try:
        fv = int(fill_value)
    except (TypeError, ValueError):
        fv = 0
    if not 1 <= fv <= 255 or fv != fill_value:
        raise ValueError("%s: fill_value must be an integer in 1 .. 255, got %r" % (what, fill_value))
    return r2, s2, classes, int(outside), fv


def _class_bits(what, classes, k):
    if classes is None:
        return (1 << k) - 2                                            # bits 1 .. K-1
    if any(c >= k for c in classes):
        raise ValueError("%s: classes %r do not all lie in 1 .. %d" % (what, classes, k - 1))
    bits = 0
    for c in classes:
        bits |= 1 << c
    return bits


def morph(pred, num_classes, op, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1):
    """One morphological op with a ball on a class map.

    ``pred``: dense uint8 [D,H,W] on the device, every dimension at most 4096, ``K = num_classes`` in 1 .. 15.  ``op`` is
    "erode", "dilate", "open" or "close".  ``radius`` is in the units of ``spacing`` = (sz, sy, sx); the default spacing is unit
    voxels, so the radius is then in voxels.  Returns ``(map, stats)``: a new uint8 map and an int64 [K,2] tensor, both on the
    device, nothing synchronised.

    Groups.  ``by="class"``: one group per class in ``classes`` -- None means all of 1 .. K-1, otherwise an int or a tuple of
    ints -- with object ``pred == k``; other classes and bytes >= K belong to its complement.  ``by="foreground"``: one group with
    object ``pred != 0`` (``classes`` is not looked at).

    Ops, per group, each computed on the INPUT map.  Dilate: every voxel with an object voxel at an offset in the ball.  Erode:
    every object voxel with no complement position at an offset in the ball; ``outside`` says what a position outside the volume
    counts as there: 1 object, 0 complement (scipy's ``border_value=0``).  Open: the dilation of the erosion, a subset of the
    object.  Close: the erosion of the dilation.  ``outside=None`` resolves to 0 for erode and open and to 1 for close, so that a
    closing never eats an organ that touches the scan's edge; dilate does not use it.

    Write.  Erode and open only clear: a voxel of group k that is not in the result becomes 0.  Dilate and close only set: a
    voxel with ``pred == 0`` in group k's result becomes k, or ``fill_value`` (1 .. 255) with ``by="foreground"``.  No non-zero
    byte is ever rewritten, and when several groups claim a zero voxel the HIGHEST class id wins, as in ``fill_holes``: a tumour
    grows into background, not into the liver, and the liver does not grow into the tumour.  Classes that are not selected and
    bytes >= K are copied through.

    ``stats[g]`` = (voxels of group g cleared, zero voxels set to g): row k is class k with ``by="class"``; row 0 is the
    foreground with ``by="foreground"``; every other row is zero.  A contested voxel is counted for the winner only.

    A radius below every spacing makes the ball the origin alone: the map is copied and the statistics are zero.

    Raises ``ValueError`` before any launch on a map that is not uint8 [D,H,W], a dimension above 4096, 2^31 - 1 voxels or
    more, a ``num_classes`` outside 1 .. 15, an unknown ``op`` or ``by``, a radius that is negative or not finite, a spacing that
    is not finite and positive, ``classes`` outside 1 .. K-1, an ``outside`` other than None, 0, 1 or a ``fill_value`` outside
    1 .. 255."""
    k = int(num_classes)
    if not 1 <= k <= MAX_CLASSES:
        raise ValueError("morph: num_classes must lie in 1 .. %d, got %d" % (MAX_CLASSES, k))
    r2, s2, classes, outside, fv = _check_settings("morph", op, radius, spacing, by, classes, outside, fill_value)
    bits = _class_bits("morph", classes, k)
    dims = _check_map("morph", pred, 6, by)
    if max(dims) > MAX_DIM:
        raise ValueError("morph: a dimension above %d in %s" % (MAX_DIM, dims))
    lib = _lib.load()
    ws = workspace(lib.cfun_morph_workspace_bytes(*dims, k), pred)
    out = torch.empty(dims, dtype=torch.uint8, device=pred.device)
    stats = torch.empty((k, 2), dtype=torch.int64, device=pred.device)
    check(lib.cfun_morph_apply(ptr(pred), (C.c_int32 * 3)(*dims), k, _MODES[by], OPS[op], bits, s2, r2, outside, fv, ptr(out),
                               ptr(stats), ptr(ws), ws.numel(), stream(pred)), "morph_apply")
    return out, stats


def erode(pred, num_classes, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1):
    """``morph(pred, num_classes, "erode", ...)``."""
    return morph(pred, num_classes, "erode", radius, spacing, by, classes, outside, fill_value)


def dilate(pred, num_classes, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1):
    """``morph(pred, num_classes, "dilate", ...)``."""
    return morph(pred, num_classes, "dilate", radius, spacing, by, classes, outside, fill_value)


def open_ball(pred, num_classes, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1):
    """``morph(pred, num_classes, "open", ...)``."""
    return morph(pred, num_classes, "open", radius, spacing, by, classes, outside, fill_value)


def close_ball(pred, num_classes, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1):
    """``morph(pred, num_classes, "close", ...)``."""
    return morph(pred, num_classes, "close", radius, spacing, by, classes, outside, fill_value)


class Morphology:
    """The settings of ``morph`` as a value: ``Morphology(op, radius, spacing=(1, 1, 1), by="class", classes=None,
    outside=None, fill_value=1, before=None)``.  The spacing is fixed at construction (the LiTS volumes are resampled to one
    mean spacing, the heart volumes resized to one shape).  ``before`` is an optional ``Postprocess``, ``FillHoles`` or
    ``Morphology`` that runs first.  ``m(pred, num_classes)`` -> ``(map, stats)`` with ``stats`` int64 [K, n + 2]: ``before``'s
    columns followed by the two of ``morph``.  Usable wherever a ``Postprocess`` is: as the ``postprocess=`` argument of
    ``evaluate.detect_original`` / ``evaluate.run_test``."""
    __slots__ = ("op", "radius", "spacing", "by", "classes", "outside", "fill_value", "before")

    def __init__(self, op, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1, before=None):
        _, _, classes, outside, fv = _check_settings("Morphology", op, radius, spacing, by, classes, outside, fill_value)
        if before is not None and not isinstance(before, (Postprocess, FillHoles, Morphology)):
            raise ValueError("Morphology: before must be a Postprocess, a FillHoles, a Morphology or None, got %r" % (before,))
        self.op, self.radius, self.spacing = op, float(radius), tuple(float(v) for v in spacing)
        self.by, self.classes, self.outside, self.fill_value, self.before = by, classes, outside, fv, before

    def __call__(self, pred, num_classes):
        before_stats = None
        if self.before is not None:
            pred, before_stats = self.before(pred, num_classes)
        out, stats = morph(pred, num_classes, self.op, self.radius, self.spacing, self.by, self.classes, self.outside,
                           self.fill_value)
        return out, (stats if before_stats is None else torch.cat((before_stats, stats), dim=1))

    def __eq__(self, other):
        return isinstance(other, Morphology) and all(getattr(self, s) == getattr(other, s) for s in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, s) for s in self.__slots__))

    def __repr__(self):
        return "Morphology(%r, %r, spacing=%r, by=%r, classes=%r, outside=%d, fill_value=%d, before=%r)" % (
            self.op, self.radius, self.spacing, self.by, self.classes, self.outside, self.fill_value, self.before)
