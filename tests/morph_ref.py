"""Host restatement of the ball morphology (cfun_amd/morphology.py, cfun_amd/csrc/morph.hip, include/cfun_morph.h) on
scipy.ndimage.binary_erosion / binary_dilation with an explicitly built structuring element.  Plain and slow on purpose; the
device is compared against this with torch.equal, and this against a brute-force three-sweep field and hand-written answers in
tests/test_morph_ref.py.  The reference project has no such function: this file and those answers are the pin."""
import numpy as np
from scipy import ndimage

OPS = ("erode", "dilate", "open", "close")
F = np.float32


def squares(spacing, radius):
    """(sz2, sy2, sx2) and r2 as the float32 of the double products."""
    with np.errstate(over="ignore"):
        s2 = tuple(F(np.float64(v) * np.float64(v)) for v in spacing)
        r2 = F(np.float64(radius) * np.float64(radius))
    return s2, r2


def term(k, a2):
    """fl(float(k * k) * a2), elementwise."""
    return (np.asarray(k, np.int64) ** 2).astype(F) * F(a2)


def reach(a2, r2, limit=4096):
    """The largest k <= limit with fl(float(k * k) * a2) <= r2."""
    k = 0
    while k < limit and term(k + 1, a2) <= r2:
        k += 1
    return k


def ball(spacing, radius):
    """The structuring element by the float32 rule of cfun_morph.h: bool [2 Rz + 1, 2 Ry + 1, 2 Rx + 1], origin at the centre."""
    (sz2, sy2, sx2), r2 = squares(spacing, radius)
    rz, ry, rx = reach(sz2, r2), reach(sy2, r2), reach(sx2, r2)
    dz, dy, dx = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    d = ((term(dx, sx2) + term(dy, sy2)).astype(F) + term(dz, sz2)).astype(F)
    b = d <= r2
    assert b[rz, ry, rx] and np.array_equal(b, b[::-1, ::-1, ::-1])
    return b


def dilate(obj, b):
    """Nothing outside the volume is ever a seed."""
    return ndimage.binary_dilation(obj, structure=b, border_value=0)


def erode(obj, b, outside):
    return ndimage.binary_erosion(obj, structure=b, border_value=int(outside))


def binary(obj, b, op, outside):
    """The binary result of one op on one group's object."""
    if op == "erode":
        return erode(obj, b, outside)
    if op == "dilate":
        return dilate(obj, b)
    if op == "open":
        return dilate(erode(obj, b, outside), b)
    assert op == "close"
    return erode(dilate(obj, b), b, outside)


def groups_of(pred, k, by, classes):
    """(row of stats, object, value written) per group, highest class first."""
    if by == "foreground":
        return [(0, pred != 0, None)]
    sel = range(1, k) if classes is None else sorted(set([classes] if isinstance(classes, int) else classes))
    return [(c, pred == c, c) for c in sorted(sel, reverse=True)]


def morph(pred, num_classes, op, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1):
    """-> (map uint8 [D,H,W], stats int64 [K,2]).  Each group's op on the INPUT map; erode and open clear the group's voxels that
    are not in the result; dilate and close set the zero voxels that are, highest class first.  stats[g] = (cleared, set)."""
    pred = np.asarray(pred).astype(np.uint8)
    assert pred.ndim == 3 and by in ("class", "foreground") and op in OPS
    k = int(num_classes)
    if outside is None:
        outside = 1 if op == "close" else 0
    stats = np.zeros((k, 2), np.int64)
    out = pred.copy()
    if pred.size == 0:
        return out, stats
    b = ball(spacing, radius)
    for g, obj, value in groups_of(pred, k, by, classes):
        res = binary(obj, b, op, outside)
        if op in ("erode", "open"):
            clear = obj & ~res
            out[clear] = 0
            stats[g, 0] = int(clear.sum())
        else:
            put = res & (pred == 0) & (out == 0)
            out[put] = fill_value if value is None else value
            stats[g, 1] = int(put.sum())
    return out, stats


def changed_fraction(pred, num_classes, op, radius, spacing, by, classes=None, outside=None):
    """Of the voxels the op could change (the groups' own for erode and open, the zeros for dilate and close), the fraction
    that does: the cases assert on this that an input tests both sides."""
    pred = np.asarray(pred)
    out, _ = morph(pred, num_classes, op, radius, spacing, by, classes, outside, 1)
    if op in ("erode", "open"):
        cand = np.zeros(pred.shape, bool)
        for _, obj, _ in groups_of(pred, int(num_classes), by, classes):
            cand |= obj
    else:
        cand = pred == 0
    n = int(cand.sum())
    return (float((out != pred).sum()) / n) if n else 0.0
