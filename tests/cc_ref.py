"""Host restatement of the connected-component path (cfun_amd/components.py, cfun_amd/csrc/cc.hip) on scipy.ndimage.label.  Plain
and slow on purpose; the device is compared against this with torch.equal / np.array_equal, and this against hand-written
answers in tests/test_cc_ref.py.  The reference project has no such function: this file and those answers are the pin."""
import numpy as np
from scipy import ndimage


def _structure(connectivity):
    assert connectivity in (6, 26)
    return ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)


def _canonical(lab, n):
    """scipy's labels 1 .. n in its own scan order -> 1 + the smallest linear (C-order) index of each component."""
    out = np.zeros(lab.shape, np.int64)
    if n == 0:
        return out
    flat = lab.reshape(-1)
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size, dtype=np.int64))
    m = flat > 0
    out.reshape(-1)[m] = first[flat[m]] + 1
    return out


def label(pred, connectivity=26, by="class"):
    """pred: integer [D,H,W] array -> int32 [D,H,W]: 0 for a zero voxel, else 1 + the smallest linear index of its component.
    by="class": one scipy.ndimage.label per byte value present (every value, whatever K is); by="foreground": one on pred > 0."""
    pred = np.asarray(pred)
    assert pred.ndim == 3 and by in ("class", "foreground")
    st = _structure(connectivity)
    out = np.zeros(pred.shape, np.int64)
    if pred.size == 0:
        return out.astype(np.int32)
    masks = [pred > 0] if by == "foreground" else [pred == c for c in np.unique(pred) if c != 0]
    for m in masks:
        lab, n = ndimage.label(m, structure=st)
        out += _canonical(lab, n)                      # (the masks are disjoint)
    return out.astype(np.int32)


def clean(pred, num_classes, connectivity=26, by="class", largest_only=True, min_voxels=0):
    """-> (labels int32, cleaned uint8, stats int64 [K,3]).  Groups: class 1 .. K-1 (by="class") or the whole foreground, row 0
    (by="foreground").  A voxel keeps its byte iff its component's size >= min_voxels and, with largest_only, its component is its
    group's largest -- a tie goes to the smaller label.  Bytes >= K with by="class": in no group, copied through, in no statistic.
    stats[g] = (components, largest size, voxels removed)."""
    pred = np.asarray(pred).astype(np.uint8)
    k = int(num_classes)
    lab = label(pred, connectivity, by)
    stats = np.zeros((k, 3), np.int64)
    out = pred.copy()
    if pred.size == 0:
        return lab, out, stats
    sizes = np.bincount(lab.reshape(-1).astype(np.int64))          # sizes[label]; sizes[0] is the background
    groups = [(0, pred > 0)] if by == "foreground" else [(c, pred == c) for c in range(1, k)]
    for g, m in groups:
        roots = np.unique(lab[m])                                   # ascending: the first of several equal sizes is the smallest
        if roots.size == 0:
            continue
        sz = sizes[roots]
        winner = roots[int(np.argmax(sz))]                          # np.argmax returns the FIRST maximum
        keep = sizes[lab] >= min_voxels
        if largest_only:
            keep &= lab == winner
        drop = m & ~keep
        out[drop] = 0
        stats[g] = (roots.size, int(sz.max()), int(drop.sum()))
    return lab, out, stats
