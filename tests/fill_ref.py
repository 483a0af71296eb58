"""Host restatement of the hole filling (cfun_amd/components.py fill_holes, cfun_amd/csrc/fill.hip) on
scipy.ndimage.binary_fill_holes and scipy.ndimage.label.  Plain and slow on purpose; the device is compared against this with
torch.equal, and this against hand-written answers in tests/test_fill_ref.py.  The reference project has no such function: this
file and those answers are the pin."""
import numpy as np
from scipy import ndimage


def structure(connectivity, axis=None):
    """The 3-D structures of 6 / 26, or the 2-D ones of 4 / 8 for a planar fill."""
    if axis is None:
        assert connectivity in (6, 26)
        return ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    assert axis in (0, 1, 2) and connectivity in (4, 8)
    return ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)


def group_holes(obj, connectivity, axis=None):
    """obj: bool [D,H,W].  -> (holes bool [D,H,W], number of hole components): holes = binary_fill_holes(obj) & ~obj and
    label(holes)[1]; the planar form is a loop over the planes perpendicular to ``axis`` with the counts summed."""
    st = structure(connectivity, axis)
    if axis is None:
        holes = ndimage.binary_fill_holes(obj, structure=st) & ~obj
        return holes, int(ndimage.label(holes, structure=st)[1])
    holes = np.zeros(obj.shape, bool)
    count = 0
    for p in range(obj.shape[axis]):
        idx = [slice(None)] * 3
        idx[axis] = p
        plane = obj[tuple(idx)]
        h = ndimage.binary_fill_holes(plane, structure=st) & ~plane
        holes[tuple(idx)] = h
        count += int(ndimage.label(h, structure=st)[1])
    return holes, count


def fill(pred, num_classes, by="class", connectivity=None, axis=None, fill_value=1):
    """-> (filled uint8 [D,H,W], stats int64 [K,2]).  Groups: class k = 1 .. K-1 with object pred == k (by="class"), or the one
    group with object pred != 0, row 0 (by="foreground").  The groups are applied in descending k, each writing its id (or
    fill_value) where pred == 0 and the output is still 0.  stats[g] = (hole components of group g, voxels changed to g)."""
    pred = np.asarray(pred).astype(np.uint8)
    assert pred.ndim == 3 and by in ("class", "foreground")
    k = int(num_classes)
    if connectivity is None:
        connectivity = 6 if axis is None else 4
    stats = np.zeros((k, 2), np.int64)
    out = pred.copy()
    if pred.size == 0:
        return out, stats
    groups = [(0, pred != 0, fill_value)] if by == "foreground" else [(c, pred == c, c) for c in range(k - 1, 0, -1)]
    for g, obj, value in groups:
        holes, count = group_holes(obj, connectivity, axis)
        write = holes & (pred == 0) & (out == 0)
        out[write] = value
        stats[g] = (count, int(write.sum()))
    return out, stats


def open_components(pred, num_classes, by, connectivity, axis=None):
    """Per group the number of complement components that are NOT holes (the open side), for the cases' own assertions."""
    pred = np.asarray(pred)
    k = int(num_classes)
    st = structure(connectivity, axis)
    groups = [(0, pred != 0)] if by == "foreground" else [(c, pred == c) for c in range(1, k)]
    res = np.zeros(k, np.int64)
    for g, obj in groups:
        holes, _ = group_holes(obj, connectivity, axis)
        rest = ~obj & ~holes
        if axis is None:
            res[g] = ndimage.label(rest, structure=st)[1]
        else:
            for p in range(pred.shape[axis]):
                idx = [slice(None)] * 3
                idx[axis] = p
                res[g] += ndimage.label(rest[tuple(idx)], structure=st)[1]
    return res
