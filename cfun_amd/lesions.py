"""Lesion-level scores on the device (include/cfun_lesion.h, cfun_amd/csrc/lesion.hip): the half of a liver / tumour protocol
that voxel-wise Dice hides -- how many reference lesions were found, how many predicted lesions are false, the Dice of each
correspondence.

    rank_components    dense ranks 1 .. n (scipy.ndimage.label's numbering), the per-component table (root, voxels, bounding box,
                       class) and the count, all left on the device
    rank_overlap       the contingency table of two rank volumes: voxels per pair of components
    lesion_scores      label, rank and overlap for a prediction and a label volume: enqueues everything, returns the buffers
    LesionScores       the one ``.cpu()`` and the matching on the host, in integers and float64

The reference has no such function and the LiTS challenge's script is not pinned here: the matching rule is this project's own
definition, stated at ``LesionScores``.  The pins are ``scipy.ndimage.label`` / ``find_objects`` and a numpy contingency count
(tests/lesion_ref.py) and hand-written known answers (tests/test_lesion_ref.py).  Nothing in this module synchronises except
``LesionScores``.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream, workspace
from .components import _check_map, _label

MAX_CAP = _lib.LESION_MAX_CAP          # rows of a component table


def _check_cap(what, name, cap):
    c = int(cap)
    if not 1 <= c <= MAX_CAP:
        raise ValueError("%s: %s must lie in 1 .. %d, got %d" % (what, name, MAX_CAP, c))
    return c


def _rank(lib, pred, labels, dims, cap):
    ranks = torch.empty(dims, dtype=torch.int32, device=pred.device)
    count = torch.empty((2,), dtype=torch.int64, device=pred.device)
    table = torch.empty((cap + 2, _lib.LESION_FIELDS), dtype=torch.int64, device=pred.device)
    ws = workspace(lib.cfun_lesion_workspace_bytes(*dims, cap), pred)
    check(lib.cfun_cc_rank(ptr(pred), ptr(labels), (C.c_int32 * 3)(*dims), cap, ptr(ranks), ptr(count), ptr(table), ptr(ws),
                           ws.numel(), stream(pred)), "cc_rank")
    return ranks, table, count


def rank_components(pred, connectivity=26, by="class", cap=1023):
    """``label_components`` with the labels a user of ``scipy.ndimage.label`` expects.  pred, ``connectivity`` and ``by`` as there.
    Returns ``(ranks, table, count)``, all on the device, nothing synchronised:

        ranks   int32 [D,H,W]: 0 for a zero voxel, otherwise 1 + the number of components whose first voxel (in C order) comes
                earlier -- for one adjacency (``by="foreground"``, or a map of one class) exactly scipy's label array.  Always
                the true rank, whatever ``cap`` is.
        count   int64 [2]: (components, components beyond ``cap``)
        table   int64 [cap + 2, 9]: row r, 1 <= r <= cap, is (first voxel's linear index, voxels, z0, y0, x0, z1, y1, x1, class
                byte) of the component of rank r, the box half-open as ``find_objects`` gives it; zeros when there is no such
                component.  Row 0 is the background: (-1, zero voxels, the whole volume as its box, 0).  Row cap + 1 collects
                every component of rank above ``cap``: (-1, voxels summed, union of the boxes, -1), zeros when there is none.

    Raises before any launch on what ``label_components`` rejects or a ``cap`` outside 1 .. 4095."""
    cap = _check_cap("rank_components", "cap", cap)
    dims = _check_map("rank_components", pred, connectivity, by)
    lib = _lib.load()
    labels = _label(lib, pred, dims, connectivity, by, workspace(0, pred))
    return _rank(lib, pred, labels, dims, cap)


def rank_overlap(ranks_a, ranks_b, cap_a=1023, cap_b=1023):
    """ranks_a, ranks_b: dense int32 [D,H,W] rank volumes of one shape on the device.  Returns the int64
    [cap_a + 2, cap_b + 2] device tensor: cell [i][j] = voxels with ``min(a, cap_a + 1) == i`` and ``min(b, cap_b + 1) == j``.
    Row and column 0 are the backgrounds, the last row and column the overflow buckets; the cells sum to D * H * W.  Nothing is
    synchronised.  Raises before any launch on a volume that is not int32 [D,H,W], a shape or device mismatch, 2^31 - 1 voxels
    or more, or a cap outside 1 .. 4095."""
    cap_a, cap_b = _check_cap("rank_overlap", "cap_a", cap_a), _check_cap("rank_overlap", "cap_b", cap_b)
    for t in (ranks_a, ranks_b):
        if not torch.is_tensor(t) or t.dtype != torch.int32:
            raise ValueError("rank_overlap: int32 rank volumes expected, got %s" % (getattr(t, "dtype", type(t)),))
    if ranks_a.dim() != 3 or tuple(ranks_a.shape) != tuple(ranks_b.shape):
        raise ValueError("rank_overlap: %s and %s differ in shape ([D,H,W] both)" % (tuple(ranks_a.shape), tuple(ranks_b.shape)))
    if ranks_a.device != ranks_b.device:
        raise ValueError("rank_overlap: the two volumes sit on different devices")
    d, h, w = [int(v) for v in ranks_a.shape]
    if d * h * w >= (1 << 31) - 1:
        raise ValueError("rank_overlap: %d voxels, 2^31 - 1 or more" % (d * h * w))
    lib = _lib.load()
    overlap = torch.empty((cap_a + 2, cap_b + 2), dtype=torch.int64, device=ranks_a.device)
    ws = workspace(0, ranks_a)
    check(lib.cfun_rank_overlap(ptr(ranks_a), ptr(ranks_b), (C.c_int32 * 3)(d, h, w), cap_a, cap_b, ptr(overlap), ptr(ws),
                                ws.numel(), stream(ranks_a)), "rank_overlap")
    return overlap


LesionBuffers = collections.namedtuple("LesionBuffers", "packed cap thresholds")
LesionBuffers.__doc__ = """What ``lesion_scores`` leaves on the device: ``packed`` is one int64 tensor -- the reference side's count
[2] and table [cap + 2, 9], the predicted side's, then the overlap [cap + 2, cap + 2] (rows: reference) -- so that reading
it is one copy."""


def _class_ids(what, cls):
    ids = tuple(int(c) for c in cls) if isinstance(cls, (tuple, list)) else (int(cls),)
    if not ids or any(not 1 <= c <= 255 for c in ids):
        raise ValueError("%s: cls must be a class id in 1 .. 255 or a tuple of them, got %r" % (what, cls))
    return ids


def _lesion_map(t, ids):
    if t.is_floating_point():
        t = torch.trunc(t)                            # (as seg_confusion and surface_distances read a float label: 2.7 is class 2)
    m = t == ids[0]
    for c in ids[1:]:
        m = m | (t == c)
    return m.to(torch.uint8).contiguous()


def lesion_scores(pred, label, cls, connectivity=26, thresholds=(0.0, 0.5), cap=1023):
    """pred: dense uint8 [D,H,W] class map on the device.  label: a [D,H,W] view of the label volume with any strides and dtype
    (for the loader's [H,W,D] array pass ``label_hwd.permute(2, 0, 1)``).  ``cls``: the class id that counts as "lesion", or a
    tuple of ids that do together.  Both sides are reduced to a dense uint8 ``== cls`` map with torch -- element-wise plumbing,
    not a kernel of this library; a float label is truncated towards zero first, as ``seg_confusion`` and
    ``surface_distances`` read it -- then labelled under ``connectivity``, ranked and overlapped.  Everything is enqueued,
    nothing synchronised; returns the ``LesionBuffers`` that ``LesionScores`` reads.  Raises before any launch on a ``pred`` that
    is not uint8 [D,H,W], a shape or device mismatch, an unknown ``connectivity``, 2^31 - 1 voxels or more, a ``cls`` outside
    1 .. 255, a threshold outside [0, 1) or a ``cap`` outside 1 .. 4095."""
    cap = _check_cap("lesion_scores", "cap", cap)
    ids = _class_ids("lesion_scores", cls)
    ts = tuple(float(t) for t in thresholds)
    if not ts or any(not 0.0 <= t < 1.0 for t in ts):
        raise ValueError("lesion_scores: thresholds must lie in [0, 1), got %r" % (thresholds,))
    dims = _check_map("lesion_scores", pred, connectivity, "foreground")
    if not torch.is_tensor(label) or tuple(label.shape) != tuple(pred.shape):
        raise ValueError("lesion_scores: pred %s and label %s differ in shape ([D,H,W] both)"
                         % (tuple(pred.shape), tuple(getattr(label, "shape", ()))))
    if pred.device != label.device:
        raise ValueError("lesion_scores: pred and label sit on different devices")
    lib = _lib.load()
    parts, ranks = [], []
    for side in (label, pred):
        m = _lesion_map(side, ids)
        labels = _label(lib, m, dims, connectivity, "foreground", workspace(0, m))
        r, table, count = _rank(lib, m, labels, dims, cap)
        ranks.append(r)
        parts += [count, table.reshape(-1)]
    parts.append(rank_overlap(ranks[0], ranks[1], cap, cap).reshape(-1))
    return LesionBuffers(torch.cat(parts), cap, ts)


class LesionScores:
    """Lesion-level scores from ``lesion_scores``' buffers: one ``.cpu()``, then integers and float64 on the host.

    The matching rule (this project's definition, modelled on the merged correspondences of the LiTS protocol; the challenge's
    script is not pinned here).  Reference lesion g and predicted lesion p are linked when they share a voxel.  The connected
    groups of that bipartite graph are the correspondences: a lesion predicted in two pieces, or two lesions bridged by one
    prediction, are one group.  For a group with A reference voxels, B predicted voxels and I shared voxels

        iou = I / (A + B - I)        dice = 2 I / (A + B)

    and at threshold t every lesion of a group, of either side, counts as matched when the group has both sides and
    ``iou > t`` (strictly: an IoU of exactly 0.5 does not match at t = 0.5).

        n_ref, n_pred          lesions of either side
        sizes_ref, sizes_pred  int64 voxel counts, in rank order
        group_dice             float64, one per group, in the order of the group's first member (reference lesions before
                               predicted ones); 0 for a miss or a false positive
        group_iou              the same for the IoU
        groups                 per group (ranks of its reference lesions, ranks of its predicted lesions), 1-based
        recall[t]              matched reference lesions / n_ref
        precision[t]           matched predicted lesions / n_pred
        f1[t]                  2 P R / (P + R)
        truncated              True when either side has more lesions than ``cap``: the table cannot say which lesion
                               overlaps which, so every rate is nan, the group lists are empty and the size lists stop at cap

    A rate whose denominator is 0 is nan.  ``thresholds`` are those given to ``lesion_scores``."""

    def __init__(self, buffers):
        cap, self.thresholds = int(buffers.cap), tuple(buffers.thresholds)
        p = buffers.packed
        p = p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)
        f, rows = _lib.LESION_FIELDS, cap + 2
        if p.dtype != np.int64 or p.shape != (2 * (2 + rows * f) + rows * rows,):
            raise ValueError("LesionScores: the packed buffers of lesion_scores expected, got %s %s" % (p.dtype, p.shape))
        o = 0
        sides = []
        for _ in range(2):
            sides.append((p[o:o + 2], p[o + 2:o + 2 + rows * f].reshape(rows, f)))
            o += 2 + rows * f
        (cg, self.table_ref), (cp, self.table_pred) = sides
        self.overlap = p[o:].reshape(rows, rows)
        self.cap = cap
        self.n_ref, self.n_pred = int(cg[0]), int(cp[0])
        self.truncated = bool(cg[1] > 0 or cp[1] > 0)
        ng, npr = min(self.n_ref, cap), min(self.n_pred, cap)
        self.sizes_ref, self.sizes_pred = self.table_ref[1:1 + ng, 1].copy(), self.table_pred[1:1 + npr, 1].copy()
        nt = len(self.thresholds)
        self.recall, self.precision, self.f1 = np.full(nt, np.nan), np.full(nt, np.nan), np.full(nt, np.nan)
        self.groups, self.group_dice, self.group_iou = [], np.zeros(0), np.zeros(0)
        if self.truncated:
            return
        ov = self.overlap[1:1 + ng, 1:1 + npr]
        parent = list(range(ng + npr))                                # union-find over at most 2 * cap nodes

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        gs, ps = np.nonzero(ov)
        for g, q in zip(gs.tolist(), ps.tolist()):
            a, b = find(g), find(ng + q)
            if a != b:
                parent[max(a, b)] = min(a, b)                         # a root is its group's smallest node: the order below
        members = collections.OrderedDict()
        for i in range(ng + npr):
            members.setdefault(find(i), []).append(i)
        dice, iou = [], []
        matched_ref, matched_pred = np.zeros(nt, np.int64), np.zeros(nt, np.int64)
        for root in sorted(members):
            ref = [i for i in members[root] if i < ng]
            prd = [i - ng for i in members[root] if i >= ng]
            a, b = int(self.sizes_ref[ref].sum()), int(self.sizes_pred[prd].sum())
            inter = int(ov[np.ix_(ref, prd)].sum()) if ref and prd else 0
            self.groups.append(([i + 1 for i in ref], [i + 1 for i in prd]))
            dice.append(2.0 * inter / float(a + b))
            iou.append(float(inter) / float(a + b - inter))
            if ref and prd:
                for k, t in enumerate(self.thresholds):
                    if iou[-1] > t:
                        matched_ref[k] += len(ref)
                        matched_pred[k] += len(prd)
        self.group_dice, self.group_iou = np.array(dice, np.float64), np.array(iou, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.n_ref:
                self.recall = matched_ref / float(self.n_ref)
            if self.n_pred:
                self.precision = matched_pred / float(self.n_pred)
            self.f1 = 2.0 * self.precision * self.recall / (self.precision + self.recall)
