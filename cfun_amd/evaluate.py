"""Scoring a segmentation on the device: the reference's ``test()`` entry (heart_main.py:286-360; LiTS_2017/LiTS_main.py:285-367).

    seg_confusion     the (K+1) x (K+1) confusion counts of a predicted class map against a label volume, one pass over the two
                      volumes on the device (cfun_seg_confusion)
    SegScores         per-class IoU (utils.compute_per_class_mask_iou), foreground IoU (utils.compute_mask_iou) and Dice from
                      those exact integer counts, in float64
    detect_original   MaskRCNN.detect for one raw volume, un-molded into the ORIGINAL image's shape (model.py:1379-1381); the
                      class map stays a uint8 device tensor
    run_test          the loop of heart_main.test / LiTS_main.test: load, detect, score, optionally draw and save, mean and std
    surface_field     the surface voxels of one class and their exact squared Euclidean distance field (cfun_surface_field)
    surface_distances per class the sums, maxima and order statistics of the surface distances between two maps, one record
                      per class left on the device (cfun_surface_stats)
    SurfaceScores     Hausdorff, HD95, ASSD and RMSD from those records, in float64 (the reference has no such scores: the
                      pin is tests/surface_ref.py)
    lesion scores     ``run_test(lesions=...)``: lesion-level recall, precision and F1 (cfun_amd/lesions.py) and the tumour burden

The reference builds two float64 one-hot arrays [H,W,D,C-1] per case, casts them to float32 and takes the diagonal of a
[C-1,V] x [V,C-1] product; every figure it prints is a function of the (K+1)^2 integer counts computed here.  The scoring path
synchronises once per case: SegScores' copy of those counts to the host.
"""
import ctypes as C
import os
import time

import numpy as np
import torch

from . import _lib, lesions as lesions_mod, model, nifti, ops
from ._lib import check, ptr, stream, workspace
from .ops import ptr_raw

MAX_CLASSES = 15          # cfun_seg_confusion: (K + 1)^2 <= 256 bins
MAX_SURFACE_DIM = 4096    # cfun_surface_*: float(k * k) exact


def seg_confusion(pred, label, num_classes):
    """pred: dense uint8 [D,H,W] class map on the device (what the un-mold kernels write).  label: a [D,H,W] VIEW of the label
    volume with any strides, read in place -- for the loader's [H,W,D] array pass ``label_hwd.permute(2, 0, 1)``; nothing is
    copied.  uint8 and int32 labels are read as they are; every other dtype is converted to int32 on the device first, which
    TRUNCATES a non-integral float label towards zero (1.5 counts as class 1) where the reference's ``label == j + 1`` would
    match no class.  Returns the int64 [(K+1),(K+1)] device tensor ``counts[g][p]`` = voxels with label class g and predicted
    class p; values outside [0, K) on either side -- negative labels, stray ids -- fall into the extra row / column K, so
    ``counts.sum()`` is always D * H * W.  Raises before any launch on a shape mismatch, a ``pred`` that is not uint8 or a
    ``num_classes`` outside 1 .. 15."""
    k = int(num_classes)
    if not 1 <= k <= MAX_CLASSES:
        raise ValueError("seg_confusion: num_classes must lie in 1 .. %d, got %d" % (MAX_CLASSES, k))
    if pred.dtype != torch.uint8:
        raise ValueError("seg_confusion: uint8 class map expected, got %s" % (pred.dtype,))
    if pred.dim() != 3 or tuple(pred.shape) != tuple(label.shape):
        raise ValueError("seg_confusion: pred %s and label %s differ in shape ([D,H,W] both)" % (tuple(pred.shape), tuple(label.shape)))
    if pred.device != label.device:
        raise ValueError("seg_confusion: pred and label sit on different devices")
    d, h, w = [int(v) for v in pred.shape]
    if d * h * w >= 1 << 31:
        raise ValueError("seg_confusion: %d voxels, 2^31 or more" % (d * h * w))
    lib = _lib.load()
    if label.dtype not in (torch.uint8, torch.int32):
        label = label.to(torch.int32)
    counts = torch.empty((k + 1, k + 1), dtype=torch.int64, device=pred.device)
    ws = workspace(lib.cfun_seg_confusion_workspace_bytes(d, h, w, k), pred)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    check(lib.cfun_seg_confusion(ptr(pred), ptr_raw(label), 0 if label.dtype == torch.uint8 else 1, i64(*label.stride()),
                                 i32(d, h, w), k, ptr(counts), ptr(ws), ws.numel(), stream(pred)), "seg_confusion")
    return counts


class SegScores:
    """The reference's scores from the confusion counts (one ``.cpu()`` of (K+1)^2 int64 values, then float64 on the exact
    integers).  With ``I_j = counts[j][j]``, ``A1_j`` = row j's sum (label) and ``A2_j`` = column j's sum (prediction):

        per_class_iou [K-1]   I_j / (A1_j + A2_j - I_j + 1e-6), j = 1 .. K-1         utils.compute_per_class_mask_iou
        mask_iou              the same formula on label > 0 against pred > 0          utils.compute_mask_iou
        dice [K-1]            2 I_j / (A1_j + A2_j + 1e-6)

    ``mask_iou`` counts the "other" row / column (ids >= K) as foreground, as ``> 0`` does; its precondition is that labels are
    non-negative (a negative label is background to the reference and "other" here).  ``dice`` is this project's definition: the
    reference publishes a Dice figure but contains no Dice function.  ``counts`` is the numpy copy of the counts."""

    def __init__(self, counts):
        c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
        if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 2:
            raise ValueError("SegScores: [(K+1),(K+1)] counts expected, got %s" % (c.shape,))
        self.counts = c.astype(np.int64)
        k = c.shape[0] - 1
        self.num_classes = k
        rows, cols = self.counts.sum(axis=1), self.counts.sum(axis=0)
        inter = np.diagonal(self.counts)[1:k].astype(np.float64)
        a1, a2 = rows[1:k].astype(np.float64), cols[1:k].astype(np.float64)
        self.per_class_iou = inter / (a1 + a2 - inter + 1e-6)
        self.dice = 2.0 * inter / (a1 + a2 + 1e-6)
        total = int(self.counts.sum())
        g_fg, p_fg = total - int(rows[0]), total - int(cols[0])
        both = total - int(rows[0]) - int(cols[0]) + int(self.counts[0, 0])
        self.mask_iou = float(both) / (float(g_fg + p_fg - both) + 1e-6)


def _spacing2(what, spacing):
    """(sz, sy, sx) in millimetres -> the three float32 squares the kernels take: float32(double(s) * double(s))."""
    sp = [float(v) for v in spacing]
    if len(sp) != 3:
        raise ValueError("%s: spacing must be (sz, sy, sx), got %r" % (what, spacing))
    with np.errstate(over="ignore"):
        sq = [float(np.float32(np.float64(v) * np.float64(v))) for v in sp]
    if not all(v > 0.0 and np.isfinite(q) and q > 0.0 for v, q in zip(sp, sq)):
        raise ValueError("%s: every spacing must be finite and positive with a finite, positive float32 square, got %r"
                         % (what, spacing))
    return (C.c_float * 3)(*sq)


def _check_surface_map(what, pred):
    if not torch.is_tensor(pred) or pred.dtype != torch.uint8:
        raise ValueError("%s: uint8 class map expected, got %s" % (what, getattr(pred, "dtype", type(pred))))
    if pred.dim() != 3:
        raise ValueError("%s: a [D,H,W] map expected, got shape %s" % (what, tuple(pred.shape)))
    d, h, w = [int(v) for v in pred.shape]
    if max(d, h, w) > MAX_SURFACE_DIM:
        raise ValueError("%s: a dimension above %d in %s" % (what, MAX_SURFACE_DIM, (d, h, w)))
    if d * h * w >= (1 << 31) - 1:
        raise ValueError("%s: %d voxels, 2^31 - 1 or more" % (what, d * h * w))
    return d, h, w


def surface_field(map, cls, spacing):
    """map: dense uint8 [D,H,W] class map on the device; ``cls`` in 1 .. 255; ``spacing`` = (sz, sy, sx) in millimetres.
    Returns ``(surface, d2)``, both device tensors: uint8 [D,H,W], 1 on the voxels of class ``cls`` with a face neighbour
    that is outside the volume or of another class; float32 [D,H,W], the squared distance in mm^2 from every voxel to the
    nearest surface voxel (+inf everywhere when there is none), bit-identical to the float32 brute force of
    include/cfun_surface.h.  Nothing synchronises.  Raises before any launch on a map that is not uint8 [D,H,W], a dimension
    above 4096, 2^31 - 1 voxels or more, a ``cls`` outside 1 .. 255 or a spacing that is not finite and positive."""
    dims = _check_surface_map("surface_field", map)
    c = int(cls)
    if not 1 <= c <= 255:
        raise ValueError("surface_field: cls must lie in 1 .. 255, got %d" % c)
    s2 = _spacing2("surface_field", spacing)
    lib = _lib.load()
    surface = torch.empty(dims, dtype=torch.uint8, device=map.device)
    field = torch.empty(dims, dtype=torch.float32, device=map.device)
    ws = workspace(0, map)
    check(lib.cfun_surface_field(ptr(map), (C.c_int32 * 3)(*dims), c, s2, ptr(surface), ptr(field), ptr(ws), ws.numel(),
                                 stream(map)), "surface_field")
    return surface, field


def surface_distances(pred, label, num_classes, spacing, percentile=95.0):
    """pred: dense uint8 [D,H,W] class map on the device.  label: any [D,H,W] view of the label volume, of any integer or
    float dtype (for the loader's [H,W,D] array pass ``label_hwd.permute(2, 0, 1)``).  The kernels take two dense uint8 maps,
    so the label is turned into one with torch first -- a few element-wise passes over the volume, not a kernel of this
    library: a float label is truncated towards zero as ``seg_confusion`` does, and ids outside [0, K) become K, which
    belongs to no class on either side.  ``spacing`` = (sz, sy, sx) in millimetres; ``percentile`` in 0 .. 100.

    Returns the int64 [K, 11] device tensor of CfunSurfaceStats records (include/cfun_surface.h), one per class, row 0 all
    zeros: columns 0 and 1 are the counts, columns 2 .. 10 hold the bits of nine doubles.  ``SurfaceScores`` reads it.
    Nothing synchronises.  Raises before any launch on a shape mismatch, a ``pred`` that is not uint8 [D,H,W], tensors on
    different devices, a ``num_classes`` outside 1 .. 15, a dimension above 4096, 2^31 - 1 voxels or more, a spacing that is
    not finite and positive or a ``percentile`` outside 0 .. 100."""
    k = int(num_classes)
    if not 1 <= k <= MAX_CLASSES:
        raise ValueError("surface_distances: num_classes must lie in 1 .. %d, got %d" % (MAX_CLASSES, k))
    dims = _check_surface_map("surface_distances", pred)
    if not torch.is_tensor(label) or tuple(label.shape) != tuple(pred.shape):
        raise ValueError("surface_distances: pred %s and label %s differ in shape ([D,H,W] both)"
                         % (tuple(pred.shape), tuple(getattr(label, "shape", ()))))
    if pred.device != label.device:
        raise ValueError("surface_distances: pred and label sit on different devices")
    q = float(percentile)
    if not 0.0 <= q <= 100.0:
        raise ValueError("surface_distances: percentile must lie in 0 .. 100, got %r" % (percentile,))
    s2 = _spacing2("surface_distances", spacing)
    if label.is_floating_point():
        label = torch.trunc(label)
    elif label.dtype == torch.bool:
        label = label.to(torch.uint8)
    label = torch.where((label >= 0) & (label < k), label, k).to(torch.uint8).contiguous()
    lib = _lib.load()
    stats = torch.empty((k, _lib.SURFACE_STATS_FIELDS), dtype=torch.int64, device=pred.device)
    ws = workspace(lib.cfun_surface_workspace_bytes(*dims, k), pred)
    check(lib.cfun_surface_stats(ptr(pred), ptr(label), (C.c_int32 * 3)(*dims), k, s2, q / 100.0, ptr(stats), ptr(ws), ws.numel(),
                                 stream(pred)), "surface_stats")
    return stats


class SurfaceScores:
    """Surface-distance scores from ``surface_distances``' records: one ``.cpu()`` of K x 11 values, then float64 on the host.
    With A and B the surfaces of class j in the prediction and the label, d(a, B) the distance in mm from a voxel to the
    nearest voxel of B, every array [K-1] for the classes 1 .. K-1:

        hausdorff             max(max over A of d(a, B), max over B of d(b, A))
        hd_percentile         the ``percentile`` of the concatenation {d(a, B)} u {d(b, A)}, numpy's linear rule (HD95 at 95)
        asd_pred_to_label     mean over A of d(a, B)
        asd_label_to_pred     mean over B of d(b, A)
        assd                  the mean of those two directed means
        assd_pooled           (sum over A of d(a, B) + sum over B of d(b, A)) / (|A| + |B|), the other definition in use
        rmsd                  sqrt((sum over A of d(a, B)^2 + sum over B of d(b, A)^2) / (|A| + |B|))
        n_pred, n_label       |A|, |B| (int64)

    A class whose surface is empty on either side has ``nan`` in every score.  ``records`` is the numpy copy [K, 11]."""

    def __init__(self, stats):
        r = stats.detach().cpu().numpy() if torch.is_tensor(stats) else np.asarray(stats)
        if r.ndim != 2 or r.shape[1] != _lib.SURFACE_STATS_FIELDS or r.shape[0] < 1 or r.dtype != np.int64:
            raise ValueError("SurfaceScores: int64 [K, %d] records expected, got %s %s" % (_lib.SURFACE_STATS_FIELDS, r.dtype, r.shape))
        self.records = np.ascontiguousarray(r)
        self.num_classes = r.shape[0]
        v = self.records[1:, 2:].copy().view(np.float64)
        self.n_pred, self.n_label = self.records[1:, 0].copy(), self.records[1:, 1].copy()
        sum_pl, sum_lp, sumsq_pl, sumsq_lp, max_pl, max_lp, q_lo, q_hi, frac = [v[:, i] for i in range(9)]
        self.frac = frac
        npred, nlab = self.n_pred.astype(np.float64), self.n_label.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = (self.n_pred > 0) & (self.n_label > 0)
            nan = np.full(v.shape[0], np.nan)
            self.hausdorff = np.where(ok, np.sqrt(np.maximum(max_pl, max_lp)), nan)
            self.hd_percentile = np.where(ok, (1.0 - frac) * np.sqrt(q_lo) + frac * np.sqrt(q_hi), nan)
            self.asd_pred_to_label = np.where(ok, sum_pl / npred, nan)
            self.asd_label_to_pred = np.where(ok, sum_lp / nlab, nan)
            self.assd = 0.5 * (self.asd_pred_to_label + self.asd_label_to_pred)
            self.assd_pooled = np.where(ok, (sum_pl + sum_lp) / (npred + nlab), nan)
            self.rmsd = np.where(ok, np.sqrt((sumsq_pl + sumsq_lp) / (npred + nlab)), nan)


def affine_spacing(affine):
    """(sz, sy, sx) of the device map [D,H,W] from the affine of the loader's [H,W,D] array: the column norms of its 3 x 3
    part are the spacings along H, W and D."""
    a = np.asarray(affine, dtype=np.float64)
    sh, sw, sd = [float(np.linalg.norm(a[:3, i])) for i in range(3)]
    return sd, sh, sw


def _is_lits(config):
    return hasattr(config, "PAD_IMAGE_SHAPE")


def _postprocess(res, postprocess, num_classes):
    """Replace ``mask_device`` by its cleaned map; zeros in, zeros out (an empty detection passes through the same kernels)."""
    raw = res["mask_device"]
    res["mask_device"], res["component_stats"] = postprocess(raw, num_classes)
    res["mask_device_raw"] = raw
    return res


def detect_original(hot, image, postprocess=None):
    """``MaskRCNN.detect`` (model.py:1341-1389; LiTS_2017/model.py:1373-1417) for ONE raw volume -- [H,W,D,1] for the heart
    configurations, [H,W,D] for the LiTS ones: ``hot.mold_inputs``, ``predict_inference``, then the un-mold into the ORIGINAL
    image's shape, as the reference does (``CFUNHotPath.detect_images`` un-molds into the network's).  Returns ``rois``
    (y1,x1,z1,y2,x2,z2), ``class_ids`` and ``scores`` as ``detect`` does, ``mask_device``: the class map as a uint8 [D,H,W]
    device tensor (``.permute(1, 2, 0)`` is the reference's [H,W,D] mask), and ``empty``: True when nothing was detected --
    ``mask_device`` is then all zeros (the reference crashes there).

    ``postprocess``: a ``components.Postprocess``, ``components.FillHoles`` or ``morphology.Morphology``, or None (the default:
    exactly the above).  With
    one, ``mask_device`` is the map cleaned by ``components.clean_components`` (and, with a ``FillHoles``, filled by
    ``components.fill_holes``) -- still on the device, nothing synchronised -- and the dict gains ``component_stats`` (the int64
    device tensor: [K,3] of a ``Postprocess``, [K,5] of a ``FillHoles``, two more columns after a ``Morphology``) and
    ``mask_device_raw`` (the map as un-molded).  The
    reference has no such step."""
    lits = _is_lits(hot.config)
    if image.ndim != (3 if lits else 4):
        raise ValueError("detect_original: %s volume expected, got shape %s" % ("[H,W,D]" if lits else "[H,W,D,1]", tuple(image.shape)))
    molded, _, windows = hot.mold_inputs([image])
    return detect_molded(hot, molded, tuple(float(v) for v in windows[0]), [int(v) for v in image.shape[:3]], postprocess)


def detect_molded(hot, molded, window, shape, postprocess=None):
    """``detect_original`` behind the mold: ``predict_inference`` on ``molded`` [1,1,D',H',W'], the un-mold through ``window``
    into a volume of ``shape`` = (h, w, d), then ``postprocess``.  ``cfun_amd.native.detect_native`` enters here with the
    tensor it molded from the scanner's grid and the RESAMPLED shape."""
    h, w, d = [int(v) for v in shape]
    det, masks = hot.predict_inference(molded[0:1], window)
    overlap = getattr(hot.config, "UNMOLD_OVERLAP_TILE", False)
    found = det.shape[1] > 0
    if found:
        probs = masks[0].permute(0, 2, 3, 4, 1).contiguous()          # [N, d, h, w, C]
        if overlap:
            rois, class_ids, scores, cmap = model.unmold_detections_overlap_device(det[0], probs, [1, d, h, w], window)
        else:
            boxes, _, keep = model._unmold_boxes(det[0], [1, d, h, w], window)
            found = keep.shape[0] > 0
            if found:
                rois, class_ids, scores, cmap = model.unmold_detections_device(det[0], probs, [1, d, h, w], window)
        found = found and rois.shape[0] > 0
    if not found:
        res = dict(rois=np.zeros((0, 6), np.int32), class_ids=np.zeros((0,), np.int32), scores=np.zeros((0,), np.float32),
                   mask_device=torch.zeros((d, h, w), dtype=torch.uint8, device=molded.device), empty=True)
    else:
        res = dict(rois=rois, class_ids=class_ids, scores=scores, mask_device=cmap, empty=False)
    if postprocess is not None:
        _postprocess(res, postprocess, int(hot.config.NUM_CLASSES))
    return res


def _load_case(case, index):
    """-> (image [H,W,D] array, label [H,W,D] array, affine, file name, shape to save at or None)"""
    if isinstance(case[0], (str, os.PathLike)):
        image_path, label_path = case[0], case[1]
        lab = nifti.load(label_path)
        return nifti.load(image_path).get_data(), lab.get_data(), lab.affine, os.path.basename(str(image_path)), tuple(lab.shape)
    image, label, affine = case[0], case[1], case[2]
    name = case[3] if len(case) > 3 else "case_%d.nii" % index
    return image, label, affine, name, (tuple(case[4]) if len(case) > 4 else None)


def _draw_box_edges(m, roi, value=10):
    """heart_main.py:336-348 on the [H,W,D] device map: the twelve edges of one box.  Indices are clipped to dim - 1 -- the
    reference raises an IndexError when a box touches the far face (y2 == H and so on)."""
    lim = [int(v) - 1 for v in m.shape]
    y1, x1, z1, y2, x2, z2 = [min(max(int(v), 0), lim[i % 3]) for i, v in enumerate(roi)]
    for y in (y1, y2):
        for z in (z1, z2):
            m[y, x1:x2, z] = value
    for x in (x1, x2):
        for z in (z1, z2):
            m[y1:y2, x, z] = value
    for y in (y1, y2):
        for x in (x1, x2):
            m[y, x, z1:z2] = value


def _lesion_settings(lesions, num_classes):
    """run_test's ``lesions`` argument -> None, or the keyword arguments of ``lesions.lesion_scores``."""
    if lesions is None:
        return None
    opts = dict(lesions) if isinstance(lesions, dict) else {"cls": lesions}
    unknown = set(opts) - {"cls", "thresholds", "connectivity", "cap"}
    if unknown or "cls" not in opts:
        raise ValueError("run_test: lesions must be a class id, a tuple of them, or a dict with 'cls' and optionally "
                         "'thresholds', 'connectivity' and 'cap', got %r" % (lesions,))
    ids = lesions_mod._class_ids("run_test", opts["cls"])
    if any(c >= num_classes for c in ids):
        raise ValueError("run_test: lesion class %r outside 1 .. %d" % (opts["cls"], num_classes - 1))
    opts["cls"] = ids
    opts["thresholds"] = tuple(float(t) for t in opts.get("thresholds", (0.0, 0.5)))
    return opts


def _tumour_burden(counts, ids):
    """(label, prediction): lesion voxels / all non-zero voxels from the confusion counts; nan when a side is all zeros."""
    rows, cols, total = counts.sum(axis=1), counts.sum(axis=0), int(counts.sum())
    out = []
    for sums in (rows, cols):
        fg = total - int(sums[0])
        out.append(float(sum(int(sums[c]) for c in ids)) / float(fg) if fg else float("nan"))
    return out


def run_test(hot, cases, save_dir=None, draw_bbox=False, limit=None, postprocess=None, surface=None, lesions=None):
    """The loop of ``heart_main.test`` (and of ``LiTS_main.test`` when ``hot.config`` is a LiTS configuration).

    ``cases``: each either ``(image_path, label_path)`` -- NIfTI files read with cfun_amd.nifti -- or ``(image, label, affine)``
    arrays [H,W,D] (optionally followed by a file name and, for LiTS, the shape to save at); ``limit``: only the first so many.
    Per case: ``detect_original``, ``seg_confusion`` of the device map against the label read in place, ``SegScores``.  Returns a
    dict: ``per_class_ious`` [n, K-1], ``mean`` and ``std`` over the cases (axis 0), ``total_mean``, ``mask_ious`` [n], ``dice``
    [n, K-1], ``detect_time`` (seconds, summed, as the reference measures it around detect), ``results`` (detect_original's
    dicts) and ``saved`` (paths).

    ``save_dir``: the map is written as [H,W,D] int32 with the label's affine under the reference's name rule
    ``str(per_class_iou.mean()) + "_" + basename``; with ``draw_bbox`` the twelve edges of ``rois[0]`` are set to 10 first
    (indices clipped to dim - 1: the reference raises an IndexError when a box touches the far face).

    LiTS configurations follow LiTS_main.test: ``rois`` are clipped as at LiTS_main.py:319-323, ``draw_bbox`` fills every box with
    100, the saved map gets an order-0 resize to the NIfTI's own shape and is stored uint8, and with a detector-only stage
    ('beginning') the mask is zeros and the mask scores are skipped (the file name then starts with "detector": the fork's
    box-IoU figure is not computed here).

    ``postprocess``: a ``components.Postprocess``, ``components.FillHoles`` or ``morphology.Morphology`` handed to
    ``detect_original``, or None (the
    default: exactly the above).  With one, the cleaned (and filled) map is what is scored, drawn into and saved; each result dict carries ``component_stats`` and
    ``mask_device_raw``.  The step adds no synchronisation -- still one per case -- and the statistics stay on the device
    until the caller reads them.

    ``surface``: None (the default: exactly the above), True, or a percentile in 0 .. 100 (True means 95).  With one,
    ``surface_distances`` runs on the map that is scored -- the cleaned one when ``postprocess`` is given -- against the label,
    with the voxel spacing taken from the label's affine (``affine_spacing``).  The dict gains ``hausdorff``, ``hd95`` (the
    chosen percentile) and ``assd``, each [n, K-1] in millimetres, and each result carries its ``SurfaceScores`` under
    ``surface_scores``.  The records are read right after the confusion counts with nothing enqueued in between: still one
    point of synchronisation per case.  Detector-only LiTS runs skip it, as they skip the mask scores.

    ``lesions``: None (the default: exactly the above), the class id that counts as "lesion" (2 for the LiTS configurations'
    tumour), a tuple of ids that do together, or a dict ``{"cls": ..., "thresholds": (0.0, 0.5), "connectivity": 26,
    "cap": 1023}``.  With one, ``lesions.lesion_scores`` runs on the map that is scored -- the cleaned one when ``postprocess``
    is given -- against the label; it is enqueued before the confusion counts are read, and its buffers are read right after
    them: still one point of synchronisation per case.  The dict gains ``lesion_recall``, ``lesion_precision`` and
    ``lesion_f1``, each [n, len(thresholds)], ``lesion_counts`` [n, 2] (reference lesions, predicted lesions) and
    ``tumour_burden`` [n, 2] (lesion voxels / all non-zero voxels of the label and of the prediction, from the confusion
    counts), and each result carries its ``LesionScores`` under ``lesion_scores``.  Detector-only LiTS runs skip it too."""
    cfg = hot.config
    lits = _is_lits(cfg)
    k = int(cfg.NUM_CLASSES)
    detector_only = lits and bool(getattr(hot, "detector_phase_only", False))
    dev = next(hot.parameters()).device
    ious, mask_ious, dices, results, saved = [], [], [], [], []
    hds, hdqs, assds = [], [], []
    lesion_opts = _lesion_settings(lesions, k)
    les_recall, les_precision, les_f1, les_counts, burdens = [], [], [], [], []
    if surface is not None and surface is not False:
        percentile = 95.0 if surface is True else float(surface)
        if not 0.0 <= percentile <= 100.0:
            raise ValueError("run_test: surface must be None, True or a percentile in 0 .. 100, got %r" % (surface,))
    else:
        percentile = None
    detect_time = 0.0
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    for index, case in enumerate(list(cases)[:limit]):
        image, label, affine, name, save_shape = _load_case(case, index)
        image_t = torch.as_tensor(image)
        if lits:
            image_t = image_t.to(torch.float32)
        elif image_t.dim() == 3:
            image_t = image_t[..., None]                              # np.expand_dims(image, -1), heart_main.py:304
        start = time.time()
        res = detect_original(hot, image_t, postprocess)
        detect_time += time.time() - start
        results.append(res)
        pred = res["mask_device"]
        if detector_only:
            pred = torch.zeros_like(pred)
            res["mask_device"] = pred
            if postprocess is not None:                               # zeros in, zeros out: the statistics of an empty map
                res["mask_device_raw"] = pred
                res["component_stats"] = torch.zeros_like(res["component_stats"])
        rois = np.asarray(res["rois"])
        h, w, d = [int(v) for v in image_t.shape[:3]]
        if lits:
            rois = rois.clip(min=0)
            for axis, dim in ((3, h), (4, w), (5, d)):
                rois[:, axis] = rois[:, axis].clip(max=dim - 1)
            rois = res["rois"] = rois.astype(np.int32)
        prefix = "detector"
        if not detector_only:
            label_t = torch.as_tensor(label).to(dev)                  # keeps the array's own strides: nothing is re-laid out
            counts = seg_confusion(pred, label_t.permute(2, 0, 1), k)
            if percentile is not None:
                records = surface_distances(pred, label_t.permute(2, 0, 1), k, affine_spacing(affine), percentile)
            if lesion_opts is not None:
                lesion_buffers = lesions_mod.lesion_scores(pred, label_t.permute(2, 0, 1), **lesion_opts)
            s = SegScores(counts)
            if percentile is not None:                                # (nothing was enqueued since the counts were read)
                ss = res["surface_scores"] = SurfaceScores(records)
                hds.append(ss.hausdorff)
                hdqs.append(ss.hd_percentile)
                assds.append(ss.assd)
            if lesion_opts is not None:
                ls = res["lesion_scores"] = lesions_mod.LesionScores(lesion_buffers)
                les_recall.append(ls.recall)
                les_precision.append(ls.precision)
                les_f1.append(ls.f1)
                les_counts.append((ls.n_ref, ls.n_pred))
                burdens.append(_tumour_burden(s.counts, lesion_opts["cls"]))
            ious.append(s.per_class_iou)
            mask_ious.append(s.mask_iou)
            dices.append(s.dice)
            prefix = str(s.per_class_iou.mean())
        if save_dir is None:
            continue
        m = pred.permute(1, 2, 0)
        if draw_bbox and rois.shape[0]:
            m = m.clone()
            if lits:
                for y1, x1, z1, y2, x2, z2 in rois.tolist():
                    m[y1:y2, x1:x2, z1:z2] = 100
            else:
                _draw_box_edges(m, rois[0])
        if lits:
            if save_shape is not None and tuple(save_shape) != tuple(m.shape):
                m = torch.round(ops.resize3d(m.to(torch.float32), save_shape, order=0))
            out = m.to(torch.uint8).cpu().numpy()
        else:
            out = m.to(torch.int32).cpu().numpy()
        path = os.path.join(save_dir, prefix + "_" + name)
        nifti.save(nifti.Nifti1Image(out, affine), path)
        saved.append(path)
    nfg = k - 1
    per = np.array(ious, dtype=np.float64).reshape(len(ious), nfg)
    summary = dict(per_class_ious=per, mean=per.mean(axis=0) if len(ious) else np.full(nfg, np.nan),
                   std=per.std(axis=0) if len(ious) else np.full(nfg, np.nan),
                   total_mean=float(per.mean()) if len(ious) else float("nan"), mask_ious=np.array(mask_ious, dtype=np.float64),
                   dice=np.array(dices, dtype=np.float64).reshape(len(dices), nfg), detect_time=detect_time, results=results,
                   saved=saved)
    if percentile is not None:
        for key, rows in (("hausdorff", hds), ("hd95", hdqs), ("assd", assds)):
            summary[key] = np.array(rows, dtype=np.float64).reshape(len(rows), nfg)
    if lesion_opts is not None:
        nt = len(lesion_opts["thresholds"])
        for key, rows in (("lesion_recall", les_recall), ("lesion_precision", les_precision), ("lesion_f1", les_f1)):
            summary[key] = np.array(rows, dtype=np.float64).reshape(len(rows), nt)
        summary["lesion_counts"] = np.array(les_counts, dtype=np.int64).reshape(len(les_counts), 2)
        summary["tumour_burden"] = np.array(burdens, dtype=np.float64).reshape(len(burdens), 2)
    return summary
