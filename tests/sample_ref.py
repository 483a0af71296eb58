"""TEST ONLY: numpy float64 restatement of the three rules of include/cfun_sample.h -- the per-slice nearest rotation, the GT
box with its 5 % expansion, and the RPN targets with the (key, index) subsampling contract.  Written from the rules, not copied
from the reference; tests/test_sample_ref.py holds it to the reference's recorded outputs (tests/golden/sample_targets.npz) and
to scipy's affine_transform, tests/sample_cases.py holds the kernels to it."""
import math

import numpy as np

NEG_IOU, POS_IOU = 0.3, 0.7


def cos_sin(angle):
    rad = math.radians(float(angle))
    return math.cos(rad), math.sin(rad)


def source_coords(h, w, angle):
    """(sy, sx) float64 [H,W]: where output pixel (y, x) samples the source; angle in degrees, None = identity."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if angle is None:
        return y, x
    c, s = cos_sin(angle)
    cy, cx = h / 2 - 0.5, w / 2 - 0.5
    dx, dy = x - cx, y - cy
    sx = c * dx + s * dy + cx
    sy = -s * dx + c * dy + cy
    return sy, sx


def source_index(h, w, angle):
    """(iy, ix, inside): the nearest source pixel of every output pixel and whether it lies inside the slice."""
    sy, sx = source_coords(h, w, angle)
    if angle is None:
        iy, ix = sy, sx
    else:
        iy, ix = np.floor(sy + 0.5), np.floor(sx + 0.5)
    inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    return np.where(inside, iy, 0).astype(np.int64), np.where(inside, ix, 0).astype(np.int64), inside


def rotate_slices(vol, angle):
    """[H,W,...] -> [H,W,...]: every [H,W] slice rotated by the rule, constant 0 outside (what an augmenter hands back)."""
    vol = np.asarray(vol)
    iy, ix, inside = source_index(vol.shape[0], vol.shape[1], angle)
    out = vol[iy, ix]
    out[~inside] = 0
    return out


def extract_box(labels_dhw):
    """(raw_box int32[6], empty): min and max + 1 over label > 0; zeros for a one-plane object and for an empty label."""
    idx = np.nonzero(np.asarray(labels_dhw) > 0)
    if idx[0].size == 0:
        return np.zeros(6, np.int32), 1
    lo = [int(i.min()) for i in idx]
    hi = [int(i.max()) for i in idx]
    if lo[0] == hi[0]:
        return np.zeros(6, np.int32), 0
    return np.array(lo + [v + 1 for v in hi], np.int32), 0


def expand_box(raw_box, dims_dhw):
    out = np.zeros(6, np.int32)
    for k in range(3):
        lo, hi = float(raw_box[k]), float(raw_box[k + 3])
        e = (hi - lo) * 0.05
        out[k] = int(math.floor(max(0.0, lo - e)))
        out[k + 3] = int(math.ceil(min(float(dims_dhw[k]), hi + e)))
    return out


def rotate_and_box(image_hwd, mask_hwd, angle):
    """-> (image [D,H,W] float32, labels [D,H,W] uint8, raw_box, box, empty)."""
    img = rotate_slices(np.asarray(image_hwd, np.float32), angle).transpose(2, 0, 1)
    lab = rotate_slices(np.asarray(mask_hwd, np.int32), angle).transpose(2, 0, 1).astype(np.uint8)
    raw, empty = extract_box(lab)
    return np.ascontiguousarray(img), np.ascontiguousarray(lab), raw, expand_box(raw, lab.shape), empty


def overlaps(anchors, gt_boxes):
    """[A,G] float64 IoU with + 1e-6 in the denominator."""
    a = np.asarray(anchors, np.float64).reshape(-1, 6)
    g = np.asarray(gt_boxes, np.float64).reshape(-1, 6)
    avol = (a[:, 3] - a[:, 0]) * (a[:, 4] - a[:, 1]) * (a[:, 5] - a[:, 2])
    out = np.zeros((a.shape[0], g.shape[0]))
    for j in range(g.shape[0]):
        gvol = (g[j, 3] - g[j, 0]) * (g[j, 4] - g[j, 1]) * (g[j, 5] - g[j, 2])
        z1, z2 = np.maximum(g[j, 0], a[:, 0]), np.minimum(g[j, 3], a[:, 3])
        y1, y2 = np.maximum(g[j, 1], a[:, 1]), np.minimum(g[j, 4], a[:, 4])
        x1, x2 = np.maximum(g[j, 2], a[:, 2]), np.minimum(g[j, 5], a[:, 5])
        inter = np.maximum(x2 - x1, 0) * np.maximum(y2 - y1, 0) * np.maximum(z2 - z1, 0)
        out[:, j] = inter / (gvol + avol - inter + 1e-6)
    return out


def _keep_smallest(match, cls, k, keys):
    ids = np.nonzero(match == cls)[0]
    if ids.size > k:
        order = ids[np.lexsort((ids, keys[ids]))]          # (key, index) ascending
        match[order[max(k, 0):]] = 0
        return max(k, 0)
    return int(ids.size)


def build_rpn_targets(anchors, gt_boxes, r, std_dev, keys):
    """-> (rpn_match int32 [A], rpn_bbox float64 [R,6], counts int32[2]).  ``keys``: uint32 per anchor."""
    a = np.asarray(anchors, np.float64).reshape(-1, 6)
    g = np.asarray(gt_boxes, np.float64).reshape(-1, 6)
    keys = np.asarray(keys).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    match = np.zeros(a.shape[0], np.int32)
    bbox = np.zeros((r, 6))
    if a.shape[0] == 0 or g.shape[0] == 0:
        return match, bbox, np.zeros(2, np.int32)
    ov = overlaps(a, g)
    arg = np.argmax(ov, axis=1)
    mx = ov[np.arange(a.shape[0]), arg]
    match[mx < NEG_IOU] = -1
    match[np.argmax(ov, axis=0)] = 1
    match[mx >= POS_IOU] = 1
    pos = _keep_smallest(match, 1, r // 2, keys)
    neg = _keep_smallest(match, -1, r - pos, keys)
    std = np.asarray(std_dev, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for row, i in enumerate(np.nonzero(match == 1)[0][:r]):
            gt = g[arg[i]]
            gs, as_ = gt[3:] - gt[:3], a[i, 3:] - a[i, :3]
            gc, ac = gt[:3] + 0.5 * gs, a[i, :3] + 0.5 * as_
            bbox[row] = np.concatenate([(gc - ac) / as_, np.log(gs / as_)]) / std
    return match, bbox, np.array([pos, neg], np.int32)


def ulp32_close(got, want64, ulps=2):
    """|got - want| <= ulps float32 ulp of the float64 golden (infinities must agree exactly)."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    fin = np.isfinite(want64)
    assert np.array_equal(got[~fin], want64[~fin])
    tol = ulps * np.spacing(np.abs(want64[fin]).astype(np.float32)).astype(np.float64)
    err = np.abs(got[fin] - want64[fin])
    assert (err <= tol).all(), "worst %g ulp32" % float((err / np.maximum(tol / ulps, 1e-300)).max())


def keys_from_drops(n, dropped):
    """Keys under which the (key, index) contract drops exactly ``dropped``: 1 for those, 0 for every other anchor."""
    keys = np.zeros(n, np.uint32)
    keys[np.asarray(dropped, np.int64)] = 1
    return keys


def load_image_gt(image_hwd, mask_hwd, angle, num_classes, anchors, r, std_dev, keys):
    """The sample dict of cfun_amd.sample.load_image_gt, as numpy (image before mold_image is ``image_raw``)."""
    img, lab, raw, box, empty = rotate_and_box(image_hwd, mask_hwd, angle)
    match, bbox, counts = build_rpn_targets(anchors, box[None].astype(np.float64), r, std_dev, keys)
    nfg = num_classes - 1
    return dict(image_raw=img, gt_labels=lab, raw_box=raw, box=box, empty=empty, gt_class_ids=np.arange(1, nfg + 1),
                gt_boxes=np.tile(box.astype(np.float32), (nfg, 1)), rpn_match=match.reshape(1, -1, 1),
                rpn_bbox_t=bbox.astype(np.float32)[None], rpn_counts=counts)
