"""A training sample built on the device: the reference's ``load_image_gt`` (model.py:1007-1181; LiTS_2017/model.py:1010-1032).

    rotate_and_box      per-slice nearest rotation of image and label, [H,W,D] -> [D,H,W], uint8 labels, utils.extract_bboxes'
                        box and its 5 % expansion (model.py:1059-1075 / utils.extend_bbox)  -- cfun_sample_rotate_bbox
    build_rpn_targets   model.build_rpn_targets (model.py:1090-1181)                         -- cfun_sample_rpn_targets
    load_image_gt       both plus utils.mold_image and the class tiling: the dict ``train.train_epoch`` consumes
    make_sample         utils.resize_image / resize_mask (mode 'self') in front of load_image_gt
    frame_rotate_resize the LiTS fork's Dataset.__getitem__ (LiTS_2017/model.py:1145-1248) up to load_image_gt: clamp-normalise,
                        centre in the zero PAD_IMAGE_SHAPE frame, rotate per slice, nearest-resize to IMAGE_SHAPE, box -- one
                        gather pass, the frame never built                                  -- cfun_sample_lits
    make_sample_lits    frame_rotate_resize plus the RPN targets, window and image_meta: the fork's training sample
    draw_angle          the fork's integer rotation angle, drawn on the host as the fork draws it
    resize_rotate_box   the heart route from the LOADER's grid: utils.resize_image (order 1, clip, the cast back to an integer
                        loader dtype), utils.resize_mask (order 0), the rotation, the box and utils.mold_image's z-score as one
                        gather pass, a finish launch and a flat pass; neither resized volume built   -- cfun_sample_heart
    make_sample_heart   resize_rotate_box plus the RPN targets: make_sample's dict
    warp_and_box        elastic and affine augmentation of a network-size sample: a trilinear control-grid displacement, an
                        in-plane affine map and flips as one gather pass, and the warped labels' box   -- cfun_sample_warp
    Warp / draw_warp / affine_map   the holder of one warp, its host-side draw, and the six doubles of an in-plane map;
                        ``augment=Warp`` on make_sample, make_sample_heart and make_sample_lits places the warp after the route

Nothing on this path waits for the device: box, tiling and counts stay device tensors.  Only ``strict=True`` reads back (the
empty flag and the label range) and raises where the reference would.

Two departures from the reference, both deliberate:
  * its two ``np.random.choice`` draws are a deterministic contract here: among the positives the ``R // 2`` smallest in
    (key, anchor index) order stay, among the negatives the ``R - positives_kept`` smallest; ``keys`` are uint32 per anchor
    (``None``: drawn with torch.randint on the device);
  * an empty label volume gives zero boxes and ``empty == 1`` instead of an exception.
Not pinned by the reference: the rotation against imgaug's ``iaa.Affine(rotate, order=0)`` -- imgaug and its backends are not
available to this project's environments.  The rule (cfun_sample.h) follows imgaug's documented construction: centre
``size / 2 - 0.5``, nearest sample, constant 0 outside; exact half-voxel ties and cv2's fixed-point coordinates may differ by one
voxel along edges.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, utils
from ._lib import check, ptr, stream, workspace
from .ops import ptr_raw

NEG_IOU, POS_IOU = 0.3, 0.7          # model.py:1119,1126


def _volume(image):
    if image.dim() == 4 and image.shape[3] == 1:
        image = image[..., 0]
    if image.dim() != 3:
        raise ValueError("sample: [H,W,D] (or [H,W,D,1]) volume expected, got %s" % (tuple(image.shape),))
    return image


def rotate_and_box(image, mask, angle, strict=False):
    """image float32 / mask integer, both [H,W,D] with any strides (the loader's arrays, read in place), ``angle`` in degrees or
    ``None`` (no rotation: the LiTS form, bit-identical to angle 0).  Returns (image [D,H,W] float32, labels [D,H,W] uint8,
    raw_box int32[6], box int32[6], empty int32[1]) on the device.  Preconditions: equal shapes; label values in [0, 255]
    (the range is verified only with ``strict``, which reads back)."""
    lib = _lib.load()
    image, mask = _volume(image), _volume(mask)
    if tuple(image.shape) != tuple(mask.shape):
        raise ValueError("rotate_and_box: image %s and mask %s differ in shape" % (tuple(image.shape), tuple(mask.shape)))
    if image.device != mask.device:
        raise ValueError("rotate_and_box: image and mask sit on different devices")
    if mask.dtype.is_floating_point or mask.dtype == torch.bool:
        raise ValueError("rotate_and_box: integer label volume expected, got %s" % (mask.dtype,))
    if image.dtype != torch.float32:
        image = image.to(torch.float32)
    if mask.dtype != torch.int32:
        mask = mask.to(torch.int32)
    h, w, d = [int(v) for v in image.shape]
    if min(h, w, d) <= 0 or h > 65535:
        raise ValueError("rotate_and_box: unsupported extent %s" % ((h, w, d),))
    if strict:
        lo, hi = torch.aminmax(mask)
        if int(lo) < 0 or int(hi) > 255:
            raise ValueError("rotate_and_box: label values must lie in [0, 255], got [%d, %d]" % (int(lo), int(hi)))
    rotate = angle is not None
    rad = math.radians(float(angle)) if rotate else 0.0
    ws = workspace(lib.cfun_sample_workspace_bytes(h, w, d, 0, 0), image)
    out = torch.empty((d, h, w), dtype=torch.float32, device=image.device)
    labels = torch.empty((d, h, w), dtype=torch.uint8, device=image.device)
    small = torch.empty(16, dtype=torch.int32, device=image.device)
    raw_box, box, empty = small[0:6], small[6:12], small[12:13]
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    check(lib.cfun_sample_rotate_bbox(ptr_raw(image), i64(*image.stride()), ptr_raw(mask), i64(*mask.stride()), i32(h, w, d),
                                      math.cos(rad), math.sin(rad), int(rotate), ptr(out), ptr(labels), ptr(raw_box), ptr(box),
                                      ptr(empty), ptr(ws), ws.numel(), stream(image)), "sample_rotate_bbox")
    if strict and int(empty):
        raise ValueError("rotate_and_box: the label volume is empty (the reference's extract_bboxes raises here as well)")
    return out, labels, raw_box, box, empty


def build_rpn_targets(anchors, gt_boxes, config, keys=None):
    """anchors [A,6] float32 on the device, gt_boxes [G,6] (same units) -> (rpn_match int32 [1,A,1], rpn_bbox float32 [1,R,6],
    counts int32[2] = positives kept, negatives kept).  ``keys``: integer tensor [A] whose low 32 bits order the subsampling."""
    lib = _lib.load()
    if anchors.dim() != 2 or anchors.shape[1] != 6 or gt_boxes.dim() != 2 or gt_boxes.shape[1] != 6:
        raise ValueError("build_rpn_targets: [A,6] anchors and [G,6] boxes expected")
    a, g, r = int(anchors.shape[0]), int(gt_boxes.shape[0]), int(config.RPN_TRAIN_ANCHORS_PER_IMAGE)
    dev = anchors.device
    anchors = anchors.to(torch.float32).contiguous()
    gt = gt_boxes.to(device=dev, dtype=torch.float32).contiguous()
    if keys is None:
        keys = torch.randint(0, 1 << 32, (a,), dtype=torch.int64, device=dev)
    if keys.numel() != a or keys.dtype.is_floating_point:
        raise ValueError("build_rpn_targets: one integer key per anchor expected")
    keys = keys.to(device=dev).reshape(a).to(torch.int64).bitwise_and(0xFFFFFFFF).to(torch.int32).contiguous()   # the uint32's bits
    std = (C.c_double * 6)(*[float(v) for v in config.RPN_BBOX_STD_DEV])
    empty_call = a == 0 or g == 0
    ws = workspace(lib.cfun_sample_workspace_bytes(0, 0, 0, a, g), anchors)
    make = torch.zeros if empty_call else torch.empty          # (a zero-size call launches nothing and writes nothing)
    rpn_match = make((1, a, 1), dtype=torch.int32, device=dev)
    rpn_bbox = make((1, r, 6), dtype=torch.float32, device=dev)
    counts = make(2, dtype=torch.int32, device=dev)
    check(lib.cfun_sample_rpn_targets(ptr(anchors), a, ptr(gt), g, ptr(keys), r, std, NEG_IOU, POS_IOU, ptr(rpn_match),
                                      ptr(rpn_bbox), ptr(counts), ptr(ws), ws.numel(), stream(anchors)), "sample_rpn_targets")
    return rpn_match, rpn_bbox, counts


def load_image_gt(image, mask, angle, config, anchors, keys=None, strict=False, augment=None):
    """model.load_image_gt on the device.  image / mask: the network-size [H,W,D] (or [H,W,D,1]) volumes; ``angle`` in degrees,
    ``None`` = the LiTS form (no rotation).  Returns the dict ``train.train_epoch`` consumes -- ``image`` [1,1,D,H,W] after
    utils.mold_image, ``gt_class_ids`` 1 .. NUM_CLASSES-1, ``gt_boxes`` the expanded box tiled NUM_CLASSES-1 times (float32
    voxels, as step.training_step_full takes them), ``gt_labels`` uint8 [D,H,W], ``rpn_match`` [1,A,1], ``rpn_bbox_t`` [1,R,6] --
    plus ``raw_box``, ``empty`` and ``rpn_counts``.  ``augment``: a ``Warp`` applied to the rotated sample before mold_image; box
    and targets are then the warped labels'."""
    img, labels, raw_box, box, empty = rotate_and_box(image, mask, angle, strict=strict)
    if augment is not None:
        img, labels, raw_box, box, empty = warp_and_box(img, labels, augment)
    dev = img.device
    nfg = int(config.NUM_CLASSES) - 1
    boxf = box.to(torch.float32)[None]
    rpn_match, rpn_bbox, counts = build_rpn_targets(anchors.to(dev), boxf, config, keys)
    return dict(image=utils.mold_image(img)[None, None], gt_class_ids=torch.arange(1, nfg + 1, device=dev),
                gt_boxes=boxf.repeat(nfg, 1), gt_labels=labels, rpn_match=rpn_match, rpn_bbox_t=rpn_bbox,
                raw_box=raw_box, empty=empty, rpn_counts=counts)


def make_sample(image_hwd, mask_hwd, angle, config, anchors, keys=None, strict=False, augment=None):
    """The loader's [H,W,D] image and label volumes (numpy or tensors, any size) -> a training sample: utils.resize_image /
    resize_mask (mode 'self') to the network size, then load_image_gt (``augment``: its ``Warp``)."""
    dev = anchors.device
    image = _volume(torch.as_tensor(image_hwd).to(dev))
    mask = _volume(torch.as_tensor(mask_hwd).to(dev))
    mx, mn = int(config.IMAGE_MAX_DIM), int(config.IMAGE_MIN_DIM)
    image = utils.resize_image(image[..., None].to(torch.float32), min_dim=mn, max_dim=mx, mode="self", device=dev)[0]
    mask = utils.resize_mask(mask, None, None, max_dim=mx, min_dim=mn, mode="self", device=dev)
    return load_image_gt(image, mask, angle, config, anchors, keys=keys, strict=strict, augment=augment)


# ------------------------------------------------------------------------------------------- the heart sample in one pass
_HEART_ELEM = {torch.int16: _lib.ELEM_INT16, torch.float32: _lib.ELEM_FLOAT32, torch.float64: _lib.ELEM_FLOAT64}
_HEART_LABEL = {torch.int8: _lib.LABEL_INT8, torch.uint8: _lib.LABEL_UINT8, torch.int16: _lib.LABEL_INT16, torch.int32: _lib.LABEL_INT32}


def resize_rotate_box(image, mask, out_shape, angle, zscore=True, strict=False, truncate=None, clip=True):
    """image [H,W,D] in the loader's dtype and memory order (int16, float32 and float64 are read in place through their strides;
    anything else is cast to float64 on the device first), mask an integer [H,W,D] volume or ``None`` (int8, uint8, int16 and
    int32 are read in place, other integers cast to int32), ``out_shape`` (H', W', D'), ``angle`` in degrees or ``None`` (no
    rotation, bit-identical to angle 0).  The rule is include/cfun_sample_heart.h's: skimage's order-1 resize with its clip to
    the source's range (``clip``; the bounds come from a device-side aminmax, nothing reads back), the reference's cast back to
    an integer loader dtype (``truncate``; ``None``: exactly when ``image``'s dtype is an integer), the float32 cast, the
    rotation in the resized grid, the order-0 label, the box, and with ``zscore`` utils.mold_image.  Returns (image [D',H',W']
    float32, labels [D',H',W'] uint8, raw_box int32[6], box int32[6], empty int32[1], stats float64[2] = mean, std) on the
    device; labels, boxes and flag are ``None`` without a mask, stats without ``zscore``."""
    lib = _lib.load()
    image = _volume(image)
    integer = not (image.dtype.is_floating_point or image.dtype.is_complex)
    if image.dtype not in _HEART_ELEM:
        image = image.to(torch.float64)
    if mask is not None:
        mask = _volume(mask)
        if tuple(image.shape) != tuple(mask.shape):
            raise ValueError("resize_rotate_box: image %s and mask %s differ in shape" % (tuple(image.shape), tuple(mask.shape)))
        if image.device != mask.device:
            raise ValueError("resize_rotate_box: image and mask sit on different devices")
        if mask.dtype.is_floating_point or mask.dtype == torch.bool:
            raise ValueError("resize_rotate_box: integer label volume expected, got %s" % (mask.dtype,))
        if mask.dtype not in _HEART_LABEL:
            mask = mask.to(torch.int32)
    n = [int(v) for v in image.shape]
    m = [int(v) for v in out_shape]
    if len(m) != 3 or min(n + m) <= 0 or m[0] > 65535:
        raise ValueError("resize_rotate_box: unsupported extents: source %s, output %s" % (n, m))
    if strict and mask is not None:
        lo, hi = torch.aminmax(mask)
        if int(lo) < 0 or int(hi) > 255:
            raise ValueError("resize_rotate_box: label values must lie in [0, 255], got [%d, %d]" % (int(lo), int(hi)))
    dev = image.device
    bounds = None
    if clip:
        lo, hi = torch.aminmax(image)
        bounds = torch.stack([lo, hi]).to(torch.float64).contiguous()        # scikit-image's clip=True: the source's own range
    rotate = angle is not None
    rad = math.radians(float(angle)) if rotate else 0.0
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    ws = workspace(lib.cfun_sample_heart_workspace_bytes(i32(*m)), image)
    out = torch.empty((m[2], m[0], m[1]), dtype=torch.float32, device=dev)
    labels = raw_box = box = empty = None
    if mask is not None:
        labels = torch.empty((m[2], m[0], m[1]), dtype=torch.uint8, device=dev)
        small = torch.empty(16, dtype=torch.int32, device=dev)
        raw_box, box, empty = small[0:6], small[6:12], small[12:13]
    stats = torch.empty(2, dtype=torch.float64, device=dev) if zscore else None
    check(lib.cfun_sample_heart(ptr_raw(image), i64(*image.stride()), _HEART_ELEM[image.dtype],
                                ptr_raw(mask) if mask is not None else None, i64(*mask.stride()) if mask is not None else None,
                                _HEART_LABEL[mask.dtype] if mask is not None else 0, i32(*n), i32(*m), ptr(bounds),
                                int(integer if truncate is None else bool(truncate)), math.cos(rad), math.sin(rad), int(rotate),
                                int(bool(zscore)), ptr(out), ptr(labels), ptr(raw_box), ptr(box), ptr(empty), ptr(stats), ptr(ws),
                                ws.numel(), stream(image)), "sample_heart")
    if strict and mask is not None and int(empty):
        raise ValueError("resize_rotate_box: the label volume is empty (the reference's extract_bboxes raises here as well)")
    return out, labels, raw_box, box, empty, stats


def make_sample_heart(image_hwd, mask_hwd, angle, config, anchors, keys=None, strict=False, augment=None):
    """``make_sample`` in one pass: the loader's [H,W,D] image and label volumes (numpy or tensors, any size, their own dtype and
    memory order) -> the dict ``train.train_epoch`` consumes, with load_image_gt's keys plus ``stats`` (mean, std of the z-score).
    One difference from ``make_sample``, stated by the rule: an integer image is cast back to its dtype after the resize, as the
    reference's resize_image and ``utils.mold_inputs`` do (``make_sample`` converts to float32 first and skips that cast).
    ``augment``: a ``Warp``; the pass then runs without its z-score, the warp follows, and utils.mold_image normalises the warped
    image (``stats`` are its mean and population std)."""
    dev = anchors.device
    image = _volume(torch.as_tensor(image_hwd)).to(dev)
    mask = _volume(torch.as_tensor(mask_hwd)).to(dev)
    mx, mn = int(config.IMAGE_MAX_DIM), int(config.IMAGE_MIN_DIM)
    if augment is None:
        img, labels, raw_box, box, empty, stats = resize_rotate_box(image, mask, (mx, mx, mn), angle, zscore=True, strict=strict)
    else:
        img, labels, _, _, _, _ = resize_rotate_box(image, mask, (mx, mx, mn), angle, zscore=False, strict=strict)
        img, labels, raw_box, box, empty = warp_and_box(img, labels, augment)
        stats = torch.stack([img.mean(), img.std(unbiased=False)]).to(torch.float64)
        img = utils.mold_image(img)
    nfg = int(config.NUM_CLASSES) - 1
    boxf = box.to(torch.float32)[None]
    rpn_match, rpn_bbox, counts = build_rpn_targets(anchors.to(dev), boxf, config, keys)
    return dict(image=img[None, None], gt_class_ids=torch.arange(1, nfg + 1, device=dev), gt_boxes=boxf.repeat(nfg, 1),
                gt_labels=labels, rpn_match=rpn_match, rpn_bbox_t=rpn_bbox, raw_box=raw_box, empty=empty, rpn_counts=counts,
                stats=stats)


# ------------------------------------------------------------------------------------------------------ the LiTS fork's sample
def rotation_map(angle, frame_h, frame_w):
    """The six doubles (m00 m01 m02 m10 m11 m12) of cfun_sample_lits.h for a rotation by ``angle`` degrees about the centre of a
    [frame_h, frame_w] slice: skimage.transform.rotate's translate(centre) . rotate . translate(-centre), used as the inverse map
    (rows = H, cols = W)."""
    t = math.radians(float(angle))
    c, s = math.cos(t), math.sin(t)
    cx, cy = frame_w / 2 - 0.5, frame_h / 2 - 0.5
    return (c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy)


def frame_rotate_resize(image, mask, frame, out_shape, angle=None, normalise=True, strict=False):
    """image float32 / mask int8, uint8 or int32, both [H,W,D] with any strides (the loader's arrays, read in place; no conversion
    pass over the label).  The pair is centred in a virtual zero ``frame`` (PH, PW, PD) -- offset ``int((P - n) / 2.0)`` per axis
    as the reference computes it --, every [PH,PW] slice is rotated by the integer or float ``angle`` in degrees (``None``: no map,
    the fork's validation form; bit-identical to angle 0), and the frame is nearest-resized to ``out_shape`` (H', W', D').
    ``normalise``: the fork's preprocess_image on the source values, (x - 300) / (-600) clamped to [0, 1] with IEEE float32
    operations (cfun_sample_lits.h step 5: utils.preprocess_image_lits on the host, within 1 ulp of it on the device, where
    torch multiplies by the reciprocal); the frame's zeros stay zeros.  Returns (image [D',H',W']
    float32, labels [D',H',W'] uint8, raw_box int32[6], box int32[6], empty int32[1]) on the device.  Preconditions: equal shapes,
    a source that fits the frame, label values in [0, 255] (the range is verified only with ``strict``, which reads back)."""
    lib = _lib.load()
    image, mask = _volume(image), _volume(mask)
    if tuple(image.shape) != tuple(mask.shape):
        raise ValueError("frame_rotate_resize: image %s and mask %s differ in shape" % (tuple(image.shape), tuple(mask.shape)))
    if image.device != mask.device:
        raise ValueError("frame_rotate_resize: image and mask sit on different devices")
    if mask.dtype not in (torch.int8, torch.uint8, torch.int32):
        raise ValueError("frame_rotate_resize: int8, uint8 or int32 label volume expected, got %s" % (mask.dtype,))
    if image.dtype != torch.float32:
        image = image.to(torch.float32)
    n = [int(v) for v in image.shape]
    frame = [int(v) for v in frame]
    m = [int(v) for v in out_shape]
    if len(frame) != 3 or len(m) != 3 or min(n + frame + m) <= 0 or m[0] > 65535:
        raise ValueError("frame_rotate_resize: unsupported extents: source %s, frame %s, output %s" % (n, frame, m))
    if any(k > p for k, p in zip(n, frame)):
        raise ValueError("frame_rotate_resize: the source %s does not fit the frame %s" % (n, frame))
    off = [int((p - k) / 2.0) for p, k in zip(frame, n)]
    if strict:
        lo, hi = torch.aminmax(mask)
        if int(lo) < 0 or int(hi) > 255:
            raise ValueError("frame_rotate_resize: label values must lie in [0, 255], got [%d, %d]" % (int(lo), int(hi)))
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    ws = workspace(lib.cfun_sample_lits_workspace_bytes(i32(*m)), image)
    out = torch.empty((m[2], m[0], m[1]), dtype=torch.float32, device=image.device)
    labels = torch.empty((m[2], m[0], m[1]), dtype=torch.uint8, device=image.device)
    small = torch.empty(16, dtype=torch.int32, device=image.device)
    raw_box, box, empty = small[0:6], small[6:12], small[12:13]
    amap = (C.c_double * 6)(*rotation_map(angle, frame[0], frame[1])) if angle is not None else None
    check(lib.cfun_sample_lits(ptr_raw(image), i64(*image.stride()), ptr_raw(mask), i64(*mask.stride()), mask.element_size(),
                               i32(*n), i32(*frame), i32(*off), i32(*m), amap, int(bool(normalise)), ptr(out), ptr(labels),
                               ptr(raw_box), ptr(box), ptr(empty), ptr(ws), ws.numel(), stream(image)), "sample_lits")
    if strict and int(empty):
        raise ValueError("frame_rotate_resize: the label volume is empty (the reference's extract_bboxes raises here as well)")
    return out, labels, raw_box, box, empty


def draw_angle(config, generator=None):
    """The fork's per-sample rotation angle: an int in [ROTATE_ANGLE[0], ROTATE_ANGLE[1]), drawn on the host with
    ``torch.randint`` as the fork draws it (LiTS_2017/model.py:1213); ``generator``: a CPU torch.Generator to draw from."""
    lo, hi = [int(v) for v in config.ROTATE_ANGLE]
    return int(torch.randint(lo, hi, (1,), generator=generator))


def make_sample_lits(image_hwd, mask_hwd, angle, config, anchors, keys=None, strict=False, augment=None):
    """The LiTS fork's training sample (Dataset.__getitem__, LiTS_2017/model.py:1145-1248) from the loader's raw [H,W,D] arrays
    (numpy or tensors): the CT in HU, the label as int8 (what the fork stores), uint8 or int32.  ``angle``: degrees (the fork:
    ``draw_angle(config)`` when ``config.AUGMENTATION``), ``None`` = the fork's validation form (``augmentation=False``).
    Returns the dict ``train.train_epoch`` consumes, with load_image_gt's keys, plus ``window`` and ``image_meta`` as
    utils.mold_inputs_lits computes them.  ``image`` [1,1,D',H',W'] is the clamp-normalised volume WITHOUT utils.mold_image:
    the fork never z-scores its input (its mold_inputs does not either).  ``augment``: a ``Warp`` applied to the resized sample;
    box and targets are then the warped labels'."""
    dev = anchors.device
    image = _volume(torch.as_tensor(image_hwd).to(dev))
    mask = _volume(torch.as_tensor(mask_hwd).to(dev))
    frame = [int(v) for v in config.PAD_IMAGE_SHAPE]
    h, w, d = [int(v) for v in config.IMAGE_SHAPE[:3]]
    img, labels, raw_box, box, empty = frame_rotate_resize(image, mask, frame, (h, w, d), angle=angle, normalise=True, strict=strict)
    if augment is not None:
        img, labels, raw_box, box, empty = warp_and_box(img, labels, augment)
    nfg = int(config.NUM_CLASSES) - 1
    boxf = box.to(torch.float32)[None]
    rpn_match, rpn_bbox, counts = build_rpn_targets(anchors, boxf, config, keys)
    sx, sy, sz = [int((p - k) / 2.0) for p, k in zip(frame, image.shape)]
    ph, pw, pd = frame
    window = (sz * d / pd, sx * h / ph, sy * w / pw, config.IMAGE_MIN_DIM - sz * d / pd, config.IMAGE_MAX_DIM - sx * h / ph,
              config.IMAGE_MAX_DIM - sy * w / pw)
    meta = utils.compose_image_meta(0, (h, w, d), window, np.zeros([config.NUM_CLASSES], dtype=np.int32))
    return dict(image=img[None, None], gt_class_ids=torch.arange(1, nfg + 1, device=dev), gt_boxes=boxf.repeat(nfg, 1),
                gt_labels=labels, rpn_match=rpn_match, rpn_bbox_t=rpn_bbox, raw_box=raw_box, empty=empty, rpn_counts=counts,
                window=window, image_meta=meta)


# ---------------------------------------------------------------------------------- elastic and affine augmentation: one warp
class Warp:
    """One warp of include/cfun_sample_warp.h, a plain holder.  ``grid``: float32 [3,gz,gy,gx] displacements in voxels (z, y, x
    components; a tensor or a numpy array) or ``None``; ``map``: six doubles (``affine_map``) or ``None``; ``flips``: one bool
    per axis (z, y, x); ``image_order`` 0 or 1 (the labels are always nearest).  ``factor``: what ``draw_warp`` scaled the drawn
    grid by to keep the map one-to-one (1.0: nothing)."""

    def __init__(self, grid=None, map=None, flips=(False, False, False), image_order=1, factor=1.0):
        self.grid, self.map, self.flips, self.image_order, self.factor = grid, map, tuple(bool(f) for f in flips), int(image_order), factor

    def __repr__(self):
        g = None if self.grid is None else tuple(self.grid.shape)
        return "Warp(grid=%s, map=%s, flips=%s, image_order=%d, factor=%r)" % (g, self.map, self.flips, self.image_order, self.factor)


def affine_map(angle, h, w, scale=(1, 1), translate=(0, 0)):
    """The six doubles of the INVERSE in-plane map (cfun_sample_lits.h's convention: col = m0 x + m1 y + m2, row = m3 x + m4 y +
    m5) of: zoom by ``scale`` = (sy, sx) about the centre of an [h, w] slice, rotate by ``angle`` degrees about it, move by
    ``translate`` = (ty, tx) voxels.  With the defaults it equals ``rotation_map(angle, h, w)`` exactly."""
    t = math.radians(float(angle))
    c, s = math.cos(t), math.sin(t)
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    sy, sx = float(scale[0]), float(scale[1])
    ty, tx = float(translate[0]), float(translate[1])
    m0, m1, m3, m4 = c / sx, -s / sy, s / sx, c / sy
    return (m0, m1, cx - m0 * (cx + tx) - m1 * (cy + ty), m3, m4, cy - m3 * (cx + tx) - m4 * (cy + ty))


def _fold_ratio(grid, shape_dhw):
    """max over the components c of |difference of neighbouring control values along axis c| / (half a cell along c, in voxels)."""
    worst = 0.0
    for c in range(3):
        n, g = int(shape_dhw[c]), int(grid.shape[1 + c])
        if n == 1:
            continue               # (only control plane 0 acts along an axis of extent 1: nothing can fold)
        half = 0.5 * (n - 1) / (g - 1)
        worst = max(worst, float(grid[c].to(torch.float64).diff(dim=c).abs().max()) / half)
    return worst


def draw_warp(shape_dhw, generator=None, grid=(5, 5, 5), sigma=(2.0, 4.0, 4.0), angle=None, scale_range=None, flip_p=(0, 0, 0),
              image_order=1):
    """Draw one ``Warp`` for a [D,H,W] sample on the host, from the CPU torch.Generator ``generator`` (as ``draw_angle`` draws):
    control values ~ N(0, sigma_c) voxels per component (``sigma``: a number or one per z, y, x), an angle uniform in
    ``angle`` = (lo, hi) degrees (a number: that angle; ``None``: no rotation), a zoom per in-plane axis uniform in
    ``scale_range`` = (lo, hi), a flip per axis with probability ``flip_p``.  The draws are made in this order, all of them
    always, so one generator state gives one Warp whatever the switches.
    The map stays one-to-one along each component's own axis: where two neighbouring control values of component c differ by more
    than half a control cell along axis c, (n_c - 1) / (g_c - 1) / 2 voxels, the whole grid is scaled down until the float32
    values meet the bound; ``Warp.factor`` is that factor."""
    shape_dhw = tuple(int(v) for v in shape_dhw)
    g = tuple(int(v) for v in grid)
    if len(shape_dhw) != 3 or min(shape_dhw) <= 0 or len(g) != 3 or min(g) < 2:
        raise ValueError("draw_warp: a positive [D,H,W] shape and a control grid of at least 2 points per axis expected")
    sig = torch.tensor([float(sigma)] * 3 if np.isscalar(sigma) else [float(v) for v in sigma], dtype=torch.float64)
    field = torch.randn((3,) + g, generator=generator, dtype=torch.float64) * sig[:, None, None, None]
    u = [float(v) for v in torch.rand(6, generator=generator, dtype=torch.float64)]      # (host tensors: nothing reads a device back)
    factor, values = 1.0, field.to(torch.float32)
    for _ in range(8):
        r = _fold_ratio(values, shape_dhw)
        if r <= 1.0:
            break
        factor = factor / r * (1.0 - 2.0 ** -20)
        values = (field * factor).to(torch.float32)
    else:
        raise RuntimeError("draw_warp: the control grid could not be scaled under the half-cell bound")
    amap = None
    if angle is not None or scale_range is not None:
        if angle is None:
            a = 0.0
        elif np.isscalar(angle):
            a = float(angle)
        else:
            a = float(angle[0]) + u[0] * (float(angle[1]) - float(angle[0]))
        sc = (1.0, 1.0)
        if scale_range is not None:
            lo, hi = float(scale_range[0]), float(scale_range[1])
            sc = (lo + u[1] * (hi - lo), lo + u[2] * (hi - lo))
        amap = affine_map(a, shape_dhw[1], shape_dhw[2], scale=sc)
    flips = tuple(u[3 + k] < float(flip_p[k]) for k in range(3))
    return Warp(values, amap, flips, image_order, factor)


def warp_and_box(image_dhw, labels_dhw, warp):
    """image float32 [D,H,W], labels uint8 [D,H,W] on the device (what every sample route yields before utils.mold_image), ``warp``
    a ``Warp``.  The rule is include/cfun_sample_warp.h's.  Returns (image [D,H,W] float32, labels [D,H,W] uint8, raw_box
    int32[6], box int32[6], empty int32[1]) on the device; nothing waits for it."""
    lib = _lib.load()
    if image_dhw.dim() != 3 or tuple(image_dhw.shape) != tuple(labels_dhw.shape):
        raise ValueError("warp_and_box: [D,H,W] image and labels of one shape expected, got %s and %s"
                         % (tuple(image_dhw.shape), tuple(labels_dhw.shape)))
    if image_dhw.device != labels_dhw.device:
        raise ValueError("warp_and_box: image and labels sit on different devices")
    if labels_dhw.dtype != torch.uint8:
        raise ValueError("warp_and_box: uint8 labels expected, got %s" % (labels_dhw.dtype,))
    dev = image_dhw.device
    image = image_dhw.to(torch.float32).contiguous()
    labels = labels_dhw.contiguous()
    n = [int(v) for v in image.shape]
    if min(n) <= 0 or n[0] * n[1] * n[2] >= 1 << 31:
        raise ValueError("warp_and_box: unsupported extent %s" % (n,))
    i32 = C.c_int32 * 3
    grid = gdims = None
    if warp.grid is not None:
        grid = torch.as_tensor(warp.grid).to(device=dev, dtype=torch.float32).contiguous()
        top = int(lib.cfun_sample_warp_max_grid())
        if grid.dim() != 4 or grid.shape[0] != 3 or min(grid.shape[1:]) < 2 or max(grid.shape[1:]) > top:
            raise ValueError("warp_and_box: a [3,gz,gy,gx] control grid with 2 .. %d points per axis expected, got %s"
                             % (top, tuple(grid.shape)))
        gdims = i32(*[int(v) for v in grid.shape[1:]])
    if warp.image_order not in (0, 1):
        raise ValueError("warp_and_box: image_order 0 or 1 expected, got %r" % (warp.image_order,))
    amap = (C.c_double * 6)(*[float(v) for v in warp.map]) if warp.map is not None else None
    flips = sum(1 << k for k in range(3) if warp.flips[k])
    ws = workspace(lib.cfun_sample_warp_workspace_bytes(i32(*n)), image)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    out_labels = torch.empty(n, dtype=torch.uint8, device=dev)
    small = torch.empty(16, dtype=torch.int32, device=dev)
    raw_box, box, empty = small[0:6], small[6:12], small[12:13]
    check(lib.cfun_sample_warp(ptr(image), ptr(labels), i32(*n), ptr(grid), gdims, amap, flips, warp.image_order, ptr(out),
                               ptr(out_labels), ptr(raw_box), ptr(box), ptr(empty), ptr(ws), ws.numel(), stream(image)),
          "sample_warp")
    return out, out_labels, raw_box, box, empty
