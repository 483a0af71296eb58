"""TEST ONLY: numpy float64 restatement of the rule of include/cfun_sample_lits.h -- the LiTS fork's Dataset.__getitem__ up to
load_image_gt as one gather: frame index per axis (cfun_resize3d's order-0 rule), optional per-slice inverse affine map with
half-away-from-zero rounding, zero outside frame and source, the float32 clamp-normalisation, the uint8 label, the box.
Written from the header, not from the kernel; tests/test_sample_lits_ref.py holds it to the oracle's skimage_resize of the
explicitly built frame and to scipy's affine_transform, tests/sample_lits_cases.py holds the kernel to it."""
import math

import numpy as np

import sample_ref as sr


def offsets(frame, shape):
    """int((P - n) / 2.0) per axis, as the reference computes it: an odd difference puts the extra voxel on the high side."""
    return tuple(int((p - n) / 2.0) for p, n in zip(frame, shape))


def rotation_map(angle, frame_h, frame_w):
    t = math.radians(float(angle))
    c, s = math.cos(t), math.sin(t)
    cx, cy = frame_w / 2 - 0.5, frame_h / 2 - 0.5
    return (c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy)


def frame_index(m, p):
    """Step 1: floor((o + 0.5) * (P / m)) for o = 0 .. m-1, clamped to [0, P-1] -> int64 [m]."""
    k = np.floor((np.arange(m, dtype=np.float64) + 0.5) * (float(p) / float(m)))
    return np.clip(k, 0, p - 1).astype(np.int64)


def round_half_away(v):
    """(long long)(v > 0 ? v + 0.5 : v - 0.5): half away from zero, truncating."""
    return np.trunc(np.where(v > 0, v + 0.5, v - 0.5))


def frame_coords(frame, out_shape, amap):
    """Steps 1-2 before rounding: (row, col) float64 [H',W'] in frame coordinates."""
    fy = frame_index(out_shape[0], frame[0]).astype(np.float64)[:, None]
    fx = frame_index(out_shape[1], frame[1]).astype(np.float64)[None, :]
    if amap is None:
        return fy + 0 * fx, fx + 0 * fy
    m00, m01, m02, m10, m11, m12 = [np.float64(v) for v in amap]
    col = m00 * fx + m01 * fy + m02
    row = m10 * fx + m11 * fy + m12
    return row, col


def source_index(shape, frame, out_shape, amap, off=None):
    """Steps 1-4: (iy [H',W'], ix [H',W'], iz [D'], inside_yx [H',W'], inside_z [D']) into the [H,W,D] source.  ``off``: the
    source's position in the frame when it is not the reference's centring (the C entry takes any offset that fits)."""
    off = offsets(frame, shape) if off is None else off
    row, col = frame_coords(frame, out_shape, amap)
    if amap is not None:
        row, col = round_half_away(row), round_half_away(col)
    in_frame = (row >= 0) & (row < frame[0]) & (col >= 0) & (col < frame[1])
    iy, ix = row - off[0], col - off[1]
    inside = in_frame & (iy >= 0) & (iy < shape[0]) & (ix >= 0) & (ix < shape[1])
    iz = frame_index(out_shape[2], frame[2]) - off[2]
    inside_z = (iz >= 0) & (iz < shape[2])
    return (np.where(inside, iy, 0).astype(np.int64), np.where(inside, ix, 0).astype(np.int64), np.where(inside_z, iz, 0),
            inside, inside_z)


def normalise(v):
    """Step 5 in float32: two separately rounded operations, then the clamp that leaves a NaN a NaN."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        v = (v - np.float32(300.0)) / np.float32(-600.0)
        v = np.where(v > 1, np.float32(1), np.where(v < 0, np.float32(0), v))
    return v.astype(np.float32)


def gather(vol, idx):
    iy, ix, iz, inside, inside_z = idx
    out = vol[iy[:, :, None], ix[:, :, None], iz[None, None, :]]
    out[~(inside[:, :, None] & inside_z[None, None, :])] = 0
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def frame_rotate_resize(image_hwd, mask_hwd, frame, out_shape, angle=None, norm=True, amap=None, off=None):
    """-> (image [D',H',W'] float32, labels [D',H',W'] uint8, raw_box, box, empty)."""
    image = np.asarray(image_hwd, np.float32)
    mask = np.asarray(mask_hwd)
    if amap is None and angle is not None:
        amap = rotation_map(angle, frame[0], frame[1])
    idx = source_index(image.shape, frame, out_shape, amap, off)
    img = gather(normalise(image) if norm else image, idx)
    lab = gather((mask.astype(np.int64) & 255).astype(np.uint8), idx)
    raw, empty = sr.extract_box(lab)
    return img, lab, raw, sr.expand_box(raw, lab.shape), empty


def explicit_frame(vol, frame):
    """The zero frame the reference builds on the host, with the volume centred in it."""
    whole = np.zeros(frame, vol.dtype)
    o = offsets(frame, vol.shape)
    whole[o[0]:o[0] + vol.shape[0], o[1]:o[1] + vol.shape[1], o[2]:o[2] + vol.shape[2]] = vol
    return whole


def window(frame, shape, out_shape, min_dim, max_dim):
    """The fractional window of the fork's mold_inputs (LiTS_2017/model.py:1741-1761), for out_shape = (H', W', D')."""
    sx, sy, sz = offsets(frame, shape)
    h, w, d = out_shape
    ph, pw, pd = frame
    return (sz * d / pd, sx * h / ph, sy * w / pw, min_dim - sz * d / pd, max_dim - sx * h / ph, max_dim - sy * w / pw)


def make_sample(image_hwd, mask_hwd, angle, frame, out_shape, num_classes, anchors, r, std_dev, keys):
    """The sample dict of cfun_amd.sample.make_sample_lits, as numpy (the box and targets are sample_ref's)."""
    img, lab, raw, box, empty = frame_rotate_resize(image_hwd, mask_hwd, frame, out_shape, angle)
    match, bbox, counts = sr.build_rpn_targets(anchors, box[None].astype(np.float64), r, std_dev, keys)
    nfg = num_classes - 1
    return dict(image=img[None, None], gt_labels=lab, raw_box=raw, box=box, empty=empty, gt_class_ids=np.arange(1, nfg + 1),
                gt_boxes=np.tile(box.astype(np.float32), (nfg, 1)), rpn_match=match.reshape(1, -1, 1),
                rpn_bbox_t=bbox.astype(np.float32)[None], rpn_counts=counts)
