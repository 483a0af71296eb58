"""TEST ONLY: numpy float64 restatement of the rule of include/cfun_sample_heart.h -- the order-1 resize with its clip, the cast
back to an integer loader dtype, the float32 cast, the rotation in the resized grid, the order-0 label, the box and the z-score.
Written from the header, not from the kernel.  Steps the header takes over from cfun_native.h and cfun_sample.h are taken over
from their restatements (native_ref: steps 3-5 and the order-0 index; sample_ref: the rotation's source index and the box).
tests/test_sample_heart_ref.py holds it to oracle.cfun_oracle.skimage_resize and to sample_ref's rotation bit for bit,
tests/sample_heart_cases.py holds the kernels to it."""
import numpy as np

import native_ref as nr
import sample_ref as sr


def resized_image(src, out_shape, clip="range", truncate=False, planes=None):
    """Steps 2-4 on the whole resized grid (or only its z ``planes``): float32 [H',W',len(planes)]."""
    src = np.asarray(src)
    if isinstance(clip, str):
        clip = (np.float64(src.min()), np.float64(src.max()))
    zs = np.arange(out_shape[2]) if planes is None else np.asarray(planes)
    t = nr.clip_range(nr.blend(src, np.arange(out_shape[0]), np.arange(out_shape[1]), zs, out_shape), clip)
    if truncate:
        t = np.trunc(t) + 0.0                                                 # step 3: no negative zero; a NaN stays a NaN
    with np.errstate(invalid="ignore", over="ignore"):
        return t.astype(np.float32)                                           # step 4: round to nearest even


def resized_label(mask, out_shape, planes=None):
    """Step 5 on the whole resized grid: the value READ, in the mask's own dtype."""
    mask = np.asarray(mask)
    zs = np.arange(out_shape[2]) if planes is None else np.asarray(planes)
    idx = [nr.frame_index(m, n) for m, n in zip(out_shape, mask.shape)]
    return mask[idx[0][:, None, None], idx[1][None, :, None], idx[2][zs][None, None, :]]


def zscore(s):
    """Step 7 in float64 with numpy's own sums: (stats float64[2], z64 float64, float32 of it)."""
    s64 = np.asarray(s, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s64.sum() / s64.size
        var = (s64 * s64).sum() / s64.size - mean * mean
        std = np.sqrt(var)
        z = (s64 - mean) / std
        return np.array([mean, std]), z, z.astype(np.float32)


def sample_heart(src, mask, out_shape, angle=None, clip="range", truncate=False, planes=None):
    """The rule without the z-score -> (image float32 [D',H',W'], labels uint8 [D',H',W'], raw_box, box, empty); labels, boxes and
    flag are None without a mask.  ``planes``: only these output z (the boxes are then those of the planes: not the kernel's)."""
    h, w = int(out_shape[0]), int(out_shape[1])
    iy, ix, inside = sr.source_index(h, w, angle)                             # step 1
    vol = resized_image(src, out_shape, clip, truncate, planes)
    img = vol[iy, ix]
    img[~inside] = 0
    img = np.ascontiguousarray(img.transpose(2, 0, 1))
    if mask is None:
        return img, None, None, None, None
    read = resized_label(mask, out_shape, planes)[iy, ix]
    read[~inside] = 0
    read = read.transpose(2, 0, 1)
    lab = np.ascontiguousarray((read.astype(np.int64) & 255).astype(np.uint8))          # the low 8 bits are stored
    raw, empty = sr.extract_box(read.astype(np.int64))                        # the box counts label > 0 on the value read
    return img, lab, raw, sr.expand_box(raw, lab.shape), empty
