"""LiTS from the scanner's grid: the step in front of the network and the step behind it, on the device.

    diag_spacing        preprocessing.get_spacing (LiTS_2017/preprocessing.py:10-13): |diagonal| of the affine
    resampled_shape     the shape preprocessing.py resamples a volume to (:28)
    mold_inputs_native  preprocessing.py's order-1 resample to MEAN_SPACING, its float32 cast, and the fork's mold_inputs
                        (LiTS_2017/model.py:1730-1775) as ONE gather from the volume as the NIfTI file holds it: neither the
                        resampled volume nor the frame is built                              -- cfun_mold_native
    map_resize          order-0 resize of a uint8 class map into NIfTI memory order          -- cfun_map_resize
    detect_native       mold_inputs_native, predict_inference, the un-mold into the RESAMPLED shape (what ``detect`` would see
                        from the .npy), postprocess, map_resize to the image's own shape
    predict_for_submit  the loop of LiTS_main.predict_for_submit (LiTS_2017/LiTS_main.py:370-394)
    mold_inputs_heart   the HEART configurations' mold_inputs (model.py:1774-1810) in one pass from the loader's array: order-1
                        resize, cast back, z-score; no label, no rotation                    -- cfun_sample_heart
    detect_heart        mold_inputs_heart, then evaluate.detect_molded into the image's own shape

The rule is include/cfun_native.h's; tests/native_ref.py restates it and tests/test_native_ref.py holds the restatement to
scipy's zoom (the code path oracle.cfun_oracle.skimage_resize stands on) bit for bit.  Nothing here waits for the device except
predict_for_submit's one read of the final map per case.
"""
import ctypes as C
import os
import re

import numpy as np
import torch

from . import _lib, evaluate, nifti, sample, utils
from ._lib import check, ptr, stream
from .ops import ptr_raw

_ELEM = {torch.int16: _lib.ELEM_INT16, torch.float32: _lib.ELEM_FLOAT32, torch.float64: _lib.ELEM_FLOAT64}


def diag_spacing(affine):
    """``preprocessing.get_spacing``: abs of the affine's three diagonal entries -- the fork's rule, NOT the column norms of
    ``evaluate.affine_spacing`` (the two agree only for an axis-aligned affine).  A zero entry would resample to an empty shape."""
    a = np.asarray(affine, dtype=np.float64)
    s = np.abs(np.array([a[0, 0], a[1, 1], a[2, 2]]))
    if not np.all(s > 0):
        raise ValueError("diag_spacing: the affine's diagonal %s has a zero entry (a rotated affine?)" % (s.tolist(),))
    return s


def resampled_shape(shape, spacing, mean_spacing):
    """``np.round(shape * spacing / MEAN_SPACING).astype(np.int32)``, the reference's expression in float64 (numpy rounds half
    to even)."""
    shape = np.asarray(tuple(int(v) for v in shape))
    return np.round(shape * np.asarray(spacing, dtype=np.float64) / np.asarray(mean_spacing, dtype=np.float64)).astype(np.int32)


def _upload(image, dev):
    """The volume on the device in its own dtype and memory order (an int16 Fortran array stays int16 Fortran); dtypes the
    kernel does not read are cast to float64 there."""
    if not torch.is_tensor(image):
        image = np.asarray(image)
        if image.dtype in (np.uint16, np.uint32, np.uint64):
            image = image.astype(np.float64)          # (no torch dtype to upload these in)
        image = torch.from_numpy(image)
    if image.dim() != 3:
        raise ValueError("mold_inputs_native: [H,W,D] volume expected, got %s" % (tuple(image.shape),))
    t = image.to(dev)
    return t if t.dtype in _ELEM else t.to(torch.float64)


def mold_inputs_native(config, image, spacing, device=None):
    """One volume [H,W,D] on the scanner's grid (numpy or tensor, any strides; int16, float32 and float64 are read as they
    are) with voxel ``spacing`` (mm along H, W, D) -> (molded [1,1,D',H',W'] float32 on the device, image_metas, windows,
    resampled_shape): what ``utils.mold_inputs_lits`` returns for the volume preprocessing.py would have stored, plus the shape
    it would have stored it at.  Raises when that shape exceeds PAD_IMAGE_SHAPE (the reference dies on a broadcast error)."""
    lib = _lib.load()
    dev = torch.device(device) if device is not None else utils._device()
    t = _upload(image, dev)
    n = [int(v) for v in t.shape]
    frame = [int(v) for v in config.PAD_IMAGE_SHAPE]
    h, w, d = [int(v) for v in config.IMAGE_SHAPE[:3]]
    rs = resampled_shape(n, spacing, config.MEAN_SPACING)
    r = [int(v) for v in rs]
    if min(n) <= 0 or min(r) <= 0:
        raise ValueError("mold_inputs_native: empty volume: source %s resamples to %s" % (n, r))
    if any(k > p for k, p in zip(r, frame)):
        raise ValueError("mold_inputs_native: the resampled shape %s does not fit PAD_IMAGE_SHAPE %s" % (r, frame))
    sx, sy, sz = [int((p - k) / 2.0) for p, k in zip(frame, r)]
    ph, pw, pd = frame
    lo, hi = torch.aminmax(t)
    clip = torch.stack([lo, hi]).to(torch.float64).contiguous()          # scikit-image's clip=True: the source's own range
    out = torch.empty((d, h, w), dtype=torch.float32, device=dev)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    check(lib.cfun_mold_native(ptr_raw(t), i64(*t.stride()), _ELEM[t.dtype], i32(*n), i32(*r), i32(*frame), i32(sx, sy, sz),
                               i32(h, w, d), ptr(clip), 1, ptr(out), stream(t)), "mold_native")
    window = (sz * d / pd, sx * h / ph, sy * w / pw, config.IMAGE_MIN_DIM - sz * d / pd, config.IMAGE_MAX_DIM - sx * h / ph,
              config.IMAGE_MAX_DIM - sy * w / pw)
    meta = utils.compose_image_meta(0, (h, w, d), window, np.zeros([config.NUM_CLASSES], dtype=np.int32))
    return out[None, None], np.stack([meta]), np.stack([window]), rs


def map_resize(cmap, out_shape, fortran=True):
    """uint8 class map [D,H,W] on the device (any strides) -> uint8 [H',W',D'] = ``out_shape`` on the device, each element
    the order-0 pick of skimage.transform.resize(cmap.permute(1, 2, 0), out_shape, order=0).  ``fortran``: the result's memory is
    in NIfTI order (H' fastest), so ``nifti.save`` writes it without a transpose; False: dense in C order."""
    lib = _lib.load()
    if cmap.dim() != 3 or cmap.dtype != torch.uint8:
        raise ValueError("map_resize: uint8 [D,H,W] map expected, got %s %s" % (cmap.dtype, tuple(cmap.shape)))
    ho, wo, do = [int(v) for v in out_shape]
    if min(ho, wo, do) <= 0 or min(cmap.shape) <= 0:
        raise ValueError("map_resize: empty extent: %s -> %s" % (tuple(cmap.shape), (ho, wo, do)))
    src = cmap.permute(1, 2, 0)
    if fortran:
        base = torch.empty((do, wo, ho), dtype=torch.uint8, device=cmap.device)
        out = base.permute(2, 1, 0)
    else:
        base = out = torch.empty((ho, wo, do), dtype=torch.uint8, device=cmap.device)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    check(lib.cfun_map_resize(ptr_raw(cmap), i64(*src.stride()), i32(*src.shape), ptr(base), i64(*out.stride()),
                              i32(ho, wo, do), stream(cmap)), "map_resize")
    return out


def detect_native(hot, image, affine, postprocess=None):
    """``evaluate.detect_original`` for one LiTS volume as its NIfTI file holds it: ``image`` [H,W,D] in the scanner's grid,
    ``affine`` the file's.  The result is detect_original's dict for the RESAMPLED volume -- rois, class_ids, scores and
    ``mask_device`` (uint8 [Dr,Hr,Wr]) are what it returns from the fork's .npy -- plus ``resampled_shape`` (Hr, Wr, Dr) and
    ``mask_native``: ``mask_device`` brought back to the image's own shape, uint8 [H,W,D] in NIfTI memory order, the array
    predict_for_submit writes.  ``postprocess`` as in detect_original; it runs on the resampled grid, before the way back."""
    if not evaluate._is_lits(hot.config):
        raise ValueError("detect_native: a LiTS configuration (PAD_IMAGE_SHAPE, MEAN_SPACING) is expected")
    dev = next(hot.parameters()).device
    molded, _, windows, rs = mold_inputs_native(hot.config, image, diag_spacing(affine), device=dev)
    res = evaluate.detect_molded(hot, molded, tuple(float(v) for v in windows[0]), [int(v) for v in rs], postprocess)
    res["resampled_shape"] = tuple(int(v) for v in rs)
    res["mask_native"] = map_resize(res["mask_device"], [int(v) for v in image.shape[:3]])
    return res


def mold_inputs_heart(config, images, device=None):
    """``utils.mold_inputs`` through cfun_sample_heart: every image [H,W,D,1] (numpy or tensor, its own dtype and memory order;
    int16, float32 and float64 are read in place) -> (molded float32 [N,1,D',H',W'] on the device, image_metas, windows), the
    same triple.  The rule is include/cfun_sample_heart.h's without a label and without a rotation; an integer image is cast
    back to its dtype after the resize, as mold_inputs does."""
    dev = torch.device(device) if device is not None else utils._device()
    if config.IMAGE_RESIZE_MODE != "self":
        raise NotImplementedError("mold_inputs_heart: IMAGE_RESIZE_MODE %r" % (config.IMAGE_RESIZE_MODE,))
    mx, mn = int(config.IMAGE_MAX_DIM), int(config.IMAGE_MIN_DIM)
    molded, metas, windows = [], [], []
    for image in images:
        if image.ndim != 4 or image.shape[3] != 1:
            raise ValueError("mold_inputs_heart: [H,W,D,1] volume expected, got %s" % (tuple(image.shape),))
        vol = image[..., 0]
        # the reference casts the resized image back to the LOADER's dtype: decided before _upload widens what the kernel cannot read
        integer = not vol.dtype.is_floating_point if torch.is_tensor(vol) else bool(np.issubdtype(np.asarray(vol).dtype, np.integer))
        out = sample.resize_rotate_box(_upload(vol, dev), None, (mx, mx, mn), None, zscore=True, truncate=integer)[0]
        molded.append(out[None])
        window = (0, 0, 0, mn, mx, mx)
        metas.append(utils.compose_image_meta(0, tuple(image.shape), window, np.zeros([config.NUM_CLASSES], dtype=np.int32)))
        windows.append(window)
    return torch.stack(molded), np.stack(metas), np.stack(windows)


def detect_heart(hot, image, postprocess=None):
    """``evaluate.detect_original`` for one raw heart volume [H,W,D,1] with the mold done by ``mold_inputs_heart``: the same
    dict, un-molded into the image's own shape."""
    if evaluate._is_lits(hot.config):
        raise ValueError("detect_heart: a heart configuration is expected (the LiTS route is detect_native)")
    if image.ndim != 4:
        raise ValueError("detect_heart: [H,W,D,1] volume expected, got shape %s" % (tuple(image.shape),))
    dev = next(hot.parameters()).device
    molded, _, windows = mold_inputs_heart(hot.config, [image], device=dev)
    return evaluate.detect_molded(hot, molded, tuple(float(v) for v in windows[0]), [int(v) for v in image.shape[:3]], postprocess)


def _submit_case(case, index):
    """-> (image array as the file holds it, affine, number in the output's name)"""
    if isinstance(case, (str, os.PathLike)):
        img = nifti.load(case)
        image, affine, name = img.get_data(), img.affine, os.path.basename(str(case))
    else:
        image, affine = case[0], case[1]
        name = case[2] if len(case) > 2 else ""
    m = re.search(r"(\d+)(?:\.nii(?:\.gz)?)?$", str(name))
    return image, np.asarray(affine, dtype=np.float64), int(m.group(1)) if m else index


def predict_for_submit(hot, cases, save_dir, limit=None, postprocess=None):
    """The loop of ``LiTS_main.predict_for_submit`` from the scanner's grid.  ``cases``: NIfTI paths (``test-volume-<i>.nii.gz``),
    or ``(array, affine[, name])`` tuples; ``limit``: only the first so many (``run_test``'s meaning; the fork's ``args.limit`` is
    the first index).  Per case: ``detect_native``, then ``mask_native`` is written as uint8 with the image's affine to
    ``save_dir/test-segmentation-<i>.nii`` -- <i> the number the case's name ends in, else its position in ``cases``.  A case
    without detections writes zeros (the reference's bare ``except`` skips it silently).  Only the final map crosses to the host.
    Returns (saved paths, detect_native's dicts)."""
    os.makedirs(save_dir, exist_ok=True)
    saved, results = [], []
    for index, case in enumerate(list(cases)[:limit]):
        image, affine, number = _submit_case(case, index)
        res = detect_native(hot, image, affine, postprocess)
        path = os.path.join(save_dir, "test-segmentation-%d.nii" % number)
        nifti.save(nifti.Nifti1Image(res["mask_native"].cpu().numpy(), affine), path)
        saved.append(path)
        results.append(res)
    return saved, results
