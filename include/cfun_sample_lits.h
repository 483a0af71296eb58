/*
 * cfun_sample_lits.h -- the LiTS fork's training sample on the device: what Dataset.__getitem__
 * (LiTS_2017/model.py:1145-1248) does on the host per sample in front of load_image_gt -- clamp-normalise
 * (preprocess_image, :1875-1883), centre image and label in two zero PAD_IMAGE_SHAPE frames, rotate both per
 * slice (skimage.transform.rotate(order=0, mode='constant')), nearest-resize both frames to IMAGE_SHAPE --
 * as ONE gather pass with the frame never materialised, plus the GT box of cfun_sample.h.
 *
 * Why a header of its own: the reason cfun_sample.h gives.  tests/test_sample_emu.py ties cfun_sample.h symbol
 * for symbol to _lib.SAMPLE_EXPORTS; these entries are bound from LITS_SAMPLE_SIGNATURES / LITS_SAMPLE_EXPORTS
 * in the same _lib.load(), and tests/test_sample_lits_*.py carry the header-equals-table and ran-under-guard
 * checks for that table.  Same conventions: device pointers, POD arguments, caller-owned workspace, stream as
 * void*, int return code, enqueue only.  Nothing here synchronises or reads device memory on the host.
 *
 * What pins the rule: scikit-image is not available to this project's environments, so no golden could be
 * recorded from the fork's __getitem__ (as for the heart rotation and the order-1 resize).  Pinned instead
 * (tests/test_sample_lits_ref.py): without a map the result equals oracle.cfun_oracle.skimage_resize(frame, out, 0)
 * of the explicitly built frame exactly; with a rotation it equals scipy.ndimage.affine_transform(order=0,
 * mode='constant') per slice followed by that resize wherever the source coordinate lies in [0, P-1] and at
 * least 1e-6 from a half-integer.  NOT pinned: exact half-voxel ties, and the last-ulp difference between this
 * operation order and scikit-image's matrix product.
 */
#ifndef CFUN_SAMPLE_LITS_H
#define CFUN_SAMPLE_LITS_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace cfun_sample_lits needs for an output of extent out_dims = {H', W', D'}; 0 for a bad extent. */
size_t cfun_sample_lits_workspace_bytes(const int32_t* out_dims);

/*
 * Frame, rotate, resize, normalise, re-lay [H,W,D] -> [D',H',W'], cast the label and box it: one pass over
 * the OUTPUT plus one small finish launch.
 *
 *   image             float32 source of extent dims = {H, W, D}, read in place through element strides {sH, sW, sD}
 *   label             source of the same extent, read in place through ITS element strides; label_elem_size is
 *                     1 (uint8 or int8) or 4 (int32).  Only the low 8 bits are used, so the three types need no flag.
 *   frame             {PH, PW, PD}: the virtual zero frame;  offset {oh, ow, od}: where the source sits in it
 *                     (the reference centres it: int((P - n) / 2.0) per axis, the extra voxel on the high side)
 *   out_dims          {H', W', D'}
 *   map               HOST pointer to six doubles m00 m01 m02 m10 m11 m12 (read before return), or NULL: none
 *   normalise         non-zero: the clamp-normalisation of step 5; 0: the image value is copied
 *   out_image         dense float32 [D',H',W'];  out_label: dense uint8 [D',H',W']
 *   raw_box, box, empty   as cfun_sample_rotate_bbox defines them (cfun_sample.h; the fork's extract_bboxes /
 *                     extend_bbox are the same rule), over out_label != 0 on [D',H',W']
 *
 * Rule for output voxel (z, y, x), every step in this operation order, double unless said, no FMA contraction:
 *   1. frame index per axis, cfun_resize3d's order-0 rule (m the output extent, P the frame's, o the index):
 *        F = (int)floor(((double)o + 0.5) * ((double)P / (double)m)), clamped to [0, P - 1]
 *      -> Fy from (y, PH, H'), Fx from (x, PW, W'), Fz from (z, PD, D').
 *   2. with a map:   col = m00 * Fx + m01 * Fy + m02      row = m10 * Fx + m11 * Fy + m12
 *                    k = (long long)(v > 0 ? v + 0.5 : v - 0.5)    for v = col, row: half away from zero,
 *      truncating -- the rounding scikit-image's nearest-neighbour warp is believed to use (from memory; unpinned).
 *      Without a map (row, col) = (Fy, Fx).  For a rotation by `angle` degrees the caller builds, in double,
 *        t = radians(angle), c = cos t, s = sin t, cx = PW / 2 - 0.5, cy = PH / 2 - 0.5,
 *        map = (c, -s, cx - c * cx + s * cy,   s, c, cy - s * cx - c * cy)
 *      -- skimage.transform.rotate's translate(centre) . rotate . translate(-centre), used as the inverse map
 *      with rows = H and cols = W.
 *   3. 0 when (row, col) lies outside [0, PH) x [0, PW).
 *   4. subtract the offsets: 0 when (row - oh, col - ow, Fz - od) lies outside [0, H) x [0, W) x [0, D).
 *   5. image: v = (src - 300) / (-600) in float32, two separately and correctly rounded operations, then
 *      v > 1 ? 1 : (v < 0 ? 0 : v) -- a NaN stays a NaN, as the reference's masked assignments leave it.
 *      (sic: the fork's MIN_BOUND = 300, MAX_BOUND = -300.)  This is numpy's and the reference's arithmetic, and
 *      utils.preprocess_image_lits on the host.  On the device torch evaluates that function's `x / scalar` as
 *      x * (1 / scalar), one bit looser: utils.mold_inputs_lits there differs from this rule by 1 float32 ulp on
 *      about 30 % of the HU values inside the window, and returns +0.0 where this rule keeps 0 / -600 = -0.0.
 *   6. label: the low 8 bits of the source element, as uint8.
 * The zeros of steps 3 and 4 are the frame's own zeros: they are not normalised.
 *
 * Preconditions (the caller's): label values lie in [0, 255] ([0, 127] for int8); outside that range nothing
 * faults and out_label and the box still agree with each other (both see the low 8 bits).
 *
 * Returns CFUN_EINVAL -- and writes nothing -- for a null pointer (map excepted), a non-positive extent, a
 * negative offset or a source that does not fit the frame at the offset (the reference raises a broadcast
 * error there), label_elem_size other than 1 or 4, H' > 65535, or a map entry that is not finite;
 * CFUN_EWORKSPACE for a null or short workspace.
 */
int cfun_sample_lits(const float* image, const int64_t* image_strides, const void* label, const int64_t* label_strides,
                     int32_t label_elem_size, const int32_t* dims, const int32_t* frame, const int32_t* offset,
                     const int32_t* out_dims, const double* map, int32_t normalise, float* out_image, uint8_t* out_label,
                     int32_t* raw_box, int32_t* box, int32_t* empty, void* workspace, size_t workspace_bytes,
                     cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
