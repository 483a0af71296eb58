/*
 * cfun_sample_heart.h -- the heart task's sample from the loader's own grid: what the reference does on the host between the
 * NIfTI file and the network's input -- utils.resize_image (skimage.transform.resize(order=1, clip=True), utils.py:342-393, with
 * its cast back to the loader's dtype at :392), utils.resize_mask (order 0, :396-408), the per-slice nearest rotation of
 * load_image_gt with the [H,W,D] -> [D,H,W] re-layout and the GT box (cfun_sample.h), and mold_image's z-score (model.py:1902) --
 * as ONE gather pass over the output, one small finish launch and one flat pass.  Every voxel of that chain depends on at most
 * eight source voxels and then on two global scalars, so neither resized volume is ever built.
 *
 * Why a header of its own: the reason cfun_sample_lits.h and cfun_native.h give.  These entries are bound from
 * HEART_SAMPLE_SIGNATURES / HEART_SAMPLE_EXPORTS in the same _lib.load(); tests/test_sample_heart_*.py carry the
 * header-equals-table and ran-under-guard checks.  Same conventions: device pointers, POD arguments, caller-owned workspace,
 * stream as void*, int return code, enqueue only.  Nothing here synchronises or reads device memory on the host.
 *
 * What pins the rule (tests/test_sample_heart_ref.py): the image before the z-score, restated in numpy float64, equals
 * oracle.cfun_oracle.skimage_resize(src, out, 1) -- scipy's zoom(order=1, mode='grid-constant', grid_mode=True) plus the clip --
 * cast, then pushed through tests/sample_ref.py's rotation and re-layout, BIT FOR BIT; labels and boxes equal
 * skimage_resize(mask, out, 0) pushed through the same restatement exactly.  NOT pinned: scikit-image and imgaug themselves (not
 * available to this project's environments), and the rotation's exact half-voxel ties (cfun_sample.h).
 */
#ifndef CFUN_SAMPLE_HEART_H
#define CFUN_SAMPLE_HEART_H

#include "cfun_hip.h"
#include "cfun_native.h" /* CFUN_ELEM_INT16 / FLOAT32 / FLOAT64: the image's elem_kind */

#ifdef __cplusplus
extern "C" {
#endif

/* label_kind of cfun_sample_heart: what cfun_amd.nifti.load yields for a label file */
#define CFUN_LABEL_INT8 0
#define CFUN_LABEL_UINT8 1
#define CFUN_LABEL_INT16 2
#define CFUN_LABEL_INT32 3

/* Bytes of workspace cfun_sample_heart needs for an output of extent out_dims = {H', W', D'}; 0 for a bad extent. */
size_t cfun_sample_heart_workspace_bytes(const int32_t* out_dims);

/*
 * Resize, cast, rotate, re-lay [H,W,D] -> [D',H',W'], cast the label, box it and z-score the image.
 *
 *   image, image_strides  source of extent dims = {H, W, D}, elements of elem_kind, read in place through element strides
 *   label, label_strides  label source of the same extent, elements of label_kind, read in place through ITS element strides;
 *                         label NULL: no label -- out_label, raw_box, box and empty are not written and may be NULL
 *   out_dims              {H', W', D'}
 *   clip                  DEVICE pointer to two doubles lo, hi (the source's min / max: scikit-image's clip=True), or NULL: none
 *   truncate              non-zero: step 3 (the loader's dtype is an integer)
 *   cos_t, sin_t, rotate  as in cfun_sample_rotate_bbox: of the angle, computed by the caller in double; rotate 0 = no rotation
 *   zscore                non-zero: step 7
 *   out_image             dense float32 [D',H',W'];  out_label: dense uint8 [D',H',W']
 *   raw_box, box, empty   int32[6], int32[6], int32[1] as in cfun_sample.h
 *   stats                 DEVICE double[2]: mean, std of step 7; may be NULL without zscore
 *
 * Rule for output voxel (z, y, x), every step in this operation order, double unless said, no FMA contraction:
 *   1. rotation in the RESIZED grid, cfun_sample.h's rule verbatim with cy = H' / 2 - 0.5, cx = W' / 2 - 0.5:
 *        sx =  c * (x - cx) + s * (y - cy) + cx        ix = floor(sx + 0.5)
 *        sy = -s * (x - cx) + c * (y - cy) + cy        iy = floor(sy + 0.5)
 *      without rotate (iy, ix) = (y, x), bit-identical to angle 0.  Outside [0, H') x [0, W') image and label are 0
 *      (the image's 0 still enters step 7).
 *   2. r = (iy, ix, z) is a voxel of the never-built resized volume: steps 3 to 5 of cfun_native.h with R = out_dims, n = dims:
 *        c = ((double)r + 0.5) * ((double)n / (double)R) - 0.5,   f = floor(c),   w1 = c - f,   w0 = 1.0 - w1     per axis
 *        t = 0.0; for a in {0,1} (H), b in {0,1} (W), c in {0,1} (D) -- D innermost --   t = t + ((v * wH_a) * wW_b) * wD_c
 *      with v the source element at (fH + a, fW + b, fD + c) converted to double; a tap outside the source is skipped, a tap
 *      inside it is always multiplied (also by a weight of 0: a non-finite float source spreads as in scipy's zoom);
 *      with clip:  t = t < lo ? lo : t;  t = t > hi ? hi : t   -- a NaN t stays a NaN, a NaN bound does not act.
 *   3. with truncate: t = trunc(t) + 0.0 -- the reference's image.astype(image_dtype) for an integer loader dtype, which rounds
 *      toward zero; the addition turns the -0.0 that trunc gives on (-1, 0) into the integer's +0.0 and changes nothing else
 *      (a NaN stays a NaN).  After the clip to an int16 source's range t always lies in int16's range, so no wrap-around is
 *      restated.
 *   4. s = (float)t, round to nearest even.
 *   5. label: the source element at cfun_resize3d's order-0 index of (iy, ix, z) per axis,
 *        i(r, n, R) = clamp((int)floor(((double)r + 0.5) * ((double)n / (double)R)), 0, n - 1);
 *      its low 8 bits are stored; the box counts `label > 0` on the value READ (cfun_sample.h: an int16 256 is stored as 0 yet
 *      counts, a negative label is stored non-zero and is left out).
 *   6. raw_box, box, empty: cfun_sample.h -- utils.extract_bboxes over label > 0, all zeros when z1 == z2 or when the label is
 *      empty, the 5 % expansion in double with floor(max(0, .)) and ceil(min(dim, .)), empty = 1 when no voxel has label > 0.
 *   7. with zscore: N = D' * H' * W';  S1 = sum of (double)s and S2 = sum of (double)s * (double)s over ALL N voxels, the
 *      rotation's zeros included, in a fixed order -- per thread, per wave, per workgroup, then over the workgroups' partials;
 *      no float atomics, so two runs agree bit for bit;
 *        mean = S1 / N,   var = S2 / N - mean * mean,   std = sqrt(var)     -> stats[0], stats[1]
 *      and a second flat pass stores (float)(((double)s - mean) / std) in place of s.  An all-zero volume gives NaN
 *      everywhere (the reference's 0 / 0); rounding can make var of a constant volume slightly negative: NaN as well.
 *      The order of the sums is the implementation's, so mean and var are held to a bound, not to bits: a double sum of N
 *      terms in any order is within N * 2^-53 * sum|term| of the exact one, hence against the float64 mean m64 and variance
 *      v64 of the un-normalised output   |mean - m64| <= N * 2^-52 * mean|s|   and   |var - v64| <= 4 * N * 2^-52 * mean(s^2)
 *      (worst case, both sides' rounding counted; the second has the two sums and the product mean * mean in it).
 *      Without zscore s itself is stored.
 *
 * Preconditions (the caller's): label and image have the extent dims.
 *
 * Returns CFUN_EINVAL -- and writes nothing -- for a null required pointer (clip never; label and its four outputs together
 * when label is NULL; stats without zscore), a non-positive extent, an unknown elem_kind or label_kind, H' > 65535, or more
 * than 2^31 - 1 tiles; CFUN_EWORKSPACE for a null workspace or one smaller than cfun_sample_heart_workspace_bytes(out_dims).
 */
int cfun_sample_heart(const void* image, const int64_t* image_strides, int32_t elem_kind, const void* label,
                      const int64_t* label_strides, int32_t label_kind, const int32_t* dims, const int32_t* out_dims,
                      const double* clip, int32_t truncate, double cos_t, double sin_t, int32_t rotate, int32_t zscore,
                      float* out_image, uint8_t* out_label, int32_t* raw_box, int32_t* box, int32_t* empty, double* stats,
                      void* workspace, size_t workspace_bytes, cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
