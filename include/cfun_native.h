/*
 * cfun_native.h -- LiTS from the scanner's grid, both ends on the device.
 *
 * In front: the fork's preprocessing.py resamples every NIfTI volume to the mean spacing on the host
 * (skimage.transform.resize(order=1, clip=True), stored as float32 .npy) and its mold_inputs (LiTS_2017/model.py:1730-1775)
 * then clamp-normalises that array, centres it in the zero PAD_IMAGE_SHAPE frame and nearest-resizes the frame.  mold_inputs
 * takes exactly ONE voxel of the resampled volume per network voxel, and that voxel is a trilinear blend of eight source
 * voxels: cfun_mold_native is the whole chain as one gather over the OUTPUT, eight taps each, with neither the resampled
 * volume nor the frame ever built.
 * Behind: predict_for_submit (LiTS_2017/LiTS_main.py:370-394) brings the class map back to the scanner's grid with an order-0
 * resize: cfun_map_resize, bytes in and bytes out through strides, so the result lands in the NIfTI file's own order.
 *
 * Why a header of its own: the reason cfun_sample_lits.h gives.  These entries are bound from NATIVE_SIGNATURES /
 * NATIVE_EXPORTS in the same _lib.load(); tests/test_native_*.py carry the header-equals-table and ran-under-guard checks.
 * Same conventions: device pointers, POD arguments, stream as void*, int return code, enqueue only.  Nothing here synchronises
 * or reads device memory on the host; neither entry needs a workspace.
 *
 * What pins the rule (tests/test_native_ref.py): steps 3-5 below, restated in numpy float64, equal
 * scipy.ndimage.zoom(order=1, mode='grid-constant', grid_mode=True) followed by the clip -- the code path
 * oracle.cfun_oracle.skimage_resize stands on -- BIT FOR BIT in float64, and the whole rule equals that resize cast to
 * float32 and pushed through the rule of cfun_sample_lits.h without a map, bit for bit.  NOT pinned: scikit-image itself
 * (not available to this project's environments), and sources with a NaN under `clip` (numpy's clip to a NaN range makes
 * every voxel NaN; here a NaN bound does not act).
 */
#ifndef CFUN_NATIVE_H
#define CFUN_NATIVE_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* elem_kind of cfun_mold_native: what cfun_amd.nifti.load yields for CT -- raw, float, or scaled by slope / inter */
#define CFUN_ELEM_INT16 0
#define CFUN_ELEM_FLOAT32 1
#define CFUN_ELEM_FLOAT64 2

/*
 * Resample, clip, cast, frame, resize, normalise, re-lay [H,W,D] -> [D',H',W']: one pass over the OUTPUT.
 *
 *   src, src_strides  source of extent dims = {H, W, D}, elements of elem_kind, read in place through element strides {sH, sW, sD}
 *   resampled         {Hr, Wr, Dr}: the extent the order-1 resize would produce (never built)
 *   frame             {PH, PW, PD}: the virtual zero frame;  offset {oh, ow, od}: where the RESAMPLED volume sits in it
 *                     (the reference centres it: int((P - R) / 2.0) per axis)
 *   out_dims          {H', W', D'}
 *   clip              DEVICE pointer to two doubles lo, hi (the source's min / max: scikit-image's clip=True), or NULL: none
 *   normalise         non-zero: the clamp-normalisation of step 7; 0: the float32 value of step 6 is stored
 *   out               dense float32 [D',H',W']
 *
 * Rule for output voxel (z, y, x), every step in this operation order, double unless said, no FMA contraction:
 *   1. frame index per axis, cfun_sample_lits.h step 1 (m the output extent, P the frame's, o the index):
 *        F = (int)floor(((double)o + 0.5) * ((double)P / (double)m)), clamped to [0, P - 1]
 *      -> Fy from (y, PH, H'), Fx from (x, PW, W'), Fz from (z, PD, D').
 *   2. r = F - offset per axis.  The result is 0 -- the frame's own zero, not normalised -- when r lies outside
 *      [0, Hr) x [0, Wr) x [0, Dr).
 *   3. per axis, n the source extent and R the resampled one:
 *        c = ((double)r + 0.5) * ((double)n / (double)R) - 0.5,   f = floor(c),   w1 = c - f,   w0 = 1.0 - w1
 *   4. t = 0.0; then for a in {0,1} (H), b in {0,1} (W), c in {0,1} (D) -- D innermost --
 *        t = t + ((v * wH_a) * wW_b) * wD_c
 *      with v the source element at (fH + a, fW + b, fD + c) converted to double.  A tap outside the source contributes
 *      nothing (it is skipped); a tap inside it is always multiplied, also by a weight of 0, so a non-finite float source
 *      spreads as it does in scipy's zoom.
 *   5. with clip:  t = t < lo ? lo : t;  t = t > hi ? hi : t   -- a NaN t stays a NaN, a NaN bound does not act.
 *   6. s = (float)t, round to nearest even: the .astype(np.float32) of preprocessing.py:31.
 *   7. with normalise: cfun_sample_lits.h step 5 on s -- v = (s - 300) / (-600) in float32 as two separately and correctly
 *      rounded operations, then v > 1 ? 1 : (v < 0 ? 0 : v), which keeps a NaN.
 *
 * Returns CFUN_EINVAL -- and writes nothing -- for a null pointer (clip excepted), a non-positive extent, a negative offset,
 * a resampled volume that does not fit the frame at the offset (the reference dies on a broadcast error there), an unknown
 * elem_kind, or an output of more than 2^31 - 1 tiles.  (No limit on H': the tiles are numbered along one grid axis.)
 */
int cfun_mold_native(const void* src, const int64_t* src_strides, int32_t elem_kind, const int32_t* dims,
                     const int32_t* resampled, const int32_t* frame, const int32_t* offset, const int32_t* out_dims,
                     const double* clip, int32_t normalise, float* out, cfun_stream_t stream);

/*
 * Order-0 resize of a byte volume, strides in and strides out:
 *
 *   src, src_strides  uint8 source of extent dims = {H, W, D}, read through three element strides
 *   out, out_strides  uint8 output of extent out_dims = {H', W', D'}, written through three element strides
 *
 * out[h', w', d'] = src[i(h', H, H'), i(w', W, W'), i(d', D, D')] with cfun_resize3d's order-0 index and no frame:
 *        i(o, n, m) = clamp((int)floor(((double)o + 0.5) * ((double)n / (double)m)), 0, n - 1)
 * Integers only once the index is known: bytes in, bytes out.  The product use is a dense [Dr,Hr,Wr] class map (W fastest)
 * going into a Fortran [H,W,D] volume (H fastest): a byte transpose per z plane.
 *
 * Returns CFUN_EINVAL -- and writes nothing -- for a null pointer, a non-positive extent, an output stride that is not
 * positive, or output strides under which two elements share an address (checked over the axes of extent > 1, sorted by
 * stride: each stride must be at least the previous one times its extent).
 */
int cfun_map_resize(const uint8_t* src, const int64_t* src_strides, const int32_t* dims, uint8_t* out,
                    const int64_t* out_strides, const int32_t* out_dims, cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
