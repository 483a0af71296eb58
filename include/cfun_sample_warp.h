/*
 * cfun_sample_warp.h -- elastic and affine training augmentation of a network-size sample on the device: a smooth displacement
 * field from a coarse control grid, an in-plane affine map (rotation, scale, translation) and per-axis flips, applied to the
 * image (order 0 or order 1) and to the labels (order 0) as ONE gather pass over the output plus one small finish launch for the
 * GT box.  It is placed AFTER any of the three sample routes (cfun_sample.h, cfun_sample_lits.h, cfun_sample_heart.h): the source
 * is what those produce before utils.mold_image, a dense float32 [D,H,W] image and dense uint8 [D,H,W] labels.
 *
 * Where it comes from: the reference's load_image_gt (model.py:1022-1045) keeps Matterport's whitelist of mask-safe augmenters
 * -- Fliplr, Flipud, CropAndPad, Affine, PiecewiseAffine -- and only ever builds iaa.Affine(rotate=angle, order=0).  This entry
 * is the rest of that list as one warp.  imgaug is not available to this project's environments, so neither its Affine nor its
 * PiecewiseAffine is recorded: the trilinear control grid below is THIS PROJECT'S OWN RULE, not a restatement of imgaug's.
 *
 * Why a header of its own: the reason cfun_sample_lits.h and cfun_sample_heart.h give.  These entries are bound from
 * WARP_SAMPLE_SIGNATURES / WARP_SAMPLE_EXPORTS in the same _lib.load(); tests/test_sample_warp_*.py carry the
 * header-equals-table and ran-under-guard checks.  Same conventions: device pointers, POD arguments, caller-owned workspace,
 * stream as void*, int return code, enqueue only.  Nothing here synchronises or reads device memory on the host.
 *
 * What pins the rule (tests/test_sample_warp_ref.py): a numpy float64 restatement written from this header equals
 * scipy.ndimage.map_coordinates on its own coordinate stack -- order 0 exactly away from half-integers and the border, order 1
 * within one float32 rounding everywhere -- and a set of hand answers; with a zero grid and a rotation map the kernel equals
 * cfun_sample_lits bit for bit (tests/sample_warp_cases.py).
 */
#ifndef CFUN_SAMPLE_WARP_H
#define CFUN_SAMPLE_WARP_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace cfun_sample_warp needs for a volume of extent dims = {D, H, W}; 0 for a bad extent. */
size_t cfun_sample_warp_workspace_bytes(const int32_t* dims);

/* The largest control-grid extent per axis cfun_sample_warp accepts.  A workgroup stages the control values of its output
 * brick in LDS; in the worst case (a grid finer than the volume) a brick spans the whole grid, so the bound is the LDS
 * budget: 3 components x max_grid^3 float32. */
int32_t cfun_sample_warp_max_grid(void);

/*
 * Warp image and labels and box the warped labels.
 *
 *   image, labels     source: dense float32 [D,H,W] and dense uint8 [D,H,W], dims = {D, H, W}
 *   grid, gdims       DEVICE float32 [3][gz][gy][gx], dense: displacements in voxels, component 0 along z, 1 along y, 2 along x;
 *                     gdims = {gz, gy, gx}.  grid NULL: no displacement (gdims is then not read and may be NULL)
 *   map               HOST pointer to six doubles m0 .. m5 (read before return), or NULL: none
 *   flips             bit 0: flip z, bit 1: flip y, bit 2: flip x
 *   image_order       0: nearest, 1: trilinear (the labels are always nearest)
 *   out_image         dense float32 [D,H,W];  out_labels: dense uint8 [D,H,W]
 *   raw_box, box, empty   int32[6], int32[6], int32[1] as in cfun_sample.h, over out_labels != 0
 *
 * Rule for output voxel o = (z, y, x), n = (D, H, W), g = (gz, gy, gx); every step in double and in this operation order, no
 * FMA contraction:
 *   1. control coordinate, per axis a:   u = (double)o_a * ((double)(g_a - 1) / (double)(n_a - 1))  -- the quotient first;
 *      u = 0 when n_a == 1;   i = min(floor(u), g_a - 2);   t = u - i.
 *   2. displacement: with lerp(a, b, t) = (1 - t) * a + t * b, each component c of d is the blend of its eight control
 *      values grid[c][iz + dz][iy + dy][ix + dx], converted float32 -> double, along x first, then y, then z:
 *        e(dz, dy) = lerp(v(dz, dy, 0), v(dz, dy, 1), tx);  f(dz) = lerp(e(dz, 0), e(dz, 1), ty);  d_c = lerp(f(0), f(1), tz).
 *      Without a grid d = 0.
 *   3. displaced position:  p = o + d   per axis.
 *   4. in-plane map, cfun_sample_lits.h's convention and k_lits_gather's operation order:
 *        col = m0 * p_x + m1 * p_y + m2      row = m3 * p_x + m4 * p_y + m5
 *        s = (p_z, row, col);   without a map s = p.
 *   5. flips:  s_a = (double)(n_a - 1) - s_a   for each flagged axis.
 *   6. labels, and the image with image_order 0:  r_a = trunc(s_a > 0 ? s_a + 0.5 : s_a - 0.5)  (half away from zero) per
 *      axis; the source element at r when 0 <= r_a < n_a on every axis -- tested in double, before any cast --, else 0.
 *   7. image with image_order 1:  i0_a = floor(s_a), f_a = s_a - i0_a; the eight taps at i0 + {0, 1} per axis converted
 *      float32 -> double, a tap outside the source counting as 0.0; the lerp nesting of step 2 (x with f_x, then y, then z),
 *      then ONE cast to float32.  A tap inside the source is always read and multiplied, also by a weight of 0, so a NaN spreads
 *      as in cfun_native.h.  When s_a <= -1 or s_a >= n_a on some axis every tap lies outside and the result is +0.0.
 *   8. a non-finite source coordinate gives image 0 and label 0 (the tests of steps 6 and 7 fail for a NaN; an infinity lies
 *      outside).  A NaN control value therefore gives zeros wherever its weight enters.
 *   9. box: per-workgroup min and max of z, y, x over out_labels != 0, then one workgroup reduces the partials and applies
 *      cfun_sample.h's rule: all zeros when z1 == z2 or when nothing is set, the 5 % expansion in double with
 *      floor(max(0, .)) and ceil(min(dim, .)), empty = 1 when no voxel is set.
 * No float atomics and no global atomics: two runs agree bit for bit.
 *
 * Returns CFUN_EINVAL -- and writes nothing -- for a null pointer (grid and map excepted; gdims with a grid), a non-positive
 * extent or 2^31 or more voxels, a grid extent below 2 or above cfun_sample_warp_max_grid(), a map entry that is not finite,
 * image_order outside {0, 1}, flip bits above 7, or an output whose bytes overlap those of image, labels or grid;
 * CFUN_EWORKSPACE for a null workspace or one smaller than cfun_sample_warp_workspace_bytes(dims).  Every accepted call has at
 * least one voxel (a zero extent is refused), so no call launches an empty grid.
 */
int cfun_sample_warp(const float* image, const uint8_t* labels, const int32_t* dims, const float* grid, const int32_t* gdims,
                     const double* map, int32_t flips, int32_t image_order, float* out_image, uint8_t* out_labels,
                     int32_t* raw_box, int32_t* box, int32_t* empty, void* workspace, size_t workspace_bytes,
                     cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
