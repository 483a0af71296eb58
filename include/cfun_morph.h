/*
 * cfun_morph.h -- morphology of a class map with a ball of a physical radius, on the device: erode, dilate, open, close.  The
 * step users put between "keep the largest component / fill the holes" (cfun_cc.h, cfun_fill.h) and the scoring: open a liver
 * mask by 2 mm to shave off leaks along vessels, close a ventricle by 1.5 mm to bridge a one-voxel gap, erode or dilate one
 * class to build a margin.  The reference has no such function, so nothing here is pinned by it: the pin is
 * scipy.ndimage.binary_erosion / binary_dilation with an explicitly built structuring element (tests/morph_ref.py), a
 * brute-force restatement of the field below and hand-written known answers (tests/test_morph_ref.py).
 *
 * A header of its own for the same reason as cfun_cc.h: the entries live in the same shared object as cfun_hip.h's and follow
 * the same conventions (device pointers, POD arguments, caller-owned workspace, stream as void*, int return code, enqueue
 * only), and are bound from a table of their own, MORPH_SIGNATURES / MORPH_EXPORTS, in cfun_amd/_lib.py's load();
 * tests/test_morph_emu.py and tests/test_morph_gpu.py carry the header-equals-table check and the ran-under-guard check.
 *
 * Nothing here synchronises or reads device memory on the host.
 *
 * Definitions.  All float32, operation for operation, no FMA contraction; fl() is rounding to float32.
 *
 *   spacing2 = {sz2, sy2, sx2}   each the float32 of the double product of a spacing with itself
 *   r2                           the float32 of the double radius * radius
 *                                (both formed on the host, as cfun_surface.h's spacing2 is)
 *
 * Ball.  An offset (dz, dy, dx) is in the ball B iff
 *     fl(fl(fl(float(dx*dx) * sx2) + fl(float(dy*dy) * sy2)) + fl(float(dz*dz) * sz2)) <= r2.
 * B always contains the origin and is symmetric.
 *
 * Field of a seed set S: cfun_surface.h's g1 -> g2 -> g3 with S in place of the surface,
 *     g1[z][y][x] = min over seeds (z, y, x') of the row       of fl(float((x - x')^2) * sx2)
 *     g2[z][y][x] = min over y'                                 of fl(g1[z][y'][x] + fl(float((y - y')^2) * sy2))
 *     g3[z][y][x] = min over z'                                 of fl(g2[z'][y][x] + fl(float((z - z')^2) * sz2))
 * with +inf for an empty minimum.  fl and + are monotone, so g3[v] <= r2 iff some seed lies at an offset in B from v.
 *
 * Dilate(O) = { v : g3_O[v] <= r2 }.  Nothing outside the volume is ever a seed.
 *
 * Erode(O, outside) = { v in O : no non-O position at an offset in B }.
 *   outside = 1: positions outside the volume count as O, so the seeds are the non-O voxels of the volume only.
 *   outside = 0: they count as non-O (scipy's border_value = 0).  This is the same field with two virtual seeds per line, at
 *   index -1 and L: in value a minimum with fl(float(k*k) * a2), k = min(i + 1, L - i), taken in each of the three sweeps.
 *
 * Open(O, outside) = Dilate(Erode(O, outside)), a subset of O.
 * Close(O, outside) = Erode(Dilate(O), outside).
 *
 * Groups, as in cfun_fill.h.  CFUN_CC_CLASS: one group per SELECTED class k in 1 .. K-1 with object pred == k; other classes and
 * bytes >= K are complement.  CFUN_CC_FOREGROUND: one group with object pred != 0.
 *
 * Write-back.  Each op is computed per group on the INPUT map, never on another group's result, and then written:
 *   ERODE and OPEN only clear: a voxel of group k that is not in the result becomes 0; nothing else changes.
 *   DILATE and CLOSE only set: a voxel with pred == 0 that is in group k's result becomes k (CLASS) or fill_value (FOREGROUND).
 *   No non-zero byte is ever rewritten.  When several groups claim a zero voxel the HIGHEST class id wins (cfun_fill_holes'
 *   rule: a tumour grows into background, not into the liver, and the liver does not grow into the tumour).
 *   CLOSE with outside = 0 can lose object voxels near a face in the binary result; the write rule ignores that: the map only
 *   gains.  Classes that are not selected, and bytes >= K in CLASS mode, are copied through.
 *
 * Statistics.  stats is int64 [K][2], fully written by every successful call: per group {voxels of the group cleared, zero
 * voxels set to the group}; a contested voxel is counted for the winner only.  Rows as in cfun_fill_holes: row k in CLASS
 * mode (row 0 and the rows of classes not selected are zero); row 0 in FOREGROUND mode, the rest zero.
 *
 * Integers only.  No result depends on the order in which workgroups arrive: every run gives the same bits.
 */
#ifndef CFUN_MORPH_H
#define CFUN_MORPH_H

#include "cfun_cc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CFUN_MORPH_ERODE 0
#define CFUN_MORPH_DILATE 1
#define CFUN_MORPH_OPEN 2
#define CFUN_MORPH_CLOSE 3

/*
 * Bytes of workspace cfun_morph_apply needs for a [D,H,W] map and K classes, whatever the op and the radius (0 when a
 * dimension is 0, or when the arguments are ones the entry rejects).
 */
size_t cfun_morph_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K);

/*
 * Apply one morphological op with the ball B(spacing2, r2) to a class map.
 *
 *   pred            dense uint8 [D,H,W] (x fastest), K classes
 *   dims            {D, H, W}, each 0 .. 4096 (float(k*k) is exact below 2^24)
 *   mode            CFUN_CC_CLASS or CFUN_CC_FOREGROUND: the groups, above
 *   op              CFUN_MORPH_ERODE, _DILATE, _OPEN or _CLOSE
 *   classes         CFUN_CC_CLASS: bit k set = class k is a group; bit 0 and bits >= K must be clear; 0 is legal (a copy, zero
 *                   stats).  CFUN_CC_FOREGROUND: not looked at.
 *   spacing2, r2    host pointer to {sz2, sy2, sx2}, and the squared radius: above
 *   outside         what a position outside the volume counts as in an erosion (ERODE, the first half of OPEN, the second
 *                   half of CLOSE): 1 object, 0 complement.  DILATE does not look at its value (it must still be 0 or 1).
 *   fill_value      CFUN_CC_FOREGROUND with DILATE or CLOSE: the byte a set voxel gets, 1 .. 255.  Otherwise not looked at.
 *   out             uint8 [D,H,W]; may not overlap pred
 *   stats           int64 [K][2], above
 *
 * Returns CFUN_EINVAL without launching, and with no output touched, when a dimension is negative or above 4096,
 * D * H * W >= 2^31 - 1, K is outside 1 .. 15, the mode or the op is unknown, classes has bit 0 or a bit >= K set in
 * CFUN_CC_CLASS mode, a spacing square is not finite and positive, r2 is negative or not finite, outside is not 0 or 1,
 * fill_value is outside 1 .. 255 where CFUN_CC_FOREGROUND DILATE or CLOSE would use it, or out overlaps pred;
 * CFUN_EWORKSPACE when the workspace is smaller than cfun_morph_workspace_bytes().  A volume with a zero dimension succeeds
 * without a kernel launch; stats is then all zeros.  When r2 is below every spacing square B is the origin alone: the call
 * succeeds, the map is copied and the stats are zero.  The call enqueues only.
 */
int cfun_morph_apply(const uint8_t* pred, const int32_t* dims, int32_t K, int32_t mode, int32_t op, uint32_t classes,
                     const float* spacing2, float r2, int32_t outside, int32_t fill_value, uint8_t* out, int64_t* stats,
                     void* workspace, size_t workspace_bytes, cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
