/*
 * cfun_fill.h -- fill the holes of a class map on the device, in 3-D or plane by plane.  A segmenter's organ mask has cavities
 * where a tumour, a vessel or a low-contrast patch was missed; keeping the largest component (cfun_cc.h) does not close them.
 * This is scipy.ndimage.binary_fill_holes per class (or on the foreground as a whole), written back into the map.  The
 * reference has no such function, so nothing here is pinned by it: the pin is scipy on the host (tests/fill_ref.py) plus
 * hand-written known answers (tests/test_fill_ref.py).
 *
 * A header of its own for the same reason as cfun_cc.h: the entries live in the same shared object as cfun_hip.h's and follow
 * the same conventions (device pointers, POD arguments, caller-owned workspace, stream as void*, int return code, enqueue
 * only), and are bound from a table of their own, FILL_SIGNATURES / FILL_EXPORTS, in cfun_amd/_lib.py's load();
 * tests/test_fill_emu.py and tests/test_fill_gpu.py carry the header-equals-table check and the ran-under-guard check.
 *
 * Nothing here synchronises or reads device memory on the host.
 */
#ifndef CFUN_FILL_H
#define CFUN_FILL_H

#include "cfun_cc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of workspace cfun_fill_holes needs for a [D,H,W] map and K classes (0 when a dimension is 0, or when the arguments
 * are ones the entry rejects).
 */
size_t cfun_fill_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K);

/*
 * Fill the enclosed holes of a class map.
 *
 *   pred            dense uint8 [D,H,W] (x fastest), K classes
 *   dims            {D, H, W}
 *   mode            the groups.  CFUN_CC_CLASS: one group per class k = 1 .. K-1; the group's object is pred == k, its
 *                   complement pred != k (other classes and bytes >= K belong to the complement).  CFUN_CC_FOREGROUND: one
 *                   group; its object is pred != 0 (bytes >= K included), its complement pred == 0.
 *   connectivity    the neighbourhood of the COMPLEMENT.  axis == -1: 6 (faces; what binary_fill_holes uses by default) or
 *   axis            26.  axis in {0, 1, 2}: the volume is a stack of independent 2-D planes perpendicular to that axis, and
 *                   connectivity is 4 or 8 within the plane; axis 0 is the axial slice of a [D,H,W] map.
 *   fill_value      CFUN_CC_FOREGROUND: the byte a filled voxel gets, 1 .. 255.  CFUN_CC_CLASS: not looked at.
 *   out             uint8 [D,H,W]; may not overlap pred (refused by pointer comparison: CFUN_EINVAL)
 *   stats           int64 [K][2], fully written by every successful call: per group {enclosed components, voxels changed to
 *                   the group}.  CFUN_CC_CLASS: row k is class k, row 0 is zero.  CFUN_CC_FOREGROUND: row 0 is the
 *                   foreground, the other rows are zero.
 *
 * Holes.  A component of a group's complement is OPEN when one of its voxels lies on a border: for axis == -1 the six faces
 * of the volume, for a planar fill the four edges of the plane (the two faces perpendicular to axis do not count).  Every
 * other component is ENCLOSED -- as in binary_fill_holes, whose dilation enters from outside the array.
 *
 * Write.  Only voxels that are 0 in pred can change; no non-zero byte is ever rewritten.  A zero voxel in an enclosed component
 * of group k becomes k (CFUN_CC_CLASS) or fill_value (CFUN_CC_FOREGROUND).  When several classes enclose the same voxel the
 * HIGHEST class id wins: in a liver map the tumour (2) lies inside the liver (1), and a cavity inside a tumour ring becomes
 * tumour, not liver.
 *
 * The two statistics can differ in either direction: an enclosed component made only of other classes' voxels (a tumour wholly
 * inside the liver) changes nothing, and a voxel enclosed by two groups is counted for the winner only.
 *
 * Returns CFUN_EINVAL without launching, and with no output touched, when D * H * W >= 2^31 - 1, a dimension is negative, K is
 * outside 1 .. 15, the mode is unknown, axis is outside -1 .. 2, connectivity does not fit axis (6 / 26 without one, 4 / 8
 * with one), fill_value is outside 1 .. 255 in CFUN_CC_FOREGROUND mode, or out overlaps pred; CFUN_EWORKSPACE when the
 * workspace is smaller than cfun_fill_workspace_bytes().  A volume with a zero dimension succeeds without a kernel launch;
 * stats is then all zeros.  Only integers are involved and none of them depends on the order in which workgroups arrive: every
 * run gives the same bits.
 */
int cfun_fill_holes(const uint8_t* pred, const int32_t* dims, int32_t K, int32_t mode, int32_t connectivity, int32_t axis,
                    int32_t fill_value, uint8_t* out, int64_t* stats, void* workspace, size_t workspace_bytes,
                    cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
