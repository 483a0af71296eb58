/*
 * cfun_cc.h -- connected components of a class map on the device: label them, and clean the map (keep the largest
 * component of each group, drop components below a size).  This is the step every user of a whole-heart or liver segmenter
 * puts between the un-mold and the scoring; the reference has no such function, so nothing here is pinned by it: the pin is
 * scipy.ndimage.label on the host (tests/cc_ref.py) plus hand-written known answers (tests/test_cc_ref.py).
 *
 * Why a header of its own: the same reason as cfun_sample.h and cfun_eval.h.  These entries live in the same shared object
 * as cfun_hip.h's and follow the same conventions (device pointers, POD arguments, caller-owned workspace, stream as void*,
 * int return code, enqueue only), but cfun_hip.h is tied symbol for symbol to cfun_amd/_lib.py's EXPORTS table.  These are
 * bound from a table of their own, CC_SIGNATURES / CC_EXPORTS, in the same _lib.load(); tests/test_cc_emu.py and
 * tests/test_cc_gpu.py carry the header-equals-table check and the ran-under-guard check for this table.
 *
 * Nothing here synchronises or reads device memory on the host.
 */
#ifndef CFUN_CC_H
#define CFUN_CC_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which non-zero neighbours are adjacent: voxels holding the same byte, or any two non-zero voxels (the organ as a whole). */
#define CFUN_CC_CLASS 0
#define CFUN_CC_FOREGROUND 1

/*
 * Bytes of workspace cfun_cc_label / cfun_cc_filter need for a [D,H,W] map and K classes (0 when a dimension is 0, or when
 * the arguments are ones the two entries reject).
 */
size_t cfun_cc_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K);

/*
 * Label the connected components of a class map.
 *
 *   pred            dense uint8 [D,H,W] (x fastest): what cfun_unmold_argmax / cfun_unmold_overlap write
 *   dims            {D, H, W}
 *   connectivity    6 (faces) or 26 (faces, edges, corners)
 *   mode            CFUN_CC_CLASS: two non-zero neighbours are adjacent when they hold the same byte;
 *                   CFUN_CC_FOREGROUND: when both are non-zero
 *   labels          int32 [D,H,W]: 0 for a zero voxel, otherwise 1 + the smallest linear index (z * H + y) * W + x of any
 *                   voxel of its component.  The labelling is canonical: it depends on the map alone, not on scheduling.
 *   workspace       reserved: cfun_cc_label keeps all its state in labels; the pointer and size are not looked at
 *
 * Every byte value is labelled, values >= K of a later cfun_cc_filter included.
 */
int cfun_cc_label(const uint8_t* pred, const int32_t* dims, int32_t connectivity, int32_t mode, int32_t* labels,
                  void* workspace, size_t workspace_bytes, cfun_stream_t stream);

/*
 * Clean a class map with the labels cfun_cc_label wrote for it (same dims, same mode).
 *
 * The components are taken in groups: in CFUN_CC_CLASS mode one group per class 1 .. K-1, in CFUN_CC_FOREGROUND mode the
 * one group of all non-zero voxels.  A voxel keeps its byte iff its component holds at least min_voxels voxels and, when
 * largest_only is non-zero, is the largest of its group -- of several components tied for largest, the one with the
 * smallest label.  Every other voxel becomes 0.
 *
 *   out             uint8 [D,H,W]
 *   stats           int64 [K][3], fully written by every successful call: per group {components, voxels of the largest
 *                   component, voxels removed}.  CFUN_CC_CLASS: row c is class c, row 0 is zero.  CFUN_CC_FOREGROUND: row 0
 *                   is the foreground, the other rows are zero.
 *
 * Bytes >= K are foreground like any other in CFUN_CC_FOREGROUND mode (as "> 0" counts them).  In CFUN_CC_CLASS mode they
 * belong to no group: they are copied through unchanged and appear in no row of stats.
 *
 * Both entries return CFUN_EINVAL without launching when D * H * W >= 2^31 - 1, a dimension is negative, connectivity is
 * not 6 or 26, the mode is unknown, K is outside 1 .. 15 or min_voxels < 0; cfun_cc_filter returns CFUN_EWORKSPACE when
 * the workspace is smaller than cfun_cc_workspace_bytes().  A volume with a zero dimension succeeds without a kernel
 * launch; stats is then all zeros.  Only integers are involved and none of them depends on the order in which workgroups
 * arrive: every run gives the same bits.
 */
int cfun_cc_filter(const uint8_t* pred, const int32_t* labels, const int32_t* dims, int32_t K, int32_t mode,
                   int32_t largest_only, int64_t min_voxels, uint8_t* out, int64_t* stats, void* workspace,
                   size_t workspace_bytes, cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
