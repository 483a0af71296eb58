/*
 * cfun_lesion.h -- what lesion-level scoring needs from two component labelings, on the device: dense ranks 1 .. n with a
 * per-component table (cfun_cc_rank), and the contingency table of two rank volumes (cfun_rank_overlap).  Lesion detection,
 * lesion-wise Dice and any instance-level matching are functions of those two tables (cfun_amd/lesions.py).  The reference
 * has no such function, so nothing here is pinned by it: the pin is scipy.ndimage.label / find_objects and a numpy contingency
 * count on the host (tests/lesion_ref.py) plus hand-written known answers (tests/test_lesion_ref.py).
 *
 * Why a header of its own: the same reason as cfun_cc.h.  These entries live in the same shared object as cfun_hip.h's and
 * follow the same conventions (device pointers, POD arguments, caller-owned workspace, stream as void*, int return code,
 * enqueue only), but cfun_hip.h is tied symbol for symbol to cfun_amd/_lib.py's EXPORTS table.  These are bound from a table
 * of their own, LESION_SIGNATURES / LESION_EXPORTS, in the same _lib.load(); tests/test_lesion_emu.py and
 * tests/test_lesion_gpu.py carry the header-equals-table check and the ran-under-guard check for this table.
 *
 * Nothing here synchronises or reads device memory on the host.  Only integers are involved and none of them depends on the
 * order in which workgroups arrive: every run gives the same bits.
 */
#ifndef CFUN_LESION_H
#define CFUN_LESION_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A component table holds rows for the ranks 1 .. cap; cap lies in 1 .. CFUN_LESION_MAX_CAP. */
#define CFUN_LESION_MAX_CAP 4095
/* int64 fields of one row of cfun_cc_rank's table */
#define CFUN_LESION_FIELDS 9

/*
 * Bytes of workspace cfun_cc_rank needs for a [D,H,W] volume (0 when a dimension is 0, or when the arguments are ones the
 * entries reject).  cfun_rank_overlap needs none.
 */
size_t cfun_lesion_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t cap);

/*
 * Dense ranks and the component table of a labelled map.
 *
 *   pred      dense uint8 [D,H,W]: the map cfun_cc_label labelled
 *   labels    int32 [D,H,W]: what cfun_cc_label wrote for it (0, or 1 + the component's smallest linear index, its root)
 *   dims      {D, H, W}
 *   cap       rows of the table, 1 .. 4095
 *   ranks     int32 [D,H,W]: 0 for a zero voxel, otherwise 1 + the number of components whose root has a smaller linear
 *             index -- scipy.ndimage.label's numbering for the same adjacency.  Always the true rank, whatever cap is.
 *   count     int64 [2]: {components, components beyond cap}
 *   table     int64 [cap + 2][9], fully written.  Row r, 1 <= r <= cap: {root index, voxels, z0, y0, x0, z1, y1, x1
 *             (half-open), class byte at the root} of the component of rank r; all zeros when there is no such component.
 *             Row 0, the background: {-1, zero voxels, 0, 0, 0, D, H, W, 0} -- the box is the whole volume and there is no
 *             root.  Row cap + 1 collects every component of rank above cap: {-1, their voxels summed, the union of their
 *             boxes, -1}; all zeros when there is none.
 */
int cfun_cc_rank(const uint8_t* pred, const int32_t* labels, const int32_t* dims, int32_t cap, int32_t* ranks, int64_t* count,
                 int64_t* table, void* workspace, size_t workspace_bytes, cfun_stream_t stream);

/*
 * The contingency table of two rank volumes.
 *
 *   a, b      dense int32 [D,H,W] (what cfun_cc_rank wrote into ranks)
 *   overlap   int64 [cap_a + 2][cap_b + 2], fully written: cell [i][j] = voxels with min(a, cap_a + 1) == i and
 *             min(b, cap_b + 1) == j.  Row and column 0 are the backgrounds, the last row and column the overflow buckets
 *             (a negative value counts as overflow too).  The cells sum to D * H * W.
 *   workspace reserved: the pointer and size are not looked at
 *
 * Both entries return CFUN_EINVAL without launching when a dimension is negative, D * H * W >= 2^31 - 1 or a cap lies
 * outside 1 .. 4095; cfun_cc_rank returns CFUN_EWORKSPACE when the workspace is smaller than
 * cfun_lesion_workspace_bytes().  A volume with a zero dimension succeeds without a kernel launch; count, table and overlap
 * are then all zeros.
 */
int cfun_rank_overlap(const int32_t* a, const int32_t* b, const int32_t* dims, int32_t cap_a, int32_t cap_b, int64_t* overlap,
                      void* workspace, size_t workspace_bytes, cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
