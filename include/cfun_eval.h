/*
 * cfun_eval.h -- the scoring entries of libcfun_hip.so: what the reference's test() (heart_main.py:286-360,
 * LiTS_2017/LiTS_main.py:285-367) computes through two float64 one-hot arrays and utils.compute_per_class_mask_iou /
 * compute_mask_iou (utils.py:580-617), as one pass over the two label volumes on the device.
 *
 * Why a header of its own: the same reason as cfun_sample.h.  These entries live in the same shared object as
 * cfun_hip.h's and follow the same conventions (device pointers, POD arguments, caller-owned workspace, stream as
 * void*, int return code, enqueue only), but cfun_hip.h is tied symbol for symbol to cfun_amd/_lib.py's EXPORTS table
 * and the guard tier accounts for that table inside its own two files.  The scoring entries are bound from a table of
 * their own, EVAL_SIGNATURES / EVAL_EXPORTS, in the same _lib.load(); tests/test_eval_emu.py and
 * tests/test_eval_gpu.py carry the header-equals-table check and the ran-under-guard check for this table.
 *
 * Nothing here synchronises or reads device memory on the host.
 */
#ifndef CFUN_EVAL_H
#define CFUN_EVAL_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace cfun_seg_confusion needs for a [D,H,W] volume and K classes (0 when a dimension is 0). */
size_t cfun_seg_confusion_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K);

/*
 * The confusion counts of a predicted class map against a label volume.
 *
 *   pred            dense uint8 [D,H,W] (x fastest): what cfun_unmold_argmax / cfun_unmold_overlap write
 *   label           the label volume of the same logical extent, read in place; label_dtype 0 = uint8, 1 = int32
 *   label_strides   element strides {sD, sH, sW} of the logical [D,H,W] index into label.  sD == 1 (the loader's
 *                   [H,W,D] array seen as a [D,H,W] view) or sH == 1 (the same array in Fortran order, as a NIfTI
 *                   file stores it) takes the tiled kernel that reads both volumes along their own fastest axis;
 *                   any other stride set (a dense [D,H,W] label, a sliced view) is indexed directly
 *   dims            {D, H, W}
 *   K               NUM_CLASSES, 1..15
 *   counts          int64 [(K+1)][(K+1)]: counts[g][p] = voxels with label class g and predicted class p.  A label or
 *                   prediction value outside [0, K) -- negative, or >= K -- counts in the extra row / column K
 *                   ("other"), so every voxel lands in exactly one cell and the sum of counts is D * H * W.
 *                   Fully written by every successful call; all zeros when a dimension is 0.
 *
 * Returns CFUN_EINVAL without launching when D * H * W >= 2^31, K is out of range or label_dtype is unknown,
 * CFUN_EWORKSPACE when the workspace is smaller than cfun_seg_confusion_workspace_bytes().  Results are integers summed
 * without global atomics: every run gives the same bits.
 */
int cfun_seg_confusion(const uint8_t* pred, const void* label, int32_t label_dtype, const int64_t* label_strides,
                       const int32_t* dims, int32_t K, int64_t* counts, void* workspace, size_t workspace_bytes,
                       cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
