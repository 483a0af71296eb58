/*
 * cfun_sample.h -- the training-sample entries of libcfun_hip.so: what the reference's load_image_gt
 * (model.py:1007-1181; LiTS_2017/model.py:1010-1032) does on the host per step, on the device.
 *
 * Why a header of its own: these entries live in the same shared object as cfun_hip.h's and follow the
 * same conventions (device pointers, POD arguments, caller-owned workspace, stream as void*, int return
 * code, enqueue only), but cfun_hip.h is tied symbol for symbol to cfun_amd/_lib.py's EXPORTS table, and
 * the guard tier demands that every entry of that table ran under guard inside its own two files.  The
 * sample entries are therefore declared here and bound from a second table, SAMPLE_SIGNATURES /
 * SAMPLE_EXPORTS, in the same _lib.load(); tests/test_sample_emu.py and tests/test_sample_gpu.py carry
 * the header-equals-table check and the ran-under-guard check for this table.
 *
 * Nothing here synchronises or reads device memory on the host.
 */
#ifndef CFUN_SAMPLE_H
#define CFUN_SAMPLE_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of workspace the two launching entries below need: the larger of the rotate pass on an [H,W,D]
 * volume and the RPN targets of A anchors against G boxes.  A group that is not used may be passed as zeros.
 */
size_t cfun_sample_workspace_bytes(int32_t H, int32_t W, int32_t D, int32_t A, int32_t G);

/*
 * Per-slice nearest-neighbour rotation of image and label, the [H,W,D] -> [D,H,W] re-layout, the label
 * cast and the GT box, in one pass over the volume plus one small finish launch.
 *
 *   image / label     float32 / int32 volumes of extent dims = {H, W, D}, read in place through their
 *                     element strides {sH, sW, sD} (as cfun_resize3d reads its source)
 *   cos_t, sin_t      of the rotation angle, computed by the caller in double
 *   rotate            0: no rotation (the LiTS form; bit-identical to angle 0), else the rule below
 *   out_image         dense float32 [D,H,W];  out_label: dense uint8 [D,H,W]
 *   raw_box           int32[6] (z1,y1,x1,z2,y2,x2) by utils.extract_bboxes: min and max + 1 over label > 0 --
 *                     all zeros when z1 == z2 (the reference's one-plane quirk), and when the label is empty
 *   box               int32[6]: raw_box expanded by 5 % per side and clamped (model.py:1059-1075, extend_bbox):
 *                     in double, z1 - depth * 0.05, floor(max(0, .)), ceil(min(dim, .))
 *   empty             int32: 1 when no voxel has label > 0 (the reference raises there), else 0
 *
 * Rule (double, this operation order; cy = H / 2 - 0.5, cx = W / 2 - 0.5):
 *   sx =  c * (x - cx) + s * (y - cy) + cx        ix = floor(sx + 0.5)
 *   sy = -s * (x - cx) + c * (y - cy) + cy        iy = floor(sy + 0.5)
 *   out[z,y,x] = in[iy,ix,z] when 0 <= ix < W and 0 <= iy < H, else 0; one (iy,ix) serves image and label.
 *
 * Preconditions (the caller's): label values lie in [0, 255]; both volumes have the extent dims; H <= 65535.
 * The Python wrapper always checks the shapes and H; the label range it checks only with strict=True, because
 * that check reads back from the device.  Outside the range nothing faults but the outputs disagree: out_label
 * keeps the low 8 bits while the box counts `label > 0` on the untruncated value (256 is stored as 0 yet counts
 * towards the box; a negative label is stored non-zero and is left out of the box).
 */
int cfun_sample_rotate_bbox(const float* image, const int64_t* image_strides, const int32_t* label,
                            const int64_t* label_strides, const int32_t* dims, double cos_t, double sin_t, int32_t rotate,
                            float* out_image, uint8_t* out_label, int32_t* raw_box, int32_t* box, int32_t* empty,
                            void* workspace, size_t workspace_bytes, cfun_stream_t stream);

/*
 * build_rpn_targets (model.py:1090-1181) for one image.
 *
 *   anchors [A,6], gt_boxes [G,6]   float32 (z1,y1,x1,z2,y2,x2), same units
 *   keys [A]                        uint32: the deterministic stand-in for the reference's two np.random.choice draws
 *   R                               RPN_TRAIN_ANCHORS_PER_IMAGE
 *   std_dev                         HOST pointer to the six RPN_BBOX_STD_DEV as doubles (read before return)
 *   neg_iou, pos_iou                0.3 and 0.7 in the reference
 *   rpn_match                       int32 [A]: 1 positive, -1 negative, 0 neutral
 *   rpn_bbox                        float32 [R,6]: the deltas of the kept positives in ascending anchor order, other rows 0
 *   counts                          int32[2]: positives kept, negatives kept
 *
 * IoU in double with + 1e-6 in the denominator.  Negatives (max IoU < neg_iou) first; then every GT's best
 * anchor positive whatever its IoU (first index wins a tie); then max IoU >= pos_iou positive; deltas against
 * the anchor's arg-max GT (first GT wins a tie).  Of the positives the R / 2 smallest in (key, index) order
 * stay, of the negatives the R - positives_kept smallest; the rest go neutral.
 * A == 0 or G == 0: nothing is launched and nothing written.
 */
int cfun_sample_rpn_targets(const float* anchors, int32_t A, const float* gt_boxes, int32_t G, const uint32_t* keys,
                            int32_t R, const double* std_dev, double neg_iou, double pos_iou, int32_t* rpn_match,
                            float* rpn_bbox, int32_t* counts, void* workspace, size_t workspace_bytes,
                            cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
