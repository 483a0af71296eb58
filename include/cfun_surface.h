/*
 * cfun_surface.h -- surface distances between two class maps on the device: the surface voxels of a class, the exact squared
 * Euclidean distance field of a surface under an anisotropic voxel spacing, and per class the statistics behind Hausdorff,
 * HD95, ASSD and RMSD.  The reference has no such function, so nothing here is pinned by it: the pin is the brute-force
 * restatement of the definitions below on the host (tests/surface_ref.py), scipy.ndimage.distance_transform_edt and
 * hand-written known answers (tests/test_surface_ref.py).
 *
 * Why a header of its own: the same reason as cfun_sample.h, cfun_eval.h and cfun_cc.h.  These entries live in the same shared
 * object as cfun_hip.h's and follow the same conventions (device pointers, POD arguments, caller-owned workspace, stream as
 * void*, int return code, enqueue only), but cfun_hip.h is tied symbol for symbol to cfun_amd/_lib.py's EXPORTS table.  These
 * are bound from a table of their own, SURFACE_SIGNATURES / SURFACE_EXPORTS, in the same _lib.load(); tests/test_surface_emu.py
 * and tests/test_surface_gpu.py carry the header-equals-table check and the ran-under-guard check for this table.
 *
 * Definitions.
 *
 *   Surface S_c(M) of class c in a dense uint8 map M[D,H,W]: the voxels with M == c that have at least one of their six face
 *   neighbours outside the volume or != c (a voxel on a face of the volume is surface).
 *
 *   Squared distance field of a surface S with spacing squares (sz2, sy2, sx2), each the float32 of the double product of a
 *   spacing with itself, formed on the host.  All of it float32, operation for operation, no FMA contraction; k = the index
 *   difference along the axis of the sweep, float(k * k) exact (every dimension is <= 4096):
 *       g1[z,y,x] = min over surface voxels x' of the row   of fl(float(k * k) * sx2)          (+inf: the row holds none)
 *       g2[z,y,x] = min over y'                             of fl(g1[z,y',x] + fl(float(k * k) * sy2))
 *       g3[z,y,x] = min over z'                             of fl(g2[z',y,x] + fl(float(k * k) * sz2))
 *   A minimum does not depend on the order of evaluation and the float32 rounding is monotone, so a scan that skips only
 *   candidates with fl(float(k * k) * a2) >= the best so far yields the same bits as the full scan: the field is bit-identical
 *   to the brute-force restatement.
 *
 * Nothing here synchronises or reads device memory on the host.
 */
#ifndef CFUN_SURFACE_H
#define CFUN_SURFACE_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One row of cfun_surface_stats' result: class c of the prediction (A = S_c(pred)) against the label (B = S_c(label)).
 * "pl" is measured at A's voxels in B's field (prediction -> label), "lp" the reverse; d = sqrt(double(d2)).
 *
 *   n_pred, n_label        |A|, |B|
 *   sum_pl, sum_lp         the sums of d
 *   sumsq_pl, sumsq_lp     the sums of double(d2)
 *   max_sq_pl, max_sq_lp   the largest float32 d2, widened
 *   q_lo_sq, q_hi_sq, frac the percentile by the linear rule on the concatenation of both directed sets: with n = |A| + |B|,
 *                          pos = double(n - 1) * qf, lo = floor(pos), hi = min(lo + 1, n - 1), frac = pos - lo; q_lo_sq and
 *                          q_hi_sq are the float32 d2 of ranks lo and hi (exact order statistics, equal values counted with
 *                          multiplicity), widened.  The percentile distance is (1 - frac) * sqrt(q_lo_sq) + frac * sqrt(q_hi_sq).
 *
 * When n_pred == 0 or n_label == 0 every floating field of the row is 0 and the counts are what they are.
 */
typedef struct CfunSurfaceStats {
  int64_t n_pred, n_label;
  double sum_pl, sum_lp, sumsq_pl, sumsq_lp, max_sq_pl, max_sq_lp, q_lo_sq, q_hi_sq, frac;
} CfunSurfaceStats;

/*
 * Bytes of workspace cfun_surface_stats needs for two [D,H,W] maps and K classes: two byte surfaces and two float32 fields
 * (10 bytes per voxel), the partial sums and the selection histograms (0 when a dimension is 0, or when the arguments are
 * ones the entries reject).  cfun_surface_field needs none.
 */
size_t cfun_surface_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K);

/*
 * The surface of one class of one map, and that surface's squared distance field.
 *
 *   map             dense uint8 [D,H,W] (x fastest)
 *   dims            {D, H, W}
 *   cls             1 .. 255
 *   spacing2        {sz2, sy2, sx2}: finite and positive
 *   surface_out     uint8 [D,H,W]: 1 on S_cls(map), else 0
 *   field_out       float32 [D,H,W]: g3 as defined above; +inf everywhere when the surface is empty
 *   workspace       reserved: the sweeps work in place in field_out; the pointer and size are not looked at
 */
int cfun_surface_field(const uint8_t* map, const int32_t* dims, int32_t cls, const float* spacing2, uint8_t* surface_out,
                       float* field_out, void* workspace, size_t workspace_bytes, cfun_stream_t stream);

/*
 * The statistics of every class 1 .. K-1 of pred against label, both dense uint8 [D,H,W]; bytes >= K belong to no class.
 *
 *   qf              the percentile as a fraction, q / 100 formed on the host, in [0, 1]
 *   stats           CfunSurfaceStats [K], fully written by every successful call; row 0 is all zeros
 *
 * The classes are taken one after another on the one stream and share the workspace.  Sums are accumulated in fp64 per
 * workgroup and added in a fixed order, counts and histograms are integers: every run gives the same bits.
 *
 * Both entries return CFUN_EINVAL without launching when a dimension is negative or above 4096, D * H * W >= 2^31 - 1, K is
 * outside 1 .. 15, cls is outside 1 .. 255, a spacing square is not finite and positive or qf is outside [0, 1];
 * cfun_surface_stats returns CFUN_EWORKSPACE when the workspace is smaller than cfun_surface_workspace_bytes().  A volume
 * with a zero dimension succeeds without a kernel launch; stats is then all zeros.
 */
int cfun_surface_stats(const uint8_t* pred, const uint8_t* label, const int32_t* dims, int32_t K, const float* spacing2,
                       double qf, CfunSurfaceStats* stats, void* workspace, size_t workspace_bytes, cfun_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
