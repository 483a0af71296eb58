/* Tile queries of the convolution kernels: forward / data gradient and weight gradient (the same shared object as cfun_hip.h).
 *
 * A header of its own, like cfun_sample.h: the entries of cfun_hip.h are tied one to one to cfun_amd/_lib.py's EXPORTS and
 * to the guard tier's account of them (tests/guard.py lists the host-side queries by name); this one launches nothing and
 * is bound through _lib.TILE_SIGNATURES. */
#ifndef CFUN_TILE_H
#define CFUN_TILE_H

#include "cfun_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The output tile {z, y, x} of the workgroups cfun_conv3d_fwd runs for p given its full workspace: {4, 4, 16} or {4, 8, 8}
 * (CFUN_ALGO_TILE_* in p->algo, CFUN_TILE_GEOM, or the library's rule -- conv3d.hip).  The data gradient of a stride-1 conv
 * is the forward of its mirrored parameter set and follows the same rule on ITS output grid.
 * Returns 0, or CFUN_EINVAL if p does not run on the MFMA / Winograd kernels (CFUN_KERNEL_MFMA / _WINO). */
int cfun_conv3d_fwd_tile(const CfunConv3dParams* p, int32_t out[3]);

/* The voxel tile {z, y, x} of the workgroups cfun_conv3d_bwd_weight runs for p: {2, 4, 16} or {2, 8, 8} ({1, ...} at stride 2),
 * by the same flags, knob and rule on the grid the weight gradient tiles (p->Do/Ho/Wo; the low-resolution grid of a folded /
 * depth-to-space conv).  {.., 4, 16} where no 8 x 8 instantiation exists (the opt-in 2-D Winograd kernel, 1x3x3, 5x5x5 ...).
 * Returns 0, or CFUN_EINVAL if the weight gradient of p does not run on the MFMA / Winograd weight-gradient kernels. */
int cfun_conv3d_wgrad_tile(const CfunConv3dParams* p, int32_t out[3]);

/* Which kernel family runs the two gradients of p given their full workspaces: out = {cfun_conv3d_bwd_data,
 * cfun_conv3d_bwd_weight*}, the counterpart of cfun_conv3d_fwd_kernel, answered by the predicates the launches ask.
 * Returns 0, or CFUN_EINVAL for parameters the library refuses. */
#define CFUN_BWD_DIRECT 0      /* generic VALU kernels (conv3d_direct.hip); under CFUN_ALGO_MFMA the weight gradient refuses instead */
#define CFUN_BWD_MFMA 1        /* data gradient: k_conv_mfma on the mirrored conv; weight gradient: k_wgrad_mfma / k_wgrad_fused */
#define CFUN_BWD_WINO 2        /* k_conv_wino on the mirrored conv / k_wgrad_wino */
#define CFUN_BWD_S2FOLD 3      /* data gradient of a 3x3x3 stride-2 conv as one folded 2x2x2 conv with a depth-to-space epilogue */
#define CFUN_BWD_C1 4          /* weight gradient of the C_in = 1 stems (k_wgrad_c1_mfma) */
int cfun_conv3d_bwd_kernels(const CfunConv3dParams* p, int32_t out[2]);

#ifdef __cplusplus
}
#endif

#endif
