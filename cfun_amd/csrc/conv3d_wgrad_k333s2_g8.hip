// Weight-gradient kernels of this shape on the TD x 8 x 8 voxel tile (WgTile's G8): a translation unit of its own, so that
// the build compiles them beside the G16 instantiations.
#include "conv3d_mfma.h"

CFUN_WGRAD_DEFINE_G8(k333s2, 3, 3, 3, 2)
