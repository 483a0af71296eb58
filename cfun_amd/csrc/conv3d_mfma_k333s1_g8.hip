// the 4 x 8 x 8 output tile (G8) of the k333s1 forward / data-gradient kernels (see conv3d_mfma.h)
#include "conv3d_mfma.h"

CFUN_MFMA_DEFINE_G8(k333s1, 3, 3, 3, 1)
