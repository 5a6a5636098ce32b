// product kernels, latency geometries (y32, l8), one manifold per instance
#define NBP_TU NBP_TU_PRODLATUNI
#include "nbp_kernels.h"
