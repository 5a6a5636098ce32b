// product kernels, latency geometries, any mix of manifolds (y32, l8)
#define NBP_TU NBP_TU_PRODLAT
#include "nbp_kernels.h"
