// product kernels, latency geometries, any mix of manifolds (y32, l8)
#define NBP_TU 8
#include "nbp_kernels.h"
