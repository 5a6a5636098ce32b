// product kernels, latency geometries (y32, l8), one manifold per instance
#define NBP_TU 1024
#include "nbp_kernels.h"
