// product kernels, throughput geometry, any mix of manifolds (t2)
#define NBP_TU 16
#include "nbp_kernels.h"
