// product kernels, throughput geometry, any mix of manifolds (t2)
#define NBP_TU NBP_TU_PRODTHR
#include "nbp_kernels.h"
