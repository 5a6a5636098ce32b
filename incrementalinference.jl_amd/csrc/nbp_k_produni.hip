// product kernels, throughput geometry, one manifold per instance (t2), two helper lanes per sample
#define NBP_TU NBP_TU_PRODUNI
#include "nbp_kernels.h"
