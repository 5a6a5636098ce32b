// proposal kernels, one wave per proposal (see nbp_kernels.h, "Translation units")
#define NBP_TU NBP_TU_PROPWAVE
#include "nbp_kernels.h"
