// proposal kernels, two waves per proposal (see nbp_kernels.h, "Translation units")
#define NBP_TU NBP_TU_PROPSPLIT
#include "nbp_kernels.h"
