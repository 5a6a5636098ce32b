// proposal kernels, two waves per proposal (see nbp_kernels.h, "Translation units")
#define NBP_TU 524288
#include "nbp_kernels.h"
