// proposal / deconv kernels and the small copy / reseed / resample kernels (see nbp_kernels.h, "Translation units")
#define NBP_TU NBP_TU_PROPOSAL
#include "nbp_kernels.h"
