// Gaussian-mixture summaries of resident beliefs: hierarchical EM on the kernel centres, all iterations in one launch (nbp_mixture.h)
#define NBP_TU NBP_TU_MIXTURE
#include "nbp_mixture.h"
