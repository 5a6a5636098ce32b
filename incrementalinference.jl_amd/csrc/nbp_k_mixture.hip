// Gaussian-mixture summaries of resident beliefs: hierarchical EM on the kernel centres, all iterations in one launch (nbp_mixture.h)
#define NBP_TU 1048576
#include "nbp_mixture.h"
