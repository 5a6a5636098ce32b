// heatmap densities: the fixed-order scans, the pre-sample, weight and draw kernels (nbp_heatmap.h)
#define NBP_TU NBP_TU_HEATMAP
#include "nbp_heatmap.h"
