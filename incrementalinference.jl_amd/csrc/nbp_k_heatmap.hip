// heatmap densities: the fixed-order scans, the pre-sample, weight and draw kernels (nbp_heatmap.h)
#define NBP_TU 32768
#include "nbp_heatmap.h"
