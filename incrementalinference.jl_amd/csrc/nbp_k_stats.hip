// belief statistics on resident slots: mean + covariance of a belief and the KL divergence of two beliefs (nbp_stats.h)
#define NBP_TU 8192
#include "nbp_stats.h"
