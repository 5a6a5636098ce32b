// belief statistics on resident slots: mean + covariance of a belief and the KL divergence of two beliefs (nbp_stats.h)
#define NBP_TU NBP_TU_STATS
#include "nbp_stats.h"
