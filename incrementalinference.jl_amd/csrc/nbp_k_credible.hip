// credible regions of resident beliefs: HDR levels, credibility of reference points, coordinate quantiles (nbp_credible.h)
#define NBP_TU NBP_TU_CREDIBLE
#include "nbp_credible.h"
