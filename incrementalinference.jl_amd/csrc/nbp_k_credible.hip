// credible regions of resident beliefs: HDR levels, credibility of reference points, coordinate quantiles (nbp_credible.h)
#define NBP_TU 128
#include "nbp_credible.h"
