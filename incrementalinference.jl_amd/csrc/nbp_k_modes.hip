// the modes of resident beliefs: mean-shift from every point of a belief, merging and ranking in one launch (nbp_modes.h)
#define NBP_TU NBP_TU_MODES
#include "nbp_modes.h"
