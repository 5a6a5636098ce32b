// marginal densities of resident beliefs: on a grid over a subset of the coordinates and at query points (nbp_marginal.h)
#define NBP_TU NBP_TU_MARGINAL
#include "nbp_marginal.h"
