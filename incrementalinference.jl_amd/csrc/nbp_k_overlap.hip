// the overlap kernels: pair form, per-belief preparation, search (nbp_overlap.h)
#define NBP_TU NBP_TU_OVERLAP
#include "nbp_overlap.h"
