// the overlap kernels: pair form, per-belief preparation, search (nbp_overlap.h)
#define NBP_TU 262144
#include "nbp_overlap.h"
