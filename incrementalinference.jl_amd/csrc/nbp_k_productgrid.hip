// local products on a grid: a variable's factor messages on a regular grid -- extents, cells, normalisation (nbp_productgrid.h)
#define NBP_TU NBP_TU_PRODUCTGRID
#include "nbp_productgrid.h"
