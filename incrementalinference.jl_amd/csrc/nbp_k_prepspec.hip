// bandwidth fits + KD builds with the speculative search (launches that cannot fill the chip)
#define NBP_TU NBP_TU_PREPSPEC
#include "nbp_kernels.h"
