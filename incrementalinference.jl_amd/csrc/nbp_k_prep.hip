// bandwidth fits + KD builds, sequential golden-section search
#define NBP_TU NBP_TU_PREP
#include "nbp_kernels.h"
