// the likelihood of factors under the resident beliefs of their variables: any number of items in one launch (nbp_likelihood.h)
#define NBP_TU NBP_TU_LIKELIHOOD
#include "nbp_likelihood.h"
