// the likelihood of factors under the resident beliefs of their variables: any number of items in one launch (nbp_likelihood.h)
#define NBP_TU 131072
#include "nbp_likelihood.h"
