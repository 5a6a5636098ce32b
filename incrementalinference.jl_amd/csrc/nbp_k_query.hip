// belief queries on resident slots: the KDE's density at query points and the mmd of two beliefs (nbp_query.h)
#define NBP_TU NBP_TU_QUERY
#include "nbp_query.h"
