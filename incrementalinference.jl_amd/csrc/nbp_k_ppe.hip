// point estimates of resident beliefs: manifold mean + the KDE's maximum among the belief's own points (nbp_ppe.h)
#define NBP_TU NBP_TU_PPE
#include "nbp_ppe.h"
