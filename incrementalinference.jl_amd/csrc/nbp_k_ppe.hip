// point estimates of resident beliefs: manifold mean + the KDE's maximum among the belief's own points (nbp_ppe.h)
#define NBP_TU 2048
#include "nbp_ppe.h"
