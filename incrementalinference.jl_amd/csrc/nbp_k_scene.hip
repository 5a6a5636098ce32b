// scene densities: every belief of a list on one grid -- preparation, automatic extent, tiles (nbp_scene.h)
#define NBP_TU NBP_TU_SCENE
#include "nbp_scene.h"
