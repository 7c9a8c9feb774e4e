// gh_inst_forecast1.hip — explicit instantiations of the forecast kernels (gh_forecast.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_forecast.h"

GH_BIN_LIGHT_LG1(GH_LG_EACH, GH_FC_KERNELS, template)
