// gh_inst_smooth6.hip — explicit instantiations of the backward-simulation kernels (gh_smooth.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_smooth.h"

GH_BIN_LIGHT_SL2(GH_SL_EACH, GH_BS_KERNELS, template)
