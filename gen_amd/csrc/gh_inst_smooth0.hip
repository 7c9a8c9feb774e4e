// gh_inst_smooth0.hip — explicit instantiations of the backward-simulation kernels (gh_smooth.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_smooth.h"

GH_BS_KERNELS(template, gh::HMMModel, gh::HMMParams)
GH_BS_KERNELS(template, gh::KitModel, gh::KitParams)
GH_BIN_LIGHT_LG0(GH_LG_EACH, GH_BS_KERNELS, template)
