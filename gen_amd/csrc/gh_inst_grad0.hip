// gh_inst_grad0.hip — explicit instantiations of the gradient kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_GRAD_KERNELS(template, gh::KitModel, gh::KitParams)
GH_GRAD_KERNELS(template, gh::RegModel, gh::RegParams)
GH_BIN_HEAVY0(GH_LG_EACH, GH_GRAD_KERNELS, template)
