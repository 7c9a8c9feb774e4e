// gh_inst_grad6.hip — explicit instantiations of the gradient kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_BIN_HEAVY6(GH_LG_EACH, GH_GRAD_KERNELS, template)
