// gh_inst_grad5.hip — explicit instantiations of the gradient kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_GRAD_UNIT5(GH_TEMPLATE)
