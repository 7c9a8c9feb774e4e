// gh_inst_grad1.hip — explicit instantiations of the gradient kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_GRAD_UNIT1(GH_TEMPLATE)
