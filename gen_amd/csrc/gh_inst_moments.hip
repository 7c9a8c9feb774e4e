// gh_inst_moments.hip — explicit instantiations of the weighted-moment kernels (gh_moments.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_moments.h"

GH_FOR_D(GH_EST_KERNELS, template)
