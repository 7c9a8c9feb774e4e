// gh_inst_quantiles.hip — explicit instantiations of the weighted-quantile kernels (gh_quantiles.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_quantiles.h"

GH_FOR_D(GH_QT_KERNELS, template)
