// gh_inst_path.hip — explicit instantiations of the index-array moment and quantile kernels (gh_path.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_path.h"

GH_FOR_D(GH_PATH_KERNELS, template)
