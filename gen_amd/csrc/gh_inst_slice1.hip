// gh_inst_slice1.hip — explicit instantiations of the slice and map_optimize kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_BIN_HEAVY1(GH_LG_EACH, GH_SLICE_KERNELS, template)
