// gh_inst_slice0.hip — explicit instantiations of the slice and map_optimize kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_SLICE_KERNELS(template, gh::KitModel, gh::KitParams)
GH_SLICE_KERNELS(template, gh::RegModel, gh::RegParams)
GH_BIN_HEAVY0(GH_LG_EACH, GH_SLICE_KERNELS, template)
