// gh_inst_ancestor6.hip — explicit instantiations of the ancestor-sampling score kernel (gh_ancestor.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_ancestor.h"

GH_BIN_LIGHT_SL2(GH_SL_EACH, GH_AS_KERNELS, template)
