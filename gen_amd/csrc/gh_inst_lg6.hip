// gh_inst_lg6.hip — explicit instantiations of LG-SSM kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_BIN_HEAVY6(GH_LG_DIM, template)
