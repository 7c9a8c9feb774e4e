// gh_inst_smooth3.hip — explicit instantiations of the backward-simulation kernels (gh_smooth.h; see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_smooth.h"

GH_BS_UNIT3(template)
