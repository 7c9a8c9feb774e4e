// gh_inst_slots1.hip — explicit instantiations of the slot family's kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_BIN_SLOTS1(GH_SL_PLAIN, template)
