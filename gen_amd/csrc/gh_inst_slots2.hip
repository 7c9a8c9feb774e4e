// gh_inst_slots2.hip — explicit instantiations of the slot family's kernels (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_BIN_SLOTS2(GH_SL_PLAIN, template)
