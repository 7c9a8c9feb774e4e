// gh_inst_slots4.hip — explicit instantiations of the slot family's kernels for models with a library slot or the switching latent (see gh_inst.h)
#include <hip/hip_runtime.h>
#include "gh_inst.h"

GH_BIN_SLOTS0(GH_SL_EXT, template)
