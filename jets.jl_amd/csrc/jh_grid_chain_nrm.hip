// jh_grid_chain_nrm.hip -- the NORMAL instantiations of k_grid_chain (jh_grid_chain_kernels.h), a translation unit of their own (build time: see
// jh_tall_chain.hip).
#include "jh_grid_chain_kernels.h"

namespace jhb {
int grid_chain_launch_normal(const jh_chain *ch, int prog, void *out, const void *in, int accumulate)
{
    return launch_grid_chain<2>(ch, prog, out, in, accumulate);
}
}  // namespace jhb
