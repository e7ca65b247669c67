// jh_grid_chain_adj.hip -- the ADJOINT instantiations of k_grid_chain (jh_grid_chain_kernels.h), a translation unit of their own (build time: see
// jh_tall_chain.hip).
#include "jh_grid_chain_kernels.h"

namespace jhb {
// end_elem < 0: the whole block; else the positions [first_elem, end_elem) of every block (jh_chain_apply_range, knob grid_chain_range)
int grid_chain_launch_adjoint(const jh_chain *ch, int prog, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem)
{
    return launch_grid_chain<1>(ch, prog, out, in, accumulate, first_elem, end_elem);
}
}  // namespace jhb
