// jh_tall_chain_nrm.hip -- the NORMAL  y = Q(sum_i conj(a_i) .* R(a_i .* P(m))) instantiations of k_chain_adj (jh_tall_chain_kernels.h), a translation unit of their own
// (build time: see jh_tall_chain.hip).
#include "jh_tall_chain_kernels.h"

namespace jhb {
int chain_launch_normal(const jh_chain *ch, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem, const ChainArgs *ca)
{
    const ChainArgs &args = ca ? *ca : ch->args;
    const jh_blockop *op = ch->op;
    const int64_t n = op->row_len[0];
    return jh_by_dtype(op->dtype, "chain_launch_normal", [&](auto t) {
        using T = decltype(t);
        return launch_chain_adj<typename T::S, T::E, T::NS, 1>(ch, args, out, in, n * T::E, accumulate, first_elem * T::E, end_elem * T::E);
    });
}
}  // namespace jhb
