// jh_tall_chain_adj.hip -- the ADJOINT  m = Q(sum_i conj(a_i) .* R(d_i)) instantiations of k_chain_adj (jh_tall_chain_kernels.h), a translation unit of their own
// (build time: see jh_tall_chain.hip).
#include "jh_tall_chain_kernels.h"

namespace jhb {
int chain_launch_adjoint(const jh_chain *ch, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem, const ChainArgs *ca)
{
    const ChainArgs &args = ca ? *ca : ch->args;
    const jh_blockop *op = ch->op;
    const int64_t n = op->row_len[0];
    return jh_by_dtype(op->dtype, "chain_launch_adjoint", [&](auto t) {
        using T = decltype(t);
        return launch_chain_adj<typename T::S, T::E, T::NS, 0>(ch, args, out, in, n * T::E, accumulate, first_elem * T::E, end_elem * T::E);
    });
}

// out = accumulate(out, Q(folded)) over the scalars [s_begin, s_end) of a domain vector: the split walk's last step, for the grid chains too
int chain_finish(const jh_chain *ch, const ChainArgs &ca, void *out, const void *folded, int64_t s_begin, int64_t s_end, int accumulate)
{
    jh_context &c = jh_ctx();
    return jh_by_dtype(ch->op->dtype, "chain_finish", [&](auto t) -> int {
        using T = decltype(t);
        using S = typename T::S;
        constexpr int NS = T::NS;
        hipLaunchKernelGGL((k_chain_finish<S, T::E, NS>), dim3((unsigned)(((s_end - s_begin + NS - 1) / NS + 255) / 256)), dim3(256), 0, c.stream, ca, (S *)out,
                           (const S *)folded, s_begin, s_end, accumulate);
        JH_CHECK_HIP(hipGetLastError());
        return JH_OK;
    });
}
}  // namespace jhb
