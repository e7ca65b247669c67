// jh_tall_chain_adj.hip -- the ADJOINT  m = Q(sum_i conj(a_i) .* R(d_i)) instantiations of k_chain_adj (jh_tall_chain_kernels.h), a translation unit of their own
// (build time: see jh_tall_chain.hip).
#include "jh_tall_chain_kernels.h"

namespace jhb {
int chain_launch_adjoint(const jh_chain *ch, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem, const ChainArgs *ca)
{
    const ChainArgs &args = ca ? *ca : ch->args;
    const jh_blockop *op = ch->op;
    const int64_t n = op->row_len[0];
    switch (op->dtype) {
    case JH_F32: return launch_chain_adj<float, 1, 4, 0>(ch, args, out, in, n, accumulate, first_elem, end_elem);
    case JH_F64: return launch_chain_adj<double, 1, 2, 0>(ch, args, out, in, n, accumulate, first_elem, end_elem);
    case JH_C32: return launch_chain_adj<float, 2, 4, 0>(ch, args, out, in, n * 2, accumulate, first_elem * 2, end_elem * 2);
    case JH_C64: return launch_chain_adj<double, 2, 2, 0>(ch, args, out, in, n * 2, accumulate, first_elem * 2, end_elem * 2);
    }
    return jh_fail(JH_ERR_INVALID, "chain_launch_adjoint: unknown dtype %d", op->dtype);
}

// out = accumulate(out, Q(folded)) over the scalars [s_begin, s_end) of a domain vector: the split walk's last step, for the grid chains too
int chain_finish(const jh_chain *ch, const ChainArgs &ca, void *out, const void *folded, int64_t s_begin, int64_t s_end, int accumulate)
{
    jh_context &c = jh_ctx();
#define JH_FINISH(S, E, NS)                                                                                                                  \
    hipLaunchKernelGGL((k_chain_finish<S, E, NS>), dim3((unsigned)(((s_end - s_begin + NS - 1) / NS + 255) / 256)), dim3(256), 0, c.stream, ca, (S *)out, \
                       (const S *)folded, s_begin, s_end, accumulate)
    switch (ch->op->dtype) {
    case JH_F32: JH_FINISH(float, 1, 4); break;
    case JH_F64: JH_FINISH(double, 1, 2); break;
    case JH_C32: JH_FINISH(float, 2, 4); break;
    case JH_C64: JH_FINISH(double, 2, 2); break;
    default: return jh_fail(JH_ERR_INVALID, "chain_finish: unknown dtype %d", ch->op->dtype);
    }
#undef JH_FINISH
    JH_CHECK_HIP(hipGetLastError());
    return JH_OK;
}
}  // namespace jhb
