// jh_tall_chain_step.hip -- the Golub-Kahan step of a FORWARD chain  u_i <- alpha R(a_i .* P(v)) + beta u_i ; w = Q(sum_i conj(a_i) .* R^H(u_i)) ; ||u||^2
// (MODE 2 of k_chain_adj, jh_tall_chain_kernels.h), a translation unit of its own (build time: see jh_tall_chain.hip).
#include "jh_tall_chain_kernels.h"

namespace jhb {
// the domain's elements [first_elem, end_elem): the whole vector (jh_chain_bidiag_step) or one exchange range (jh_chain_bidiag_step_range) -- those
// columns of every row of u, that range of w, that range's share of ||u||^2.  The bounds are kernel ARGUMENTS (s_begin, s_end of k_chain_adj, as for the
// ranged ADJOINT / NORMAL chains): the ranged step runs the whole-vector step's instantiations.  defer: normsq NULL adds the share to the deferred
// accumulator (jh_normsq_reset / jh_normsq_read) instead of dropping it.
int chain_launch_step(const jh_chain *ch, const ChainArgs &ca, void *u, const void *v, void *w, double alpha, double beta, double *normsq,
                      int64_t first_elem, int64_t end_elem, bool defer)
{
    const jh_blockop *op = ch->op;
    const int64_t n = op->row_len[0], lo = first_elem, hi = end_elem;
    ChainStep st;
    st.u = u;
    st.alpha = alpha;
    st.beta = beta;
    st.normsq = normsq;
    st.defer = defer;
    return jh_by_dtype(op->dtype, "chain_launch_step", [&](auto t) {
        using T = decltype(t);
        return launch_chain_adj<typename T::S, T::E, T::NS, 2>(ch, ca, w, v, n * T::E, 0, lo * T::E, hi * T::E, &st);
    });
}
}  // namespace jhb
