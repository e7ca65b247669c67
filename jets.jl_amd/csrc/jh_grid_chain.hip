// jh_grid_chain.hip -- the FORWARD instantiations of k_grid_chain (jh_grid_chain_kernels.h: fused chains through an N x K grid), and the grid
// side of the chain handle: the checks jh_chain_create makes before it builds a grid chain.  ADJOINT and NORMAL live in jh_grid_chain_adj.hip and
// jh_grid_chain_nrm.hip, as the tall chains' do (build time).
#include "jh_grid_chain_kernels.h"

namespace jhb {
int grid_chain_launch_adjoint(const jh_chain *ch, int prog, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem);   // jh_grid_chain_adj.hip
int grid_chain_launch_normal(const jh_chain *ch, int prog, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem);    // jh_grid_chain_nrm.hip

// may jh_chain_create build a grid chain on `op`?  An N x K grid, N >= 2, K = 2 .. 4, of equal blocks of >= 16 bytes, every block a diagonal, an
// adjointed diagonal, a zero, an identity or a scalar (the kinds of k_grid_normal_mixed), no nonlinear child, coefficients aligned like their scalar;
// knob grid_chain = 1.  That is grid_shape_ok(op, true): an operator is tall only with one block column, and jh_blockop_create leaves all_diag set only
// where every block is a DIAG -- elementwise, linear, no wide scalar --, which is all that grid_shape_ok skips for plain diagonals
bool grid_chain_ok(const jh_blockop *op) { return jh_ctx().grid_chain != 0 && grid_shape_ok(op, true); }

// vectors aligned like their scalar (the under-aligned packs of jh_blockop_common.h take any such address)
bool grid_chain_vectors_ok(const jh_blockop *op, const void *a, const void *b) { return vectors_scalar_aligned(op->dtype, a, b) && op->coeff_scalar_aligned; }

// out = chain(in) for chain type `type` over program `prog` (GRID_PROG_OWN: the handle's own; GRID_PROG_ADJ / _NRM: derived from a FORWARD chain)
int grid_chain_launch(const jh_chain *ch, int prog, int type, void *out, const void *in, int accumulate)
{
    if (type == JH_CHAIN_ADJOINT) return grid_chain_launch_adjoint(ch, prog, out, in, accumulate, 0, -1);
    if (type == JH_CHAIN_NORMAL) return grid_chain_launch_normal(ch, prog, out, in, accumulate, 0, -1);
    return launch_grid_chain<0>(ch, prog, out, in, accumulate);
}

// the ADJOINT / NORMAL grid chain over the positions [first_elem, first_elem + count) of every block (jh_chain_apply_range, knob grid_chain_range; the
// caller has made the whole-vector call's checks and grid_range_bounds): the K pieces out_k[first_elem, first_elem + count) and nothing else
int grid_chain_launch_range(const jh_chain *ch, void *out, const void *in, int accumulate, int64_t first_elem, int64_t count)
{
    if (ch->type == JH_CHAIN_ADJOINT) return grid_chain_launch_adjoint(ch, GRID_PROG_OWN, out, in, accumulate, first_elem, first_elem + count);
    return grid_chain_launch_normal(ch, GRID_PROG_OWN, out, in, accumulate, first_elem, first_elem + count);
}
}  // namespace jhb
