// jh_grid_common.h -- what the one-pass kernels over an N x K GRID of equal elementwise blocks share (jh_grid_normal.hip: the fused A'A,
// jh_grid_step.hip: the Golub-Kahan step): the packed block table of a grid of several kinds -- one 64-bit word per block, row-major,
// pointer | kind << 48 | adjoint << 51 | real scalar << 52 -- and the child mul! of one block on a pack from its word.
#pragma once
#include "jh_blockop_common.h"

namespace {

constexpr uint64_t GW_PTR = (((uint64_t)1) << 48) - 1;
__device__ inline int gw_kind(uint64_t w) { return (int)((w >> 48) & 7u); }
__device__ inline bool gw_adj(uint64_t w) { return ((w >> 51) & 1u) != 0; }
__device__ inline bool gw_real(uint64_t w) { return ((w >> 52) & 1u) != 0; }

// child mul! of block `idx` on a pack (jh_blockop_common.h: apply_block_loaded, on the block's table word; scalars from the block table)
template <typename S, int E, int NS, typename V>
__device__ inline V grid_apply(uint64_t w, const jh_dev_block *blocks, int64_t idx, V x, V c, bool transposed)
{
    const bool cj = gw_adj(w) != transposed;
    switch (gw_kind(w)) {
    case JH_OP_DIAG: return vmul<S, E, NS, V>(c, x, cj);
    case JH_OP_IDENTITY: return x;
    case JH_OP_SCALE: {
        const double sre = blocks[idx].sre;
        if (E == 1 || gw_real(w)) return (V)(S)sre * x;
        const double sim = blocks[idx].sim;
        V a;
#pragma unroll
        for (int q = 0; q < NS; q += 2) { a[q] = (S)sre; a[q + 1] = (S)sim; }
        return vmul<S, E, NS, V>(a, x, cj);
    }
    default: return (V)(S)0;
    }
}

}  // namespace

namespace jhb {
// ---- jh_grid_normal.hip
bool grid_shape_ok(const jh_blockop *op, bool mixed_ok);   // N >= 2, K = 2 .. 4, equal blocks of >= 16 bytes of the kinds above (mixed_ok: not only plain diagonals), aligned coefficients
int grid_words_ensure(const jh_blockop *op);               // the packed table of a mixed grid (op->grid_words), built on first use (not inside a stream capture)
}  // namespace jhb
