// jh_grid_common.h -- what the one-pass kernels over an N x K GRID of equal elementwise blocks share (jh_grid_normal.hip: the fused A'A,
// jh_grid_step.hip: the Golub-Kahan step): the packed block table of a grid of several kinds -- one 64-bit word per block, row-major,
// pointer | kind << 48 | adjoint << 51 | real scalar << 52 --, the child mul! of one block on a pack from its word, and the launchers' plan (GridPlan).
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

// THE LAUNCH PLAN of the one-pass grid kernels (A'A, the ranged adjoint, the step, the grid chains and their step).  The lanes cover the scalars
// [s_begin, s_end) of a block in gx workgroups of 256 packs -- end_elem < 0: the whole block; else the positions [first_elem, end_elem) of every block,
// launched as a vector of its own length -- on (gx, parts) workgroups: the part rule of the tall chains over the RANGE's workgroups (pick_row_parts;
// tolerance parity, adj_split = 0 keeps the ordered walk).  n_scalars stays the stride of the pieces of the vectors and of the slabs.
// What the launchers keep for themselves: the bytes their nontemporal rule sees, the counters they write, and the order of their checks.
struct GridPlan {
    int64_t n_scalars, s_begin, s_end, gx, parts, rows_per_part;
    bool ranged;
};
// the lanes alone, in one part (the FORWARD grid chain: not a reduction, its part rule is its own)
inline GridPlan grid_lanes(const jh_blockop *op, int E, int NS, int64_t first_elem, int64_t end_elem)
{
    const bool ranged = end_elem >= 0;
    const int64_t n_scalars = op->row_len[0] * E, s_begin = ranged ? first_elem * E : 0, s_end = ranged ? end_elem * E : n_scalars;
    return {n_scalars, s_begin, s_end, ((s_end - s_begin + NS - 1) / NS + 255) / 256, 1, op->nrow, ranged};
}
inline GridPlan grid_plan(const jh_blockop *op, int E, int NS, int64_t first_elem, int64_t end_elem)
{
    GridPlan p = grid_lanes(op, E, NS, first_elem, end_elem);
    const RowParts r = jhb::pick_row_parts(p.s_end - p.s_begin, NS, p.gx, op->nrow);
    p.parts = r.parts;
    p.rows_per_part = r.rows_per_part;
    return p;
}
// the split walk's slabs (NULL: one part) -- parts x K x n_scalars: the whole block's stride, of which a range touches its share (the kernels then need
// no second stride; the split walk is the regime of small blocks, where that is little memory) --, plus the folded slab when a stage follows the fold
template <typename S> int grid_slabs(const GridPlan &p, int K, void *out, S **slabs, bool finish = false)
{
    *slabs = nullptr;
    if (p.parts == 1) return JH_OK;
    void *sp = nullptr;
    JH_TRY(jhb::split_slabs(out, (size_t)(p.parts + (finish ? 1 : 0)) * (size_t)K * (size_t)p.n_scalars * sizeof(S), &sp));
    *slabs = (S *)sp;
    return JH_OK;
}
// the fold of the slabs: the whole vector at once, or (ranged) the range of each of the K pieces.  finish: into the folded slab, and after(folded, lo, hi)
// -- the stages after A' and the accumulation, k_chain_finish -- takes every fold from there to `out`
struct GridNoFinish { int operator()(const void *, int64_t, int64_t) const { return JH_OK; } };
template <typename S, class F = GridNoFinish> int grid_fold(const GridPlan &p, int K, S *slabs, void *out, bool finish = false, F after = F{})
{
    if (!slabs) return JH_OK;
    const int64_t ndom = (int64_t)K * p.n_scalars;
    S *folded = finish ? slabs + p.parts * ndom : (S *)out;
    for (int k = 0; k < (p.ranged ? K : 1); k++) {
        const int64_t lo = p.ranged ? (int64_t)k * p.n_scalars + p.s_begin : 0, hi = p.ranged ? (int64_t)k * p.n_scalars + p.s_end : ndom;
        JH_TRY(jhb::fold_parts(sizeof(S) == 4 ? JH_F32 : JH_F64, slabs + lo, ndom, p.parts, folded, lo, hi));
        if (finish) JH_TRY(after(folded, lo, hi));
    }
    return JH_OK;
}
