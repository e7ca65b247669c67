// jh_grid_range.hip -- the three ranged calls that pipeline a row partition's exchange, on an N x K GRID of equal elementwise blocks, K = 2 .. 4
// (knob grid_range = 1): jh_blockop_mul_adj_range, jh_blockop_normal_mul_range and jh_blockop_bidiag_step_range.
//
// A grid kernel's lane owns one pack position of the blocks across all K columns (it needs every v_k[p] for the row's forward sum), so the range of a
// grid is [first, first + count) INSIDE a block, not a piece of the flat K n domain slab: one call reads those positions of every u_i / d_i and writes
// the K pieces w_k[first, first + count) and nothing else.  A'A and the step are the whole-vector kernels over those lanes (k_grid_normal, k_grid_step:
// first and last scalar are run-time arguments, the row stride stays n -- jh_grid_normal.hip, jh_grid_step.hip).  The adjoint of a grid is otherwise the
// register-tiled general kernel (jh_general.hip: a workgroup per group of columns), which has no range; k_grid_adj below is the same lane layout as the
// other two:
//     m_k = ((0 + A_1k' d_1) + A_2k' d_2) + ...        columns summed from +0 in row order, zero blocks skipped (src/Jets.jl:1042-1049)
// -- the bits of the whole-vector adjoint wherever that walks the rows in one part (-ffp-contract=off).  Many rows of small blocks take the split-row
// walk (pick_adj_parts over the RANGE's workgroups; tolerance parity, adj_split = 0: ordered).  Blocks off the 16-byte grid: under-aligned packs, the
// partial last pack only in the range that ends the block.
#include "jh_grid_common.h"

namespace {

// MIXED: blocks of several kinds through the packed table words[i * K + k]; else plain diagonals, block (i, k) = blocks[i + k * nrow]
template <typename S, int E, int NS, int K, int DEPTH, bool NT, bool MIXED>
__global__ __launch_bounds__(256) void k_grid_adj(const jh_dev_block *__restrict__ blocks, const uint64_t *__restrict__ words, int64_t nrow, int64_t n_scalars,
                                                  const S *__restrict__ d, S *__restrict__ m, int64_t rows_per_part, S *__restrict__ part_out,
                                                  int64_t s_begin, int64_t s_end)
{
    typedef typename vec_of<S, NS>::type V;
    const int64_t s0 = s_begin + ((int64_t)blockIdx.x * 256 + threadIdx.x) * NS;
    const bool ok = s0 < s_end;
    const int64_t sk = pack_start<NS>(ok ? s0 : s_begin, s_end);                      // (a range shorter than one pack ends with the block: loaded from s_end - NS)
    V acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = (V)(S)0;                                     // m_k .= 0 (1042)
    int64_t i = 0, iend = nrow;
    if (part_out) {
        i = (int64_t)blockIdx.y * rows_per_part;
        iend = iend < i + rows_per_part ? iend : i + rows_per_part;
    }
    if constexpr (MIXED) {
        for (; i + DEPTH <= iend; i += DEPTH) {
            uint64_t wd[DEPTH][K];
#pragma unroll
            for (int j = 0; j < DEPTH; j++)
#pragma unroll
                for (int k = 0; k < K; k++) wd[j][k] = words[(i + j) * K + k];
            V c[DEPTH][K], dv[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
#pragma unroll
                for (int k = 0; k < K; k++)
                    c[j][k] = gw_kind(wd[j][k]) == JH_OP_DIAG ? ldu<NT, S, NS>(reinterpret_cast<const S *>(wd[j][k] & GW_PTR) + sk) : (V)(S)0;
                dv[j] = ldu<NT, S, NS>(d + (i + j) * n_scalars + sk);
            }
#pragma unroll
            for (int j = 0; j < DEPTH; j++)
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (gw_kind(wd[j][k]) != JH_OP_ZERO) acc[k] = acc[k] + grid_apply<S, E, NS, V>(wd[j][k], blocks, (i + j) + (int64_t)k * nrow, dv[j], c[j][k], true);
        }
        for (; i < iend; i++) {
            const V dv = ldu<NT, S, NS>(d + i * n_scalars + sk);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint64_t wd = words[i * K + k];
                const V c = gw_kind(wd) == JH_OP_DIAG ? ldu<NT, S, NS>(reinterpret_cast<const S *>(wd & GW_PTR) + sk) : (V)(S)0;
                if (gw_kind(wd) != JH_OP_ZERO) acc[k] = acc[k] + grid_apply<S, E, NS, V>(wd, blocks, i + (int64_t)k * nrow, dv, c, true);
            }
        }
    } else {
        // the next batch's pointers are requested while this batch's packs are in flight (k_grid_normal)
        const S *nxt[DEPTH][K];
#pragma unroll
        for (int j = 0; j < DEPTH; j++)
#pragma unroll
            for (int k = 0; k < K; k++) nxt[j][k] = (const S *)blocks[(i + j < iend ? i + j : i) + (int64_t)k * nrow].coeff;
        for (; i + DEPTH <= iend; i += DEPTH) {
            const S *a[DEPTH][K];
#pragma unroll
            for (int j = 0; j < DEPTH; j++)
#pragma unroll
                for (int k = 0; k < K; k++) {
                    a[j][k] = nxt[j][k];
                    const int64_t r = i + DEPTH + j;
                    nxt[j][k] = (const S *)blocks[(r < iend ? r : i) + (int64_t)k * nrow].coeff;
                }
            V c[DEPTH][K], dv[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
#pragma unroll
                for (int k = 0; k < K; k++) c[j][k] = ldu<NT, S, NS>(a[j][k] + sk);
                dv[j] = ldu<NT, S, NS>(d + (i + j) * n_scalars + sk);
            }
#pragma unroll
            for (int j = 0; j < DEPTH; j++)
#pragma unroll
                for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(c[j][k], dv[j], true);   // m_k .+= A_ik' d_i (1049)
        }
        for (; i < iend; i++) {
            const V dv = ldu<NT, S, NS>(d + i * n_scalars + sk);
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(ldu<NT, S, NS>((const S *)blocks[i + (int64_t)k * nrow].coeff + sk), dv, true);
        }
    }
    if (!ok) return;
    S *o = part_out ? part_out + (int64_t)blockIdx.y * (K * n_scalars) : m;
#pragma unroll
    for (int k = 0; k < K; k++) st_pack<false, S, NS>(o + (int64_t)k * n_scalars, s0, sk, acc[k]);
}

// rows in flight: the depths of k_grid_normal -- K x DEPTH = 8 (6 for K = 3) coefficient packs per lane, plus DEPTH packs of d
template <int K> struct grid_adj_depth { static constexpr int value = K == 2 ? 4 : 2; };

template <typename S, int E, int NS, int K> struct GridAdjPicker {
    static constexpr int D = grid_adj_depth<K>::value;
    using Kernel = decltype(&k_grid_adj<S, E, NS, K, D, false, false>);
    bool nt, mixed;
    Picked<Kernel> got;
    template <bool NTV, bool MIX> bool row()
    {
        if (nt == NTV && mixed == MIX) got = {&k_grid_adj<S, E, NS, K, D, NTV, MIX>, 256, 1, D};
        return got.k != nullptr;
    }
    Picked<Kernel> pick() { (void)(row<false, false>() || row<true, false>() || row<false, true>() || row<true, true>()); return got; }
};

// (end_elem >= 0: the adjoint is only ever ranged)
template <typename S, int E, int NS, int K>
int launch_grid_adj(const jh_blockop *op, void *m, const void *d, int64_t first_elem, int64_t end_elem)
{
    jh_context &c = jh_ctx();
    const GridPlan p = grid_plan(op, E, NS, first_elem, end_elem);
    S *slabs = nullptr;
    JH_TRY(grid_slabs(p, K, m, &slabs));
    c.last_adj_parts = p.parts;
    c.last_adj_launches = 1;
    // streamed once per pass: the coefficients and d -- over the WHOLE adjoint's bytes, so that a range streams like the whole vector would
    const bool nt = jh_stream_nt(((double)K + 1.0) * (double)op->nrow * (double)p.n_scalars * sizeof(S));
    c.last_grid_range_shape = (nt ? 1 : 0) | (p.parts > 1 ? 2 : 0);
    const auto k = GridAdjPicker<S, E, NS, K>{nt, !op->all_diag, {}}.pick();
    hipLaunchKernelGGL(k.k, dim3((unsigned)p.gx, (unsigned)p.parts), dim3(k.blk), 0, c.stream, op->dev_blocks, (const uint64_t *)op->grid_words, op->nrow,
                       p.n_scalars, (const S *)d, (S *)m, p.rows_per_part, slabs, p.s_begin, p.s_end);
    JH_CHECK_HIP(hipGetLastError());
    return grid_fold(p, K, slabs, m);
}

}  // namespace

namespace jhb {

// the grids of the whole-vector one-pass kernels (grid_shape_ok: N >= 2, K = 2 .. 4, equal elementwise blocks of >= 16 bytes, no nonlinear child), the
// knob, and vectors aligned like their scalar (c may be NULL)
bool grid_range_ok(const jh_blockop *op, const void *a, const void *b, const void *c)
{
    if (jh_ctx().grid_range != 1 || !grid_shape_ok(op, true)) return false;
    return vectors_scalar_aligned(op->dtype, a, b, c);
}

int grid_range_bounds(const jh_blockop *op, int64_t first_elem, int64_t count, const char *who)
{
    const int64_t n = op->row_len[0], es = (int64_t)jh_dtype_size(op->dtype);
    JH_REQUIRE(first_elem >= 0 && count >= 0 && first_elem + count <= n,
               "%s: on an N x K grid the range is positions inside a block: [%lld, %lld) is outside a block of %lld elements", who, (long long)first_elem,
               (long long)(first_elem + count), (long long)n);
    JH_REQUIRE((first_elem * es) % 16 == 0 && ((count * es) % 16 == 0 || first_elem + count == n),
               "%s: range boundaries must be 16-byte aligned inside the block (the last range may end with the block)", who);
    return JH_OK;
}

int grid_adj_range(const jh_blockop *op, void *m, const void *d, int64_t first_elem, int64_t count)
{
    JH_TRY(grid_words_ensure(op));
    return jh_by_dtype(op->dtype, "grid adjoint", [&](auto t) {
        using T = decltype(t);
        return grid_by_k(op->ncol, [&](auto k) { return launch_grid_adj<typename T::S, T::E, T::NS, decltype(k)::value>(op, m, d, first_elem, first_elem + count); });
    });
}

}  // namespace jhb
