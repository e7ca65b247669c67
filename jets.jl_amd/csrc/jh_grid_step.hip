// jh_grid_step.hip -- the one-pass Golub-Kahan step of an N x K GRID of equal elementwise blocks, K = 2 .. 4 (jh_blockop_bidiag_step on a
// multi-parameter operator; the LSQR and CGLS loops of jh_lsqr.hip iterate on it).
//
// The route it replaces runs the grid forward into a zeroed range temporary, a range lincomb and norm, and the grid adjoint:
//     t_i = ((0 + A_i1 v_1) + A_i2 v_2) + ...        rows summed from +0 in column order, zero blocks skipped (src/Jets.jl:1022-1026)
//     u_i <- alpha t_i + beta u_i                   product, product, sum, each rounded; beta == 0: alpha t_i, u is not read
//     w_k = ((0 + A_1k' u_1) + A_2k' u_2) + ...     the NEW u, columns summed from +0 in row order (1042-1049)
//     ||u||^2                                       fp64 per-workgroup partials, folded in a fixed order (jh_tall_step.hip: finish_normsq)
// -- (2 N K + 5 N + 3 K) n s bytes and a range-sized temporary.  Here a lane owns one pack position of the blocks, keeps v_1 .. v_K and w_1 .. w_K in
// registers (the structure of k_grid_normal, jh_grid_normal.hip) and walks the block rows in order: every coefficient is read once, u_i is read
// (beta != 0), updated and written between the row's forward sum and its adjoint products.  (N K + 2 N + 2 K) n s bytes; u and w keep the bits
// of the three-call route (-ffp-contract=off), ||u||^2 counts each scalar once from the lane that owns it (vnorm2_from).
// Grids of several kinds (zero / identity / scalar / adjointed diagonal blocks -- the regularised [[A11 A12]; [lam I, 0]; [0, lam I]]) walk the packed
// block table (jh_grid_common.h); a batch of rows whose blocks are all plain diagonals takes the tight loop.  A row whose blocks are all zero gets
// u_i <- alpha*0 + beta*u_i and adds nothing to w.  Many rows of small blocks take the split-row walk (pick_adj_parts, the part rules of
// launch_grid_normal): u is updated row by row either way (same bits); w is summed per part and folded (tolerance; adj_split = 0: ordered).
#include "jh_grid_common.h"

namespace {

// u_i <- alpha t + beta u_i on this lane's pack, stored (the scalars the lane owns) and counted into ||u||^2
template <bool NT, bool OLD, typename S, int NS, typename V>
__device__ inline V grid_u_update(S *urow, int64_t s0, int64_t sk, int e0, bool ok, V t, V uo, S alpha, S beta, double &nrm)
{
    V r = (V)alpha * t;
    if constexpr (OLD) { V s2 = (V)beta * uo; r = r + s2; }
    if (ok) {
        st_pack<NT, S, NS>(urow, s0, sk, r);
        nrm += vnorm2_from<S, NS, V>(r, e0);
    }
    return r;
}

// MIXED: blocks of several kinds through the packed table words[i * K + k]; else plain diagonals, block (i, k) = blocks[i + k * nrow].
// OLD: beta != 0 -- u is read; else it is write-only.  (Decided at compile time: with the choice made per row, as in the tall plain walk, the
// walks of K = 2 .. 4 spilled 2-15 SGPRs.)
// The lanes cover the scalars [s_begin, s_end) of a block (the whole block: 0, n_scalars; a range of it: jh_blockop_bidiag_step_range with the knob
// grid_range); n_scalars stays the stride of the rows of u and of the pieces of v, w and the parts' slabs.
template <typename S, int E, int NS, int K, int DEPTH, bool NT, bool MIXED, bool OLD>
__global__ __launch_bounds__(256) void k_grid_step(const jh_dev_block *__restrict__ blocks, const uint64_t *__restrict__ words, int64_t nrow, int64_t n_scalars,
                                                   S *__restrict__ u, const S *__restrict__ v, S *__restrict__ w, S alpha, S beta,
                                                   double *__restrict__ partials, int64_t rows_per_part, S *__restrict__ part_out, int64_t s_begin, int64_t s_end)
{
    typedef typename vec_of<S, NS>::type V;
    const int64_t s0 = s_begin + ((int64_t)blockIdx.x * 256 + threadIdx.x) * NS;
    const bool ok = s0 < s_end;
    const int64_t sk = pack_start<NS>(ok ? s0 : s_begin, s_end);                      // (a range shorter than one pack ends with the block: loaded from s_end - NS)
    const int e0 = ok ? (int)(s0 - sk) : 0;                                         // a row's partial last pack counts the scalars it OWNS
    V x[K], acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        x[k] = ldu<false, S, NS>(v + (int64_t)k * n_scalars + sk);
        acc[k] = (V)(S)0;                                                           // m_k .= 0 (1042)
    }
    int64_t i = 0, iend = nrow;
    if (part_out) {
        i = (int64_t)blockIdx.y * rows_per_part;
        iend = iend < i + rows_per_part ? iend : i + rows_per_part;
    }
    double nrm = 0.0;
    // (alpha and beta in vector registers, as in k_grid_chain_step: with the range's two bounds among the arguments one walk spilled 2 SGPRs otherwise)
    S av = alpha, bv = beta;
    asm volatile("" : "+v"(av), "+v"(bv));
    if constexpr (MIXED) {
        // (the words of a batch are read when the batch starts, not one batch ahead as in k_grid_normal_mixed: the SGPRs of the records in flight
        // plus u's row are what made this walk spill -- DESIGN 3.8b, the grid chain's lesson)
        for (; i + DEPTH <= iend; i += DEPTH) {
            uint64_t wd[DEPTH][K];
            bool plain = true;
#pragma unroll
            for (int j = 0; j < DEPTH; j++)
#pragma unroll
                for (int k = 0; k < K; k++) {
                    wd[j][k] = words[(i + j) * K + k];
                    plain = plain && ((wd[j][k] >> 48) & 0xFu) == (uint64_t)JH_OP_DIAG;     // kind DIAG, not adjointed
                }
            V c[DEPTH][K], uo[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
#pragma unroll
                for (int k = 0; k < K; k++)
                    c[j][k] = gw_kind(wd[j][k]) == JH_OP_DIAG ? ldu<NT, S, NS>(reinterpret_cast<const S *>(wd[j][k] & GW_PTR) + sk) : (V)(S)0;
                uo[j] = OLD ? ldu<NT, S, NS>(u + (i + j) * n_scalars + sk) : (V)(S)0;
            }
            if (plain) {
#pragma unroll
                for (int j = 0; j < DEPTH; j++) {
                    V t = (V)(S)0;
#pragma unroll
                    for (int k = 0; k < K; k++) t = t + vmul<S, E, NS, V>(c[j][k], x[k], false);
                    const V r = grid_u_update<NT, OLD, S, NS, V>(u + (i + j) * n_scalars, s0, sk, e0, ok, t, uo[j], av, bv, nrm);
#pragma unroll
                    for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(c[j][k], r, true);
                }
                continue;
            }
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
                V t = (V)(S)0;                                                      // zeros(range(A)); a zero block is skipped (1022 / 1047)
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (gw_kind(wd[j][k]) != JH_OP_ZERO) t = t + grid_apply<S, E, NS, V>(wd[j][k], blocks, (i + j) + (int64_t)k * nrow, x[k], c[j][k], false);
                const V r = grid_u_update<NT, OLD, S, NS, V>(u + (i + j) * n_scalars, s0, sk, e0, ok, t, uo[j], av, bv, nrm);
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (gw_kind(wd[j][k]) != JH_OP_ZERO) acc[k] = acc[k] + grid_apply<S, E, NS, V>(wd[j][k], blocks, (i + j) + (int64_t)k * nrow, r, c[j][k], true);
            }
        }
        for (; i < iend; i++) {
            uint64_t wd[K];
            V c[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                wd[k] = words[i * K + k];
                c[k] = gw_kind(wd[k]) == JH_OP_DIAG ? ldu<NT, S, NS>(reinterpret_cast<const S *>(wd[k] & GW_PTR) + sk) : (V)(S)0;
            }
            const V uo = OLD ? ldu<NT, S, NS>(u + i * n_scalars + sk) : (V)(S)0;
            V t = (V)(S)0;
#pragma unroll
            for (int k = 0; k < K; k++)
                if (gw_kind(wd[k]) != JH_OP_ZERO) t = t + grid_apply<S, E, NS, V>(wd[k], blocks, i + (int64_t)k * nrow, x[k], c[k], false);
            const V r = grid_u_update<NT, OLD, S, NS, V>(u + i * n_scalars, s0, sk, e0, ok, t, uo, av, bv, nrm);
#pragma unroll
            for (int k = 0; k < K; k++)
                if (gw_kind(wd[k]) != JH_OP_ZERO) acc[k] = acc[k] + grid_apply<S, E, NS, V>(wd[k], blocks, i + (int64_t)k * nrow, r, c[k], true);
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
            V c[DEPTH][K], uo[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
#pragma unroll
                for (int k = 0; k < K; k++) c[j][k] = ldu<NT, S, NS>(a[j][k] + sk);
                uo[j] = OLD ? ldu<NT, S, NS>(u + (i + j) * n_scalars + sk) : (V)(S)0;
            }
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
                V t = (V)(S)0;                                                      // zeros(range(A)) (531)
#pragma unroll
                for (int k = 0; k < K; k++) t = t + vmul<S, E, NS, V>(c[j][k], x[k], false);     // d_i .+= A_ik v_k (1024)
                const V r = grid_u_update<NT, OLD, S, NS, V>(u + (i + j) * n_scalars, s0, sk, e0, ok, t, uo[j], av, bv, nrm);
#pragma unroll
                for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(c[j][k], r, true);  // m_k .+= A_ik' u_i (1049)
            }
        }
        for (; i < iend; i++) {
            V c[K];
#pragma unroll
            for (int k = 0; k < K; k++) c[k] = ldu<NT, S, NS>((const S *)blocks[i + (int64_t)k * nrow].coeff + sk);
            const V uo = OLD ? ldu<NT, S, NS>(u + i * n_scalars + sk) : (V)(S)0;
            V t = (V)(S)0;
#pragma unroll
            for (int k = 0; k < K; k++) t = t + vmul<S, E, NS, V>(c[k], x[k], false);
            const V r = grid_u_update<NT, OLD, S, NS, V>(u + i * n_scalars, s0, sk, e0, ok, t, uo, av, bv, nrm);
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(c[k], r, true);
        }
    }
    if (ok) {
        S *o = part_out ? part_out + (int64_t)blockIdx.y * (K * n_scalars) : w;
#pragma unroll
        for (int k = 0; k < K; k++) st_pack<false, S, NS>(o + (int64_t)k * n_scalars, s0, sk, acc[k]);
    }
    wg_sum_store<256>(nrm, partials + blockIdx.x + (size_t)blockIdx.y * gridDim.x);     // by (part, tile): a fixed fold order
}

// rows in flight: plain diagonals keep the depths of k_grid_normal -- K x DEPTH = 8 (6 for K = 3) coefficient packs per lane, plus DEPTH packs
// of u; grids of several kinds half of that for K = 2 and 4 (MDEPTH): at the plain depths their walk spills SGPRs (the block words, the scalars).
// ComplexF32 (the longest product code) also takes one row at a time for K = 3 of several kinds and K = 4 of plain diagonals: 2 SGPRs spilled otherwise
template <typename S, int E, int K, bool MIX> struct grid_step_depth {
    static constexpr bool c32 = E == 2 && sizeof(S) == 4;
    static constexpr int DEPTH = K == 2 ? 4 : (K == 3 ? 2 : (c32 ? 1 : 2)), MDEPTH = K == 2 ? 2 : (K == 3 ? (c32 ? 1 : 2) : 1);
    static constexpr int value = MIX ? MDEPTH : DEPTH;
};

// first match of (nontemporal, several kinds, u read: beta != 0)
template <typename S, int E, int NS, int K> struct GridStepPicker {
    using Kernel = decltype(&k_grid_step<S, E, NS, K, 1, false, false, false>);
    bool nt, mixed, old;
    Picked<Kernel> got;
    template <bool NTV, bool MIX, bool OLDV> bool row()
    {
        constexpr int D = grid_step_depth<S, E, K, MIX>::value;
        if (nt == NTV && mixed == MIX && old == OLDV) got = {&k_grid_step<S, E, NS, K, D, NTV, MIX, OLDV>, 256, 1, D};
        return got.k != nullptr;
    }
    template <bool MIX, bool OLDV> bool rows() { return row<false, MIX, OLDV>() || row<true, MIX, OLDV>(); }
    Picked<Kernel> pick() { (void)(rows<false, false>() || rows<false, true>() || rows<true, false>() || rows<true, true>()); return got; }
};

// end_elem < 0: the whole block; else the positions [first_elem, end_elem) of every block, ||u||^2 deferred
template <typename S, int E, int NS, int K>
int launch_grid_step(const jh_blockop *op, void *u, const void *v, void *w, double alpha, double beta, double *normsq, int64_t first_elem, int64_t end_elem)
{
    jh_context &c = jh_ctx();
    const GridPlan p = grid_plan(op, E, NS, first_elem, end_elem);
    S *slabs = nullptr;
    JH_TRY(grid_slabs(p, K, w, &slabs));
    JH_TRY(jh_ensure_partials(p.gx * p.parts));
    // streamed per pass: the coefficients, and u -- written, and read as well when beta != 0
    const bool nt = jh_stream_nt(((double)K + (beta != 0.0 ? 2.0 : 1.0)) * (double)op->nrow * (double)p.n_scalars * sizeof(S));
    c.last_adj_parts = p.parts;
    c.last_adj_launches = 1;
    (p.ranged ? c.last_grid_range_shape : c.last_grid_step_shape) = (nt ? 1 : 0) | (p.parts > 1 ? 2 : 0);
    const auto k = GridStepPicker<S, E, NS, K>{nt, !op->all_diag, beta != 0.0, {}}.pick();
    hipLaunchKernelGGL(k.k, dim3((unsigned)p.gx, (unsigned)p.parts), dim3(k.blk), 0, c.stream, op->dev_blocks, (const uint64_t *)op->grid_words, op->nrow,
                       p.n_scalars, (S *)u, (const S *)v, (S *)w, (S)alpha, (S)beta, c.part_dev, p.rows_per_part, slabs, p.s_begin, p.s_end);
    JH_CHECK_HIP(hipGetLastError());
    JH_TRY(grid_fold(p, K, slabs, w));
    return jhb::step_finish_normsq(p.gx * p.parts, normsq, p.ranged);
}

}  // namespace

namespace jhb {

bool grid_step_ok(const jh_blockop *op, const void *u, const void *v, const void *w)
{
    if (jh_ctx().grid_step == 0 || !grid_shape_ok(op, true)) return false;
    return vectors_scalar_aligned(op->dtype, u, v, w);
}

// the caller has checked grid_step_ok; w must not alias v (jh_blockop_bidiag_step)
static int grid_step_by_dtype(const jh_blockop *op, void *u, const void *v, void *w, double alpha, double beta, double *normsq, int64_t first_elem, int64_t end_elem)
{
    JH_TRY(grid_words_ensure(op));
    return jh_by_dtype(op->dtype, "grid step", [&](auto t) {
        using T = decltype(t);
        return grid_by_k(op->ncol, [&](auto k) {
            return launch_grid_step<typename T::S, T::E, T::NS, decltype(k)::value>(op, u, v, w, alpha, beta, normsq, first_elem, end_elem);
        });
    });
}

int grid_step(const jh_blockop *op, void *u, const void *v, void *w, double alpha, double beta, double *normsq)
{
    return grid_step_by_dtype(op, u, v, w, alpha, beta, normsq, 0, -1);
}

// positions [first_elem, first_elem + count) of every block (jh_blockop_bidiag_step_range, knob grid_range; the caller has checked grid_range_ok and
// grid_range_bounds): the same kernel over those lanes.  The nontemporal rule sees the WHOLE step's bytes, so a ranged step streams like the whole one;
// the range's share of ||u||^2 is returned, or (normsq == NULL) added to the context's accumulator in enqueue order.
int grid_step_range(const jh_blockop *op, void *u, const void *v, void *w, double alpha, double beta, int64_t first_elem, int64_t count, double *normsq)
{
    return grid_step_by_dtype(op, u, v, w, alpha, beta, normsq, first_elem, first_elem + count);
}

}  // namespace jhb
