// jh_grid_chain_kernels.h -- fused chains through an N x K GRID of equal elementwise blocks, K = 2 .. 4 (the chain family of jh_tall_chain_kernels.h on
// the grid walk of jh_grid_normal.hip).
//
// A multi-parameter operator (N shots x K model parameters) under a data weight, a mask or a preconditioner: the reference applies the composite
// stage by stage (src/Jets.jl:530-540), the grid through JetBlock_df! / df'! (1010-1057), every stage into a range- or domain-sized temporary.  Here
//     FORWARD   d_i = R( ((0 + a_i1 .* P(m)_1) + a_i2 .* P(m)_2) + ... )                      W o A o M
//     ADJOINT   y_k = Q( ((0 + conj(a_1k) .* R(d_1)) + conj(a_2k) .* R(d_2)) + ... )          M' o A' o W'
//     NORMAL    y_k = Q( sum_i conj(a_ik) .* R( sum_k' a_ik' .* P(m)_k' ) )                   M' o A' o W o A o M
// in ONE pass: a lane owns one pack position of the blocks, keeps P(m)_1 .. P(m)_K and y_1 .. y_K in registers and walks the block rows in order,
// DEPTH rows of loads in flight (a software pipeline: one copy of the row's arithmetic).  Every coefficient is read once.  The stage lists are the
// tall chains' (ChainProg, dom_prog, mid_prog): P / Q on the whole domain vector (K n elements: lane sk of column k reads coef + k n + sk), R per
// block row.  Rounding is the stage-by-stage chain's: every product rounded in the element type (-ffp-contract=off), the block row's sum from +0 in
// column order (1024), the block column's from +0 in row order (1042 / 1049), zero blocks skipped (1022 / 1047), so the bits are the same.
//
// THE ROW TABLE: one record of K + NW 64-bit words per block row, built by jh_chain_create: words 0 .. K-1 the row's blocks (the tall chains' word 0:
// pointer | kind << 48 | adjoint << 51 | real scalar << 52), words K .. K+NW-1 the row's range-side coefficient streams (pointer | conj << 48 | zero << 49).
// mid_prog reads a row's weight words at e[1 .. NW]: it is handed the record from word K - 1 on.
#pragma once
#include "jh_tall_chain_kernels.h"
#include "jh_grid_common.h"

namespace jhb {
// k_chain_finish on `ch`'s element type (jh_tall_chain_adj.hip: the tall chains' instantiations, not a second copy per grid unit)
int chain_finish(const jh_chain *ch, const ChainArgs &ca, void *out, const void *folded, int64_t s_begin, int64_t s_end, int accumulate);
}  // namespace jhb

// which of a grid chain's programs a launch runs: the handle's own, or the ADJOINT / NORMAL program derived from a FORWARD chain.  It indexes
// jh_chain::dev_mid (the device copies of the range-side lists) and picks the ChainArgs: one index for both, so they cannot disagree
enum { GRID_PROG_OWN = 0, GRID_PROG_ADJ = 1, GRID_PROG_NRM = 2 };

namespace {

// MODE 0 FORWARD, 1 ADJOINT, 2 NORMAL.  Launched on (tiles, parts): workgroup row blockIdx.y walks block rows [y, y + 1) * rows_per_part.  FORWARD: the
// parts are independent row groups (no fold); ADJOINT / NORMAL: part_out != NULL -- the split walk, slab y of part_out (K n scalars apart) gets the
// part's row sums and the fold (k_fold_parts) and the list after A' (k_chain_finish) follow in launches of their own.
// The lanes cover the scalars [s_begin, s_end) of a block (the whole block: 0, n_scalars; a range of it: jh_chain_apply_range with the knob
// grid_chain_range -- a range shorter than one pack ends with the block and is loaded from s_end - NS); n_scalars stays the stride of the rows of the
// range vector, of the K pieces of the domain vectors (the domain-side lists address coef + k n_scalars + sk) and of the slabs.
template <typename S, int E, int NS, int K, int DEPTH, bool NT, int MODE, int NW>
__global__ __launch_bounds__(256) void k_grid_chain(const jh_dev_block *__restrict__ blocks, int64_t nrow, const ChainArgs ca, S *__restrict__ out,
                                                    const S *__restrict__ in, int64_t n_scalars, int accumulate, int64_t rows_per_part,
                                                    S *__restrict__ part_out, const ChainProg *__restrict__ mid_dev, int64_t s_begin, int64_t s_end)
{
    typedef typename vec_of<S, NS>::type V;
    constexpr int NWA = NW > 0 ? NW : 1, RW = K + NW;
    const int64_t s0 = s_begin + ((int64_t)blockIdx.x * 256 + threadIdx.x) * NS;
    const bool ok = s0 < s_end;
    const int64_t sk = pack_start<NS>(ok ? s0 : s_begin, s_end);
    const bool rmw = accumulate == 1 || accumulate == -1;
    const bool has_mid = NW > 0 || (ca.mid.st[0] & 15u) != CK_NONE;
    V x[K], acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        x[k] = MODE != 1 ? ldu<false, S, NS>(in + (int64_t)k * n_scalars + sk) : (V)(S)0;
        acc[k] = (V)(S)0;                                                                 // m_k .= 0 (1042)
    }
    if (MODE != 1 && (ca.pre.st[0] & 15u) != CK_NONE) {
#pragma unroll
        for (int k = 0; k < K; k++) x[k] = dom_prog<S, E, NS, V>(ca.pre, ca.pre_c[0], ca.pre_c[1], x[k], (int64_t)k * n_scalars + sk);
    }
    int64_t i = (int64_t)blockIdx.y * rows_per_part;
    const int64_t iend = nrow < i + rows_per_part ? nrow : i + rows_per_part;
    // block row r's sum of A's products (FORWARD / NORMAL): 0 + a_r1 .* x_1 + ... in column order, a zero block skipped (1022)
    auto row_fwd = [&](int64_t r, const uint64_t *e, const V *c, bool plain) -> V {
        V t = (V)(S)0;                                                                    // zeros(range(A)) (531)
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (plain) t = t + vmul<S, E, NS, V>(c[k], x[k], false);
            else if (cr_kind(e[k]) != JH_OP_ZERO) t = t + chain_apply_row<S, E, NS, V>(e[k], blocks, r + (int64_t)k * nrow, x[k], c[k], false);
        }
        return t;
    };
    // one block row whose record `e`, coefficient packs `c`, weight packs `wv` and input pack `dv` are loaded
    auto row_op = [&](int64_t r, const uint64_t *e, const V *c, const V *wv, V dv, bool plain) {
        V t = MODE == 1 ? dv : row_fwd(r, e, c, plain);
        if (has_mid) {
            // (ca.mid's device copy read per row through an opaque pointer: the predicates derived from the list, hoisted out of the row loop, were held
            //  as lane masks in SGPRs -- every instantiation spilled SGPRs; per row it is a few scalar loads from the constant cache and scalar instructions.
            //  The address of the argument itself put the whole struct in a scratch frame)
            typedef const ChainProg __attribute__((address_space(1))) *gp;
            gp pp = (gp)mid_dev;
            asm volatile("" : "+s"(pp));
            ChainProg mp;
#pragma unroll
            for (int q = 0; q < JH_CHAIN_MAX_STAGES; q++) { mp.st[q] = pp->st[q]; mp.a32[q] = pp->a32[q]; mp.a[q] = pp->a[q]; }
            t = mid_prog<S, E, NS, NW, V>(mp, t, wv, e + (K - 1));
        }
        if constexpr (MODE == 0) {
            if (ok) st_pack<true, S, NS>(out + r * n_scalars, s0, sk, chain_accumulate<S, NS, V>(accumulate, dv, t));
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) {
                if (plain) acc[k] = acc[k] + vmul<S, E, NS, V>(c[k], t, true);
                else if (cr_kind(e[k]) != JH_OP_ZERO)                                     // _m .+= mul!(mtmp, op', _d) (1047 / 1049)
                    acc[k] = acc[k] + chain_apply_row<S, E, NS, V>(e[k], blocks, r + (int64_t)k * nrow, t, c[k], true);
            }
        }
    };
    // (MODE 0: dv is what the output row holds -- read for accumulate = +-1 only; MODE 1: the input row)
    auto load_row = [&](int64_t r, const uint64_t *e, V *c, V *wv, V &dv, bool plain) {
#pragma unroll
        for (int k = 0; k < K; k++)
            c[k] = (plain || cr_kind(e[k]) == JH_OP_DIAG) ? ldu<NT, S, NS>(cr_ptr<S>(e[k]) + sk) : (V)(S)0;
#pragma unroll
        for (int w = 0; w < NWA; w++) {
            const uint64_t we = e[NW > 0 ? K + w : 0];
            wv[w] = (NW > 0 && (plain || (we & CR_PTR))) ? ldu<NT, S, NS>(cr_ptr<S>(we) + sk) : (V)(S)0;
        }
        if (MODE == 1) dv = ldu<NT, S, NS>(in + r * n_scalars + sk);
        else if (MODE == 0) dv = rmw ? ldu<NT, S, NS>(out + r * n_scalars + sk) : (V)(S)0;
    };
    // a software pipeline DEPTH rows deep: the loads of rows r + 1 .. r + DEPTH - 1 are in flight while row r is computed.  ONE copy of the row's
    // arithmetic in the loop body (an unrolled batch inlined the range-side list once per row and held its loop-invariant predicates in SGPRs: every
    // instantiation spilled SGPRs, up to 145).  A row's record is requested when its loads are issued: records requested a batch ahead as well
    // (DEPTH + 1 records live) spilled SGPRs in a third of the instantiations.
    uint64_t rec[DEPTH][RW];
    V c[DEPTH][K], wv[DEPTH][NWA], dv[DEPTH];
    bool pl[DEPTH];
    auto fetch = [&](int64_t r, uint64_t *e) {                                          // (past the part's last row: its first row again, not loaded)
        bool p = true;
#pragma unroll
        for (int w = 0; w < RW; w++) {
            e[w] = ca.rows[(r < iend ? r : i) * RW + w];
            // a PLAIN row -- every block an un-adjointed diagonal, every weight word a bare pointer -- takes the tight products (jh_grid_normal.hip)
            if (w < K) p = p && ((e[w] >> 48) & 0xFu) == (uint64_t)JH_OP_DIAG;
            else p = p && (e[w] & CR_PTR) != 0 && (e[w] >> 48) == 0;
        }
        return p;
    };
#pragma unroll
    for (int j = 0; j < DEPTH; j++) {
        pl[j] = fetch(i + j, rec[j]);
        if (i + j < iend) load_row(i + j, rec[j], c[j], wv[j], dv[j], pl[j]);
    }
    for (; i < iend; i++) {
        row_op(i, rec[0], c[0], wv[0], dv[0], pl[0]);
#pragma unroll
        for (int j = 0; j < DEPTH - 1; j++) {
            pl[j] = pl[j + 1];
            dv[j] = dv[j + 1];
#pragma unroll
            for (int w = 0; w < RW; w++) rec[j][w] = rec[j + 1][w];
#pragma unroll
            for (int k = 0; k < K; k++) c[j][k] = c[j + 1][k];
#pragma unroll
            for (int w = 0; w < NWA; w++) wv[j][w] = wv[j + 1][w];
        }
        const int64_t r = i + DEPTH;
        pl[DEPTH - 1] = fetch(r, rec[DEPTH - 1]);
        if (r < iend) load_row(r, rec[DEPTH - 1], c[DEPTH - 1], wv[DEPTH - 1], dv[DEPTH - 1], pl[DEPTH - 1]);
    }
    if constexpr (MODE != 0) {
        if (!ok) return;
        if (part_out) {
            S *slab = part_out + (int64_t)blockIdx.y * (K * n_scalars);
#pragma unroll
            for (int k = 0; k < K; k++) st_pack<false, S, NS>(slab + (int64_t)k * n_scalars, s0, sk, acc[k]);
            return;
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            S *ok_ = out + (int64_t)k * n_scalars;
            const V found = rmw ? ldu<false, S, NS>(ok_ + sk) : (V)(S)0;
            const V r = dom_prog<S, E, NS, V>(ca.post, ca.post_c[0], ca.post_c[1], acc[k], (int64_t)k * n_scalars + sk);
            st_pack<false, S, NS>(ok_, s0, sk, chain_accumulate<S, NS, V>(accumulate, found, r));
        }
    }
}

// rows in flight: two for every K (K x 2 coefficient packs per lane, and the weights'); K = 2 at four rows spilled SGPRs with two range weights
template <int K> struct grid_chain_depth { static constexpr int value = 2; };

// first match of (nontemporal, range-side coefficient streams)
template <typename S, int E, int NS, int K, int MODE> struct GridChainPicker {
    static constexpr int D = grid_chain_depth<K>::value;
    using Kernel = decltype(&k_grid_chain<S, E, NS, K, D, false, MODE, 0>);
    bool nt;
    int nw;
    Picked<Kernel> got;
    template <bool NTV, int NWV> bool row()
    {
        if (nt == NTV && nw == NWV) got = {&k_grid_chain<S, E, NS, K, D, NTV, MODE, NWV>, 256, 1, D};
        return got.k != nullptr;
    }
    Picked<Kernel> pick() { (void)(row<false, 0>() || row<true, 0>() || row<false, 1>() || row<true, 1>() || row<false, 2>() || row<true, 2>()); return got; }
};

// end_elem < 0: the whole block; else the positions [first_elem, end_elem) of every block (jh_chain_apply_range, MODE != 0; the caller has checked the
// bounds): the same kernel over those lanes (GridPlan, jh_grid_common.h), the list after A' over each of the K pieces' range like the fold, and the
// nontemporal rule sees the WHOLE vector's bytes, so that a range streams like the whole vector.
template <typename S, int E, int NS, int K, int MODE>
int launch_grid_chain_k(const jh_chain *ch, int prog, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem)
{
    const ChainArgs &ca = prog == GRID_PROG_ADJ ? ch->adj_args : (prog == GRID_PROG_NRM ? ch->nrm_args : ch->args);
    jh_context &c = jh_ctx();
    const jh_blockop *op = ch->op;
    GridPlan p = MODE == 0 ? grid_lanes(op, E, NS, first_elem, end_elem) : grid_plan(op, E, NS, first_elem, end_elem);
    if (MODE == 0) {
        // FORWARD: the rows are independent; row groups of their own workgroups where one walk per tile would leave the chip short of
        // workgroups (P(m) is formed once per group: K n s more bytes per extra group).  adj_split > 1 forces the count.
        const int64_t want = (4 * (int64_t)c.cu_count + p.gx - 1) / p.gx;
        p.parts = c.adj_split > 1 ? c.adj_split : (c.adj_split == 0 ? 1 : want);
        if (p.parts > op->nrow) p.parts = op->nrow;
        if (p.parts < 1) p.parts = 1;
        p.rows_per_part = (op->nrow + p.parts - 1) / p.parts;
        p.parts = (op->nrow + p.rows_per_part - 1) / p.rows_per_part;
        JH_REQUIRE(p.parts < 65536, "grid chain: %lld row parts", (long long)p.parts);
    }
    const bool finish = MODE != 0 && (accumulate != 0 || (ca.post.st[0] & 15u) != CK_NONE);
    S *slabs = nullptr;
    if (MODE != 0) {
        JH_TRY(grid_slabs(p, K, out, &slabs, finish));
        c.last_adj_parts = p.parts;
    }
    const ChainProg *mid_dev = ch->dev_mid + prog;                                      // (ca.mid's device copy: the kernel reads it per row)
    const double streamed = ch->stream_bytes + (MODE != 2 ? (double)op->nrow * (double)p.n_scalars * sizeof(S) : 0.0);
    const bool nt = jh_stream_nt(streamed);
    if (p.ranged) c.last_grid_chain_range_shape = (nt ? 1 : 0) | (p.parts > 1 ? 2 : 0);
    else c.last_grid_chain_shape = (nt ? 1 : 0) | (p.parts > 1 ? 2 : 0) | (finish && p.parts > 1 ? 4 : 0);
    const auto k = GridChainPicker<S, E, NS, K, MODE>{nt, ch->nw < 2 ? ch->nw : 2, {}}.pick();
    JH_REQUIRE(k.k, "grid chain: no kernel for %d range-side streams", ch->nw);
    hipLaunchKernelGGL(k.k, dim3((unsigned)p.gx, (unsigned)p.parts), dim3(k.blk), 0, c.stream, op->dev_blocks, op->nrow, ca, (S *)out, (const S *)in,
                       p.n_scalars, accumulate, p.rows_per_part, slabs, mid_dev, p.s_begin, p.s_end);
    JH_CHECK_HIP(hipGetLastError());
    return grid_fold(p, K, slabs, out, finish, [&](const void *folded, int64_t lo, int64_t hi) { return jhb::chain_finish(ch, ca, out, folded, lo, hi, accumulate); });
}

// first_elem, end_elem: positions inside a block (end_elem < 0: the whole block)
template <int MODE>
int launch_grid_chain(const jh_chain *ch, int prog, void *out, const void *in, int accumulate, int64_t first_elem = 0, int64_t end_elem = -1)
{
    return jh_by_dtype(ch->op->dtype, "grid chain", [&](auto t) {
        using T = decltype(t);
        return grid_by_k(ch->op->ncol, [&](auto k) {
            return launch_grid_chain_k<typename T::S, T::E, T::NS, decltype(k)::value, MODE>(ch, prog, out, in, accumulate, first_elem, end_elem);
        });
    });
}

}  // namespace
