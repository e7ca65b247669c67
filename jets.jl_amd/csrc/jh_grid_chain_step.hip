// jh_grid_chain_step.hip -- the one-pass Golub-Kahan step of a FORWARD chain L = R o A o P through an N x K GRID of equal elementwise blocks,
// K = 2 .. 4 (jh_chain_bidiag_step on a grid chain; the LSQR and CGLS loops of jh_lsqr_solve_chain / jh_cgls_solve_chain iterate on it).  Knob
// grid_chain_step (default 0: the decline of jh_grid_chain.hip's first version).
//
// The route it replaces runs the FORWARD grid chain into a zeroed range temporary, a range lincomb and norm, and the derived ADJOINT grid chain:
//     t_i = R( ((0 + a_i1 .* P(v)_1) + a_i2 .* P(v)_2) + ... )     rows summed from +0 in column order, zero blocks skipped (src/Jets.jl:1022-1026)
//     u_i <- alpha t_i + beta u_i                                   product, product, sum, each rounded; beta == 0: alpha t_i, u is not read
//     z_i = R^H(u_i)                                                R's stages in reverse order, every diagonal conjugated (mid_step<1>)
//     w_k = Q( ((0 + conj(a_1k) .* z_1) + conj(a_2k) .* z_2) + ... )   the NEW u, columns summed from +0 in row order (1042-1049); Q = P^H
//     ||u||^2                                                       fp64 per-workgroup partials, folded in a fixed order
// -- (2 N K + (2 NW + 6) N + 2 K) n s bytes and a range-sized temporary.  Here a lane owns one pack position of the blocks (the layout of k_grid_chain
// and k_grid_step), keeps P(v)_1 .. P(v)_K and w_1 .. w_K in registers and walks the block rows in order, DEPTH rows of loads in flight: every
// coefficient and every weight is read once, u_i is read (beta != 0), updated and written between R and R^H.  (N K + (NW + 2) N + 2 K) n s bytes; u
// and w keep the bits of the three-call route (-ffp-contract=off), ||u||^2 counts each scalar once from the lane that owns it (vnorm2_from).
// Many rows of small blocks take the split-row walk (grid_plan, jh_grid_common.h): u is updated row by row either way (same
// bits); w is summed per part, folded, and Q follows on the folded vector (k_chain_finish) -- tolerance parity; adj_split = 0: the ordered walk.
#include "jh_grid_chain_kernels.h"

namespace {

// OLD: beta != 0 -- u is read; else it is write-only.  (Decided at compile time: jh_grid_step.hip's lesson -- the choice per row spilled SGPRs.)
// The lanes cover the scalars [s_begin, s_end) of a block (the whole block: 0, n_scalars; a range of it: jh_chain_bidiag_step_range with the knob
// grid_chain_range); n_scalars stays the stride of the rows of u, of the pieces of v and w (and of the domain-side lists' coefficients) and of the slabs.
template <typename S, int E, int NS, int K, int DEPTH, bool NT, int NW, bool OLD>
__global__ __launch_bounds__(256) void k_grid_chain_step(const jh_dev_block *__restrict__ blocks, int64_t nrow, const ChainArgs ca, S *__restrict__ w,
                                                         const S *__restrict__ v, S *__restrict__ u, int64_t n_scalars, S alpha, S beta,
                                                         double *__restrict__ partials, int64_t rows_per_part, S *__restrict__ part_out,
                                                         const ChainProg *__restrict__ mid_dev, int64_t s_begin, int64_t s_end)
{
    typedef typename vec_of<S, NS>::type V;
    constexpr int NWA = NW > 0 ? NW : 1, RW = K + NW;
    const int64_t s0 = s_begin + ((int64_t)blockIdx.x * 256 + threadIdx.x) * NS;
    const bool ok = s0 < s_end;
    const int64_t sk = pack_start<NS>(ok ? s0 : s_begin, s_end);                          // (a range shorter than one pack ends with the block: loaded from s_end - NS)
    const int e0 = ok ? (int)(s0 - sk) : 0;                                               // a row's partial last pack counts the scalars it OWNS
    const bool has_mid = NW > 0 || (ca.mid.st[0] & 15u) != CK_NONE;
    V x[K], acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        x[k] = ldu<false, S, NS>(v + (int64_t)k * n_scalars + sk);
        acc[k] = (V)(S)0;                                                                 // m_k .= 0 (1042)
    }
    if ((ca.pre.st[0] & 15u) != CK_NONE) {
#pragma unroll
        for (int k = 0; k < K; k++) x[k] = dom_prog<S, E, NS, V>(ca.pre, ca.pre_c[0], ca.pre_c[1], x[k], (int64_t)k * n_scalars + sk);
    }
    int64_t i = (int64_t)blockIdx.y * rows_per_part;
    const int64_t iend = nrow < i + rows_per_part ? nrow : i + rows_per_part;
    double nrm = 0.0;
    // (alpha and beta in vector registers: as scalars they were spilled across the row loop -- 2-13 SGPRs in 40 of the 144 instantiations)
    S av = alpha, bv = beta;
    asm volatile("" : "+v"(av), "+v"(bv));
    // one block row whose record `e`, coefficient packs `c`, weight packs `wv` and old u pack `uo` are loaded
    auto row_op = [&](int64_t r, const uint64_t *e, const V *c, const V *wv, V uo, bool plain) {
        V t = (V)(S)0;                                                                    // zeros(range(A)) (531); a zero block is skipped (1022)
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (plain) t = t + vmul<S, E, NS, V>(c[k], x[k], false);
            else if (cr_kind(e[k]) != JH_OP_ZERO) t = t + chain_apply_row<S, E, NS, V>(e[k], blocks, r + (int64_t)k * nrow, x[k], c[k], false);
        }
        // (R's list read per row through an opaque pointer, as k_grid_chain reads it: held across the row loop its predicates spill SGPRs)
        ChainProg mp;
        if (has_mid) {
            typedef const ChainProg __attribute__((address_space(1))) *gp;
            gp pp = (gp)mid_dev;
            asm volatile("" : "+s"(pp));
#pragma unroll
            for (int q = 0; q < JH_CHAIN_MAX_STAGES; q++) { mp.st[q] = pp->st[q]; mp.a32[q] = pp->a32[q]; mp.a[q] = pp->a[q]; }
            t = mid_step<0, S, E, NS, NW, V>(mp, t, wv, e + (K - 1));
        }
        V z = (V)av * t;                                                               // u_i <- alpha t_i + beta u_i
        if constexpr (OLD) { const V s2 = (V)bv * uo; z = z + s2; }
        if (ok) {
            st_pack<NT, S, NS>(u + r * n_scalars, s0, sk, z);
            nrm += vnorm2_from<S, NS, V>(z, e0);
        }
        if (has_mid) z = mid_step<1, S, E, NS, NW, V>(mp, z, wv, e + (K - 1));
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (plain) acc[k] = acc[k] + vmul<S, E, NS, V>(c[k], z, true);
            else if (cr_kind(e[k]) != JH_OP_ZERO)                                         // _m .+= mul!(mtmp, op', _d) (1047 / 1049)
                acc[k] = acc[k] + chain_apply_row<S, E, NS, V>(e[k], blocks, r + (int64_t)k * nrow, z, c[k], true);
        }
    };
    // (a row of zero blocks still has its weights and u loaded: u_i <- alpha R(0) + beta u_i)
    auto load_row = [&](int64_t r, const uint64_t *e, V *c, V *wv, V &uo, bool plain) {
#pragma unroll
        for (int k = 0; k < K; k++)
            c[k] = (plain || cr_kind(e[k]) == JH_OP_DIAG) ? ldu<NT, S, NS>(cr_ptr<S>(e[k]) + sk) : (V)(S)0;
#pragma unroll
        for (int q = 0; q < NWA; q++) {
            const uint64_t we = e[NW > 0 ? K + q : 0];
            wv[q] = (NW > 0 && (plain || (we & CR_PTR))) ? ldu<NT, S, NS>(cr_ptr<S>(we) + sk) : (V)(S)0;
        }
        uo = OLD ? ldu<NT, S, NS>(u + r * n_scalars + sk) : (V)(S)0;
    };
    // the software pipeline of k_grid_chain: DEPTH rows' loads in flight, ONE copy of the row's arithmetic, a row's record requested when its loads
    // are issued
    uint64_t rec[DEPTH][RW];
    V c[DEPTH][K], wv[DEPTH][NWA], uo[DEPTH];
    bool pl[DEPTH];
    auto fetch = [&](int64_t r, uint64_t *e) {                                          // (past the part's last row: its first row again, not loaded)
        bool p = true;
#pragma unroll
        for (int q = 0; q < RW; q++) {
            e[q] = ca.rows[(r < iend ? r : i) * RW + q];
            if (q < K) p = p && ((e[q] >> 48) & 0xFu) == (uint64_t)JH_OP_DIAG;
            else p = p && (e[q] & CR_PTR) != 0 && (e[q] >> 48) == 0;
        }
        return p;
    };
#pragma unroll
    for (int j = 0; j < DEPTH; j++) {
        pl[j] = fetch(i + j, rec[j]);
        if (i + j < iend) load_row(i + j, rec[j], c[j], wv[j], uo[j], pl[j]);
    }
    for (; i < iend; i++) {
        row_op(i, rec[0], c[0], wv[0], uo[0], pl[0]);
#pragma unroll
        for (int j = 0; j < DEPTH - 1; j++) {
            pl[j] = pl[j + 1];
            uo[j] = uo[j + 1];
#pragma unroll
            for (int q = 0; q < RW; q++) rec[j][q] = rec[j + 1][q];
#pragma unroll
            for (int k = 0; k < K; k++) c[j][k] = c[j + 1][k];
#pragma unroll
            for (int q = 0; q < NWA; q++) wv[j][q] = wv[j + 1][q];
        }
        const int64_t r = i + DEPTH;
        pl[DEPTH - 1] = fetch(r, rec[DEPTH - 1]);
        if (r < iend) load_row(r, rec[DEPTH - 1], c[DEPTH - 1], wv[DEPTH - 1], uo[DEPTH - 1], pl[DEPTH - 1]);
    }
    if (ok) {
        if (part_out) {
            S *slab = part_out + (int64_t)blockIdx.y * (K * n_scalars);
#pragma unroll
            for (int k = 0; k < K; k++) st_pack<false, S, NS>(slab + (int64_t)k * n_scalars, s0, sk, acc[k]);
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) {
                const V r = dom_prog<S, E, NS, V>(ca.post, ca.post_c[0], ca.post_c[1], acc[k], (int64_t)k * n_scalars + sk);
                st_pack<false, S, NS>(w + (int64_t)k * n_scalars, s0, sk, r);
            }
        }
    }
    wg_sum_store<256>(nrm, partials + blockIdx.x + (size_t)blockIdx.y * gridDim.x);       // by (part, tile): a fixed fold order
}

// rows in flight: two, as k_grid_chain (K x 2 coefficient packs per lane, the weights' and u's) -- one where 32-bit scalars meet two weight streams
// and four more streams (K blocks, u when it is read): two rows' records, addresses and predicates spill 2-6 SGPRs there
template <typename S, int K, int NW, bool OLD> struct grid_chain_step_depth {
    static constexpr int value = (sizeof(S) == 4 && NW == 2 && K + (OLD ? 1 : 0) >= 4) ? 1 : 2;
};

// first match of (nontemporal, range-side coefficient streams, u read: beta != 0)
template <typename S, int E, int NS, int K> struct GridChainStepPicker {
    using Kernel = decltype(&k_grid_chain_step<S, E, NS, K, 1, false, 0, false>);
    bool nt;
    int nw;
    bool old;
    Picked<Kernel> got;
    template <bool NTV, int NWV, bool OLDV> bool row()
    {
        constexpr int D = grid_chain_step_depth<S, K, NWV, OLDV>::value;
        if (nt == NTV && nw == NWV && old == OLDV) got = {&k_grid_chain_step<S, E, NS, K, D, NTV, NWV, OLDV>, 256, 1, D};
        return got.k != nullptr;
    }
    template <int NWV> bool rows() { return row<false, NWV, false>() || row<true, NWV, false>() || row<false, NWV, true>() || row<true, NWV, true>(); }
    Picked<Kernel> pick() { (void)(rows<0>() || rows<1>() || rows<2>()); return got; }
};

// end_elem < 0: the whole block; else the positions [first_elem, end_elem) of every block (jh_chain_bidiag_step_range, knob grid_chain_range): the same
// kernel over those lanes (GridPlan), Q over each of the K pieces' range, ||u||^2 deferred (normsq == NULL: added to the context's accumulator in enqueue order)
template <typename S, int E, int NS, int K>
int launch_grid_chain_step_k(const jh_chain *ch, void *u, const void *v, void *w, double alpha, double beta, double *normsq, int64_t first_elem, int64_t end_elem)
{
    const ChainArgs &ca = ch->step_args;
    jh_context &c = jh_ctx();
    const jh_blockop *op = ch->op;
    const GridPlan p = grid_plan(op, E, NS, first_elem, end_elem);
    const bool finish = (ca.post.st[0] & 15u) != CK_NONE;
    S *slabs = nullptr;
    JH_TRY(grid_slabs(p, K, w, &slabs, finish));
    JH_TRY(jh_ensure_partials(p.gx * p.parts));
    // streamed per pass: the coefficients and the weights, and u -- written, and read as well when beta != 0
    const bool nt = jh_stream_nt(ch->stream_bytes + (beta != 0.0 ? 2.0 : 1.0) * (double)op->nrow * (double)p.n_scalars * sizeof(S));
    c.last_adj_parts = p.parts;
    (p.ranged ? c.last_grid_chain_range_shape : c.last_grid_chain_step_shape) = (nt ? 1 : 0) | (p.parts > 1 ? 2 : 0);
    const ChainProg *mid_dev = ch->dev_mid + GRID_PROG_OWN;                              // (R: the FORWARD chain's own range-side list)
    const auto k = GridChainStepPicker<S, E, NS, K>{nt, ch->nw < 2 ? ch->nw : 2, beta != 0.0, {}}.pick();
    JH_REQUIRE(k.k, "grid chain step: no kernel for %d range-side streams", ch->nw);
    hipLaunchKernelGGL(k.k, dim3((unsigned)p.gx, (unsigned)p.parts), dim3(k.blk), 0, c.stream, op->dev_blocks, op->nrow, ca, (S *)w, (const S *)v, (S *)u,
                       p.n_scalars, (S)alpha, (S)beta, c.part_dev, p.rows_per_part, slabs, mid_dev, p.s_begin, p.s_end);
    JH_CHECK_HIP(hipGetLastError());
    JH_TRY(grid_fold(p, K, slabs, w, finish, [&](const void *folded, int64_t lo, int64_t hi) { return jhb::chain_finish(ch, ca, w, folded, lo, hi, 0); }));
    return jhb::step_finish_normsq(p.gx * p.parts, normsq, p.ranged);
}

}  // namespace

namespace jhb {

// the caller (jh_chain_bidiag_step / _range) has checked the knobs, the handle (a FORWARD grid chain, R + R^H within one list), the vectors, the row
// table and (ranged) the bounds
static int grid_chain_step_by_dtype(const jh_chain *ch, void *u, const void *v, void *w, double alpha, double beta, double *normsq, int64_t first_elem,
                                    int64_t end_elem)
{
    return jh_by_dtype(ch->op->dtype, "grid chain step", [&](auto t) {
        using T = decltype(t);
        return grid_by_k(ch->op->ncol, [&](auto k) {
            return launch_grid_chain_step_k<typename T::S, T::E, T::NS, decltype(k)::value>(ch, u, v, w, alpha, beta, normsq, first_elem, end_elem);
        });
    });
}

int grid_chain_step(const jh_chain *ch, void *u, const void *v, void *w, double alpha, double beta, double *normsq)
{
    return grid_chain_step_by_dtype(ch, u, v, w, alpha, beta, normsq, 0, -1);
}

// positions [first_elem, first_elem + count) of every block: those positions of every u_i, the K pieces w_k[first_elem, first_elem + count), the
// range's share of ||u||^2 (returned, or with normsq == NULL added to the context's accumulator in enqueue order)
int grid_chain_step_range(const jh_chain *ch, void *u, const void *v, void *w, double alpha, double beta, int64_t first_elem, int64_t count, double *normsq)
{
    return grid_chain_step_by_dtype(ch, u, v, w, alpha, beta, normsq, first_elem, first_elem + count);
}

}  // namespace jhb
