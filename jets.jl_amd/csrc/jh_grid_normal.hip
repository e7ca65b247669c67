// jh_grid_normal.hip -- the fused normal operator y = A'(A m) of an N x K GRID of equal diagonal blocks, K = 2 .. 4 (round 6).
//
// The reference applies (A', A) stage by stage (src/Jets.jl:530-534): JetBlock_df! (1010-1032) writes the N range blocks
//     t_i = ((0 + a_i1 .* m_1) + a_i2 .* m_2) + ...            (the composite's zeros(range(A)), 531, then d_i .+= A_ik m_k in column order, 1024)
// and JetBlock_df'! (1034-1057) sums them back per block column,
//     y_k = ((0 + conj(a_1k) .* t_1) + conj(a_2k) .* t_2) + ...   (m_k .= 0, 1042, then rows in order, 1049)
// -- 2 N K n s bytes of coefficients and 2 N n s of the range-sized temporary.  A multi-parameter operator (N shots x K model
// parameters) has a SMALL K: a lane that owns one pack position of the blocks keeps m_1 .. m_K and y_1 .. y_K in registers,
// walks the rows in order and reads every coefficient ONCE: N K n s + 2 K n s bytes, no temporary.  Every product and every sum
// is rounded where the two-stage chain rounds it (-ffp-contract=off), so the result has the chain's bits.
// Many rows of small blocks take the split-row walk of the tall kernels (jh_tall.hip: pick_adj_parts; tolerance parity, adj_split = 0
// keeps the ordered walk).  Blocks need not be whole 16-byte packs (under-aligned packs, jh_blockop_common.h).
//
// Later in round 6: grids whose blocks are of SEVERAL elementwise kinds -- the regularised multi-parameter operator [[A11 A12]; [lam I, 0]; [0, lam I]]: zero
// blocks (skipped: 1022 / 1047), identities, scalars, adjointed diagonals -- through a packed table of one 64-bit word per block (pointer | kind << 48 |
// adjoint << 51 | real scalar << 52, built on first use) and the lesson of the tall kernels: a batch of rows whose blocks are all PLAIN diagonals takes the tight
// loop, any other batch the per-block switch.
#include "jh_grid_common.h"
#include <vector>

namespace {

// the same walk over the PACKED table (MIXED grids): words[(i) * K + k]
template <typename S, int E, int NS, int K, int DEPTH, bool NT>
__global__ __launch_bounds__(256) void k_grid_normal_mixed(const jh_dev_block *__restrict__ blocks, const uint64_t *__restrict__ words, int64_t nrow, int64_t n_scalars,
                                                           const S *__restrict__ m, S *__restrict__ y, int64_t rows_per_part, S *__restrict__ part_out,
                                                           int64_t s_begin, int64_t s_end)
{
    typedef typename vec_of<S, NS>::type V;
    const int64_t s0 = s_begin + ((int64_t)blockIdx.x * 256 + threadIdx.x) * NS;      // (the lanes cover [s_begin, s_end) of a block: k_grid_normal)
    const bool ok = s0 < s_end;
    const int64_t sk = pack_start<NS>(ok ? s0 : s_begin, s_end);
    V x[K], acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        x[k] = ldu<false, S, NS>(m + (int64_t)k * n_scalars + sk);
        acc[k] = (V)(S)0;                                                                 // m_k .= 0 (1042)
    }
    int64_t i = 0, iend = nrow;
    if (part_out) {
        i = (int64_t)blockIdx.y * rows_per_part;
        iend = iend < i + rows_per_part ? iend : i + rows_per_part;
    }
    uint64_t nxt[DEPTH][K];
#pragma unroll
    for (int j = 0; j < DEPTH; j++)
#pragma unroll
        for (int k = 0; k < K; k++) nxt[j][k] = words[(i + j < iend ? i + j : i) * K + k];
    for (; i + DEPTH <= iend; i += DEPTH) {
        uint64_t w[DEPTH][K];
        bool plain = true;
#pragma unroll
        for (int j = 0; j < DEPTH; j++)
#pragma unroll
            for (int k = 0; k < K; k++) {
                w[j][k] = nxt[j][k];
                const int64_t r = i + DEPTH + j;
                nxt[j][k] = words[(r < iend ? r : i) * K + k];
                plain = plain && ((w[j][k] >> 48) & 0xFu) == (uint64_t)JH_OP_DIAG;       // kind DIAG, not adjointed
            }
        V c[DEPTH][K];
        if (plain) {
#pragma unroll
            for (int j = 0; j < DEPTH; j++)
#pragma unroll
                for (int k = 0; k < K; k++) c[j][k] = ldu<NT, S, NS>(reinterpret_cast<const S *>(w[j][k] & GW_PTR) + sk);
#pragma unroll
            for (int j = 0; j < DEPTH; j++) {
                V t = (V)(S)0;
#pragma unroll
                for (int k = 0; k < K; k++) t = t + vmul<S, E, NS, V>(c[j][k], x[k], false);
#pragma unroll
                for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(c[j][k], t, true);
            }
            continue;
        }
#pragma unroll
        for (int j = 0; j < DEPTH; j++)
#pragma unroll
            for (int k = 0; k < K; k++)
                c[j][k] = gw_kind(w[j][k]) == JH_OP_DIAG ? ldu<NT, S, NS>(reinterpret_cast<const S *>(w[j][k] & GW_PTR) + sk) : (V)(S)0;
#pragma unroll
        for (int j = 0; j < DEPTH; j++) {
            V t = (V)(S)0;                                                                // zeros(range(A)) (531); a zero block is skipped (1022 / 1047)
#pragma unroll
            for (int k = 0; k < K; k++)
                if (gw_kind(w[j][k]) != JH_OP_ZERO) t = t + grid_apply<S, E, NS, V>(w[j][k], blocks, (i + j) + (int64_t)k * nrow, x[k], c[j][k], false);
#pragma unroll
            for (int k = 0; k < K; k++)
                if (gw_kind(w[j][k]) != JH_OP_ZERO) acc[k] = acc[k] + grid_apply<S, E, NS, V>(w[j][k], blocks, (i + j) + (int64_t)k * nrow, t, c[j][k], true);
        }
    }
    for (; i < iend; i++) {
        uint64_t w[K];
        V c[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            w[k] = words[i * K + k];
            c[k] = gw_kind(w[k]) == JH_OP_DIAG ? ldu<NT, S, NS>(reinterpret_cast<const S *>(w[k] & GW_PTR) + sk) : (V)(S)0;
        }
        V t = (V)(S)0;
#pragma unroll
        for (int k = 0; k < K; k++)
            if (gw_kind(w[k]) != JH_OP_ZERO) t = t + grid_apply<S, E, NS, V>(w[k], blocks, i + (int64_t)k * nrow, x[k], c[k], false);
#pragma unroll
        for (int k = 0; k < K; k++)
            if (gw_kind(w[k]) != JH_OP_ZERO) acc[k] = acc[k] + grid_apply<S, E, NS, V>(w[k], blocks, i + (int64_t)k * nrow, t, c[k], true);
    }
    if (!ok) return;
    S *o = part_out ? part_out + (int64_t)blockIdx.y * (K * n_scalars) : y;
#pragma unroll
    for (int k = 0; k < K; k++) st_pack<false, S, NS>(o + (int64_t)k * n_scalars, s0, sk, acc[k]);
}

template <typename S, int E, int NS, int K, int DEPTH, bool NT>
__global__ __launch_bounds__(256) void k_grid_normal(const jh_dev_block *__restrict__ blocks, int64_t nrow, int64_t n_scalars, const S *__restrict__ m,
                                                     S *__restrict__ y, int64_t rows_per_part, S *__restrict__ part_out, int64_t s_begin, int64_t s_end)
{
    // the lanes cover the scalars [s_begin, s_end) of a block (the whole block: 0, n_scalars; a range of it: jh_blockop_normal_mul_range with the knob
    // grid_range -- a range shorter than one pack ends with the block and is loaded from s_end - NS); n_scalars stays the stride of the pieces of m, y and the slabs
    typedef typename vec_of<S, NS>::type V;
    const int64_t s0 = s_begin + ((int64_t)blockIdx.x * 256 + threadIdx.x) * NS;
    const bool ok = s0 < s_end;
    const int64_t sk = pack_start<NS>(ok ? s0 : s_begin, s_end);
    V x[K], acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        x[k] = ldu<false, S, NS>(m + (int64_t)k * n_scalars + sk);
        acc[k] = (V)(S)0;                                                                 // m_k .= 0 (1042)
    }
    int64_t i = 0, iend = nrow;
    if (part_out) {
        i = (int64_t)blockIdx.y * rows_per_part;
        iend = iend < i + rows_per_part ? iend : i + rows_per_part;
    }
    // block (i, k) = blocks[i + k * nrow] (column-major table); the next batch's pointers are requested while this batch's packs are in flight
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
        V c[DEPTH][K];
#pragma unroll
        for (int j = 0; j < DEPTH; j++)
#pragma unroll
            for (int k = 0; k < K; k++) c[j][k] = ldu<NT, S, NS>(a[j][k] + sk);
#pragma unroll
        for (int j = 0; j < DEPTH; j++) {
            V t = (V)(S)0;                                                                // zeros(range(A)) (531)
#pragma unroll
            for (int k = 0; k < K; k++) t = t + vmul<S, E, NS, V>(c[j][k], x[k], false);  // d_i .+= A_ik m_k (1024)
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(c[j][k], t, true);   // m_k .+= A_ik' d_i (1049)
        }
    }
    for (; i < iend; i++) {
        V c[K];
#pragma unroll
        for (int k = 0; k < K; k++) c[k] = ldu<NT, S, NS>((const S *)blocks[i + (int64_t)k * nrow].coeff + sk);
        V t = (V)(S)0;
#pragma unroll
        for (int k = 0; k < K; k++) t = t + vmul<S, E, NS, V>(c[k], x[k], false);
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] = acc[k] + vmul<S, E, NS, V>(c[k], t, true);
    }
    if (!ok) return;
    S *o = part_out ? part_out + (int64_t)blockIdx.y * (K * n_scalars) : y;
#pragma unroll
    for (int k = 0; k < K; k++) st_pack<false, S, NS>(o + (int64_t)k * n_scalars, s0, sk, acc[k]);
}

// rows in flight: K x DEPTH = 8 (6 for K = 3) coefficient packs per lane; 12 / 9 / 12 measured 2-3 % slower for K = 2 / 4 and within the noise for
// K = 3 (profiles/bench_grid_normal_r06.txt)
template <int K> struct grid_normal_depth { static constexpr int value = K == 2 ? 4 : 2; };

// plain diagonals through the block table, or (MIXED) any grid through the packed one
template <typename S, int E, int NS, int K, bool MIXED> auto pick_grid_normal(bool nt)
{
    constexpr int D = grid_normal_depth<K>::value;
    if constexpr (MIXED) {
        using P = Picked<decltype(&k_grid_normal_mixed<S, E, NS, K, D, false>)>;
        return nt ? P{&k_grid_normal_mixed<S, E, NS, K, D, true>, 256, 1, D} : P{&k_grid_normal_mixed<S, E, NS, K, D, false>, 256, 1, D};
    } else {
        using P = Picked<decltype(&k_grid_normal<S, E, NS, K, D, false>)>;
        return nt ? P{&k_grid_normal<S, E, NS, K, D, true>, 256, 1, D} : P{&k_grid_normal<S, E, NS, K, D, false>, 256, 1, D};
    }
}

template <typename S, int E, int NS, int K>
int launch_grid_normal(const jh_blockop *op, void *y, const void *m, int64_t first_elem, int64_t end_elem)
{
    jh_context &c = jh_ctx();
    const GridPlan p = grid_plan(op, E, NS, first_elem, end_elem);
    S *slabs = nullptr;
    JH_TRY(grid_slabs(p, K, y, &slabs));
    c.last_adj_parts = p.parts;
    c.last_adj_launches = 1;
    const bool nt = jh_stream_nt((double)op->nrow * (double)K * (double)p.n_scalars * sizeof(S));   // (a range too: the whole pass's bytes)
    if (p.ranged) c.last_grid_range_shape = (nt ? 1 : 0) | (p.parts > 1 ? 2 : 0);
    auto launch = [&](auto k, auto... table) {
        hipLaunchKernelGGL(k.k, dim3((unsigned)p.gx, (unsigned)p.parts), dim3(k.blk), 0, c.stream, op->dev_blocks, table..., op->nrow, p.n_scalars, (const S *)m,
                           (S *)y, p.rows_per_part, slabs, p.s_begin, p.s_end);
    };
    // (the packed table for grids of plain diagonals too: within the noise of this kernel, profiles/bench_grid_normal_r06.txt)
    if (!op->all_diag) launch(pick_grid_normal<S, E, NS, K, true>(nt), (const uint64_t *)op->grid_words);
    else launch(pick_grid_normal<S, E, NS, K, false>(nt));
    JH_CHECK_HIP(hipGetLastError());
    return grid_fold(p, K, slabs, y);
}

}  // namespace

namespace jhb {

// an N x K grid (N >= 2, K = 2 .. 4) of equal blocks of >= 16 bytes -- plain diagonals, or (mixed_ok) zero / identity / scalar / diagonal blocks, no
// nonlinear child --, coefficients aligned like their scalar
bool grid_shape_ok(const jh_blockop *op, bool mixed_ok)
{
    if (!(op->nrow >= 2 && op->ncol >= 2 && op->ncol <= 4 && op->uniform_rows)) return false;
    if (!op->all_diag) {
        if (!mixed_ok || !op->elementwise || op->nonlinear || op->wide_scale) return false;
        for (const jh_block_desc &b : op->blocks)
            if (b.kind != JH_OP_ZERO && b.kind != JH_OP_IDENTITY && b.kind != JH_OP_SCALE && b.kind != JH_OP_DIAG) return false;
    }
    const size_t es = jh_dtype_size(op->dtype);
    const int64_t n = op->row_len[0];
    if (n * (int64_t)es < 16) return false;
    for (int64_t v : op->col_len)
        if (v != n) return false;
    return op->coeff_scalar_aligned;
}

// the grids above (knob grid_normal = 1: later in round 6, grids of several kinds), vectors aligned like their scalar
bool grid_normal_ok(const jh_blockop *op, const void *y, const void *m)
{
    const int64_t knob = jh_ctx().grid_normal;
    if (knob == 0 || !grid_shape_ok(op, knob != 2)) return false;
    return vectors_scalar_aligned(op->dtype, y, m);
}

int grid_words_ensure(const jh_blockop *op)
{
    if (op->all_diag || op->grid_words) return JH_OK;
    if (stream_is_capturing(jh_ctx().stream))                 // (an allocation and a synchronous copy: not inside a stream capture -- the caller chains the two stages)
        return jh_fail(JH_ERR_UNSUPPORTED, "grid kernels: the block table of this operator is built on the first call, which must not be inside a stream capture");
    const size_t nw = (size_t)op->nrow * (size_t)op->ncol;
    std::vector<uint64_t> h(nw);
    for (int64_t i = 0; i < op->nrow; i++)
        for (int64_t k = 0; k < op->ncol; k++) {
            const jh_block_desc &b = op->blocks[(size_t)(i + k * op->nrow)];
            const jh_dev_block db = jh_dev_block_of(b);
            const uint64_t p = (uint64_t)(uintptr_t)(b.kind == JH_OP_DIAG ? b.coeff : nullptr);
            JH_REQUIRE((p >> 48) == 0, "grid kernels: a coefficient address does not fit 48 bits");
            h[(size_t)(i * op->ncol + k)] = p | ((uint64_t)(b.kind & 7) << 48) | ((uint64_t)(b.adjoint ? 1 : 0) << 51) | ((uint64_t)(db.real_scale ? 1 : 0) << 52);
        }
    void *dev = nullptr;
    JH_CHECK_HIP(hipMalloc(&dev, nw * sizeof(uint64_t)));
    const hipError_t e = hipMemcpy(dev, h.data(), nw * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dev); JH_CHECK_HIP(e); }
    op->grid_words = dev;
    return JH_OK;
}

static int grid_normal_by_dtype(const jh_blockop *op, void *y, const void *m, int64_t first_elem, int64_t end_elem)
{
    JH_TRY(grid_words_ensure(op));                            // the packed table of a mixed grid, row-major (N x K words), built on first use
    return jh_by_dtype(op->dtype, "grid_normal", [&](auto t) {
        using T = decltype(t);
        return grid_by_k(op->ncol, [&](auto k) { return launch_grid_normal<typename T::S, T::E, T::NS, decltype(k)::value>(op, y, m, first_elem, end_elem); });
    });
}

int grid_normal(const jh_blockop *op, void *y, const void *m) { return grid_normal_by_dtype(op, y, m, 0, -1); }

// positions [first_elem, first_elem + count) of every block (jh_blockop_normal_mul_range, knob grid_range; the caller has checked grid_range_ok and
// grid_range_bounds): the same kernels over those lanes -- the K pieces y_k[first, first + count) and nothing else
int grid_normal_range(const jh_blockop *op, void *y, const void *m, int64_t first_elem, int64_t count)
{
    return grid_normal_by_dtype(op, y, m, first_elem, first_elem + count);
}

}  // namespace jhb
